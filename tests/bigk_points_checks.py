"""The checks of mmg_selftest_bigk_points: the three shortcuts of the conditional-binomial chain's kernel (k_sample_bigk) at their decision
boundaries -- the STEP bound binv_zero_bound, the fp32 inversion binv_pretest and the fp32 acceptance test btrs_pretest (mmg_math.h).
Written once: tests/test_bigk_points.py runs the host instantiation (device -1, no GPU), tests/test_gpu_bigk_points.py the kernels.

Random (n, p, uniform) meet a boundary of the cumulative sum, or the acceptance threshold, with a probability of the order of the fp32
bounds themselves.  Here the boundaries of the fp64 code are FOUND, by bisection on the host instantiation over a structured grid of
(n, p), and the inputs are placed on and around them: the boundary itself, 1-3 ulps and 2^-8 ... 2^-40 to either side, and the two uniforms
of the row stream (u32_unit) that bracket it.  The high-precision reference is Python's decimal at 80 digits: a double converts to it
exactly."""
import decimal
from decimal import Decimal

import numpy as np

CTX = decimal.Context(prec=80)
U_MAX = 1.0 - 2.0 ** -20      # no inversion point lies above it: the fp64 search on a uniform closer to 1 may walk a tail of n terms
X_MAX = 300                   # and the host's search ends within this many terms on every point that goes to a device

N_GRID = sorted({1, 2, 3, 9, 10, 11, 19, 20, 21, 63, 64, 65, 2 ** 32 - 1} | {2 ** k + d for k in (8, 12, 16, 20, 24, 28, 31) for d in (-1, 0, 1)})
NP_LADDER = [1e-6, 3e-6, 1e-5, 1e-4, 1e-3, 0.01, 0.03, 0.06, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 9.5, 9.8,
             9.9, 9.99, 9.999]
TINY_P = [2.0 ** -54, 2.0 ** -53, 1e-300]                   # 1 - p rounds to 1 (2^-53: to the double below 1)
REL_E = list(range(8, 41))                                  # offsets u (1 +- 2^-e)
STRATA = [(21, 2 ** 12), (2 ** 12, 2 ** 24), (2 ** 24, 2 ** 32)]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _of_bits(b):
    return np.ascontiguousarray(b, np.int64).view(np.float64)


def _cases(rows, limit=12):
    rows = list(rows)
    return "%d cases, the first: %s" % (len(rows), "; ".join(str(r) for r in rows[:limit]))


# ----------------------------------------------------------------------------------------------------------------- inversion: the grid
def inversion_grid():
    g = []
    for n in N_GRID:
        for npv in NP_LADDER:
            p = npv / n
            if p <= 0.5 and float(n) * p < 10.0:
                g.append((n, p))
        g += [(n, p) for p in TINY_P]
        if n <= 19:
            g.append((n, 0.5))
    return sorted(set(g))


def exact_cdf(n, p, as_searched=True):
    """C_0 .. C_(K+1) at 80 digits, C_K <= U_MAX < C_(K+1) (the last one may be C_n).  as_searched: of the sum the fp64 search forms,
    C_k = q^n sum_(x <= k) binom(n, x) (p / q)^x with q the DOUBLE 1 - p the search starts from -- its terms in exact arithmetic; otherwise of
    Binomial(n, p) itself, q = 1 - p exactly.  The two differ by up to n 2^-54 (the rounding of 1 - p), 2^-22 at n = 2^32."""
    with decimal.localcontext(CTX):
        P = Decimal(p)
        Q = Decimal(1.0 - p) if as_searched else 1 - P
        ratio = P / Q
        r = Q ** n
        c, k, out = r, 0, [r]
        lim = Decimal(U_MAX)
        while c <= lim and k < n:
            r = r * (n - k) / (k + 1) * ratio
            k += 1
            c = c + r
            out.append(c)
        return out


class Inversion:
    """grid: (n, p); cdf[g]: the exact C_k; cf[g]: rounded to double; bnd[g]: the fp64 code's boundaries u_k (the largest double with
    out_x == k), NaN where the bisection's bracket [C_k (1 - 2^-30), min(C_k (1 + 2^-30), U_MAX)] does not hold one;
    pts: the adversarial points n, p, u with their grid index g; host: the host instantiation's outputs on them"""


def _host_x(gibbs, n, p, u):
    x = gibbs.selftest_bigk_inversion(n, p, u, device=-1)["x"]
    assert (x >= 0).all() and (x <= X_MAX).all(), "host search left [0, %d]" % X_MAX
    return x


def _u32_bracket(gibbs, u):
    """the two uniforms of the row stream (u32_unit of consecutive words) around u, through the words part of mmg_selftest_keyed"""
    w = np.clip(np.floor(u * 2.0 ** 32 - 0.5), 0, 2 ** 32 - 2).astype(np.uint32)
    lo = gibbs.selftest_keyed_words(w, 0, 1.0, device=-1)["u32"]
    hi = gibbs.selftest_keyed_words(w + np.uint32(1), 0, 1.0, device=-1)["u32"]
    return lo, hi


def _around(c, ulps=3, rel=REL_E, wide=()):
    """[len(c), offsets]: c itself, +-1..ulps ulps, c (1 +- 2^-e), c 2^+-j"""
    b = _bits(c)
    cols = [c]
    for j in range(1, ulps + 1):
        cols += [_of_bits(b + j), _of_bits(b - j)]
    for e in rel:
        cols += [c * (1.0 + 2.0 ** -e), c * (1.0 - 2.0 ** -e)]
    for j in wide:
        cols += [c * 2.0 ** j, c * 2.0 ** -j]
    return np.stack(cols, axis=1)


_CACHE = {}


def inversion(gibbs):
    if "inv" in _CACHE:
        return _CACHE["inv"]
    I = Inversion()
    I.grid = inversion_grid()
    I.cdf = [exact_cdf(n, p) for n, p in I.grid]
    I.cf = [np.array([float(c) for c in cs]) for cs in I.cdf]
    I.cdf_bin = [exact_cdf(n, p, as_searched=False) for n, p in I.grid]
    # (a) the boundaries of the fp64 search: every (g, k) with C_k <= U_MAX
    g = np.concatenate([np.full(len(c) - 1, i) for i, c in enumerate(I.cf)]).astype(np.int64)
    k = np.concatenate([np.arange(len(c) - 1) for c in I.cf]).astype(np.int64)
    c = np.concatenate([cf[:-1] for cf in I.cf])
    n = np.array([I.grid[i][0] for i in g], np.uint32)
    p = np.array([I.grid[i][1] for i in g])
    lo, hi = c * (1.0 - 2.0 ** -30), np.minimum(c * (1.0 + 2.0 ** -30), U_MAX)
    ok = lo < hi
    g, k, c, n, p, lo, hi = [a[ok] for a in (g, k, c, n, p, lo, hi)]
    x_lo, x_hi = _host_x(gibbs, n, p, lo), _host_x(gibbs, n, p, hi)
    bad = np.nonzero(x_lo > k)[0]
    assert bad.size == 0, "the fp64 search passes k more than 2^-30 below the exact C_k: " + _cases((n[i], p[i], k[i], lo[i], x_lo[i]) for i in bad)
    ok = x_hi > k                                              # (a C_k within 2^-30 of U_MAX may keep its boundary above the cap: left out)
    g, k, c, n, p, lo, hi = [a[ok] for a in (g, k, c, n, p, lo, hi)]
    bl, bh = _bits(lo).copy(), _bits(hi).copy()                 # positive doubles order like their bit patterns
    steps = 0
    while (bh - bl > 1).any():
        mid = bl + (bh - bl) // 2
        le = _host_x(gibbs, n, p, _of_bits(mid)) <= k
        bl, bh = np.where(le, mid, bl), np.where(le, bh, mid)
        steps += 1
        assert steps <= 53
    uk = _of_bits(bl)
    assert same(_host_x(gibbs, n, p, uk), k) and same(_host_x(gibbs, n, p, _of_bits(bl + 1)), k + 1)
    I.bnd = [np.full(len(cf), np.nan) for cf in I.cf]
    for gi, ki, u in zip(g, k, uk):
        I.bnd[gi][ki] = u
    I.b_g, I.b_k, I.b_u, I.b_n, I.b_p = g, k, uk, n, p
    # (b) the adversarial points
    pts = _around(uk)
    w_lo, w_hi = _u32_bracket(gibbs, uk)
    pts = np.concatenate([pts, w_lo[:, None], w_hi[:, None]], axis=1)
    pg = np.repeat(g, pts.shape[1])
    pu = pts.ravel()
    # ... and the STEP bound of every grid point as a uniform, where it is one
    gn = np.array([q[0] for q in I.grid], np.uint32)
    gp = np.array([q[1] for q in I.grid])
    I.g_bound = gibbs.selftest_bigk_inversion(gn, gp, 0.5, device=-1)["bound"]
    pg = np.concatenate([pg, np.arange(len(I.grid))])
    pu = np.concatenate([pu, I.g_bound])
    keep = (pu > 0.0) & (pu <= U_MAX)
    pg, pu = pg[keep], pu[keep]
    order = np.lexsort((pu, pg))
    pg, pu = pg[order], pu[order]
    first = np.concatenate([[True], (pg[1:] != pg[:-1]) | (pu[1:] != pu[:-1])])
    I.p_g, I.p_u = pg[first], pu[first]
    I.p_n, I.p_p = gn[I.p_g], gp[I.p_g]
    I.host = gibbs.selftest_bigk_inversion(I.p_n, I.p_p, I.p_u, device=-1)
    for a in (I.p_g, I.p_u, I.p_n, I.p_p, *I.host.values()):
        a.setflags(write=False)
    _CACHE["inv"] = I
    return I


def check_inversion_inputs(gibbs):
    """the condition on the inputs, on the host, before anything goes to a device"""
    I = inversion(gibbs)
    assert I.p_u.size > 200_000 and (I.p_u > 0.0).all() and (I.p_u <= U_MAX).all()
    assert (I.host["x"] >= 0).all() and (I.host["x"] <= X_MAX).all()
    assert (I.host["pre"] == -1).all()                          # the host has no fp32 search
    assert (I.p_n >= 1).all() and (I.p_p > 0).all() and (I.p_p <= 0.5).all() and (I.p_n.astype(np.float64) * I.p_p < 10.0).all()
    # the grid is what it is meant to be: boundaries at every n, tiny p, p = 1/2, x beyond 20
    assert set(int(v) for v in I.b_n) == set(N_GRID) and I.b_k.max() >= 25 and (I.b_p == 0.5).any()
    assert I.b_u.size > 5000
    return I


# ----------------------------------------------------------------------------------------------------------------- inversion: the CPU's assertions
def check_step_bound_settles_zero(gibbs):
    """out_x == 0 at u = out_bound wherever the bound is a uniform: what k_sample_bigk relies on.  (The search ends at once where that
    holds: these points may lie above U_MAX on the host.)"""
    I = inversion(gibbs)
    gn = np.array([q[0] for q in I.grid], np.uint32)
    gp = np.array([q[1] for q in I.grid])
    pos = (I.g_bound > 0.0) & (I.g_bound < 1.0)
    assert pos.sum() > 500 and (I.g_bound < 1.0).all()
    x = gibbs.selftest_bigk_inversion(gn[pos], gp[pos], I.g_bound[pos], device=-1)["x"]
    bad = np.nonzero(x != 0)[0]
    assert bad.size == 0, "x != 0 at u = binv_zero_bound: " + _cases((gn[pos][i], gp[pos][i], I.g_bound[pos][i], x[i]) for i in bad)


def check_step_bound_below_exact_r0(gibbs):
    """out_bound <= (1 - p)^n at 80 digits -- with 1 - p exact, and with the double the search starts from"""
    I = inversion(gibbs)
    for cdf in (I.cdf_bin, I.cdf):
        bad = [(n, p, b, float(cs[0])) for (n, p), b, cs in zip(I.grid, I.g_bound, cdf) if Decimal(float(b)) > cs[0]]
        assert not bad, "binv_zero_bound above (1 - p)^n: " + _cases(bad)


def check_step_claim(gibbs):
    """the comment's claim r0 >= 1 - n p - n 2^-54 - 2^-46 on the fp64 code's own r0: u_0, the largest uniform with x = 0, is r0 (or the
    largest double below 1).  Where u_0 was bisected it is compared; where (1 - p)^n lies above U_MAX it is probed: x = 0 at the smallest
    double that is not below the claim's right-hand side.  Returns (the smallest u_0 - bound, its n, p)."""
    I = inversion(gibbs)
    worst, bad, probe, above = None, [], [], []
    with decimal.localcontext(CTX):
        for gi, (n, p) in enumerate(I.grid):
            claim = 1 - n * Decimal(p) - n * Decimal(2) ** -54 - Decimal(2) ** -46
            # the chain of the argument: binv_zero_bound <= the derived bound (here) <= r0 (below).  Bernoulli's inequality alone leaves
            # (n p)^2 / 2 of room, so a bound without its margins still passes the checks against r0 itself: this one it does not
            if Decimal(float(I.g_bound[gi])) > claim:
                above.append((n, p, float(I.g_bound[gi]), float(claim)))
            u0 = I.bnd[gi][0]
            if u0 == u0:
                if Decimal(float(u0)) < claim:
                    bad.append((n, p, float(u0), float(claim)))
                gap = float(u0) - float(I.g_bound[gi])
                if worst is None or gap < worst[0]:
                    worst = (gap, n, p)
            elif claim > 0:
                u = float(claim)
                if Decimal(u) < claim:
                    u = float(np.nextafter(u, 2.0))
                assert 0.0 < u < 1.0
                probe.append((n, p, u))
    assert not above, "binv_zero_bound above the bound the comment derives: " + _cases(above)
    assert not bad, "u_0 below the bound the comment derives: " + _cases(bad)
    assert len(probe) >= 3 * len(N_GRID) - 8
    x = gibbs.selftest_bigk_inversion([q[0] for q in probe], [q[1] for q in probe], [q[2] for q in probe], device=-1)["x"]
    badp = [q + (int(v),) for q, v in zip(probe, x) if v != 0]
    assert not badp, "x != 0 at the bound the comment derives: " + _cases(badp)
    assert worst[0] > 0.0
    return worst


def _truth(I, cdfs, extra):
    """points farther than 2^-40 (k + 1) + extra[g] from every C_k of cdfs[g]; the x of that CDF on every point"""
    want = np.empty(I.p_u.size, np.int64)
    far = np.empty(I.p_u.size, bool)
    start = np.searchsorted(I.p_g, np.arange(len(I.grid) + 1))
    sliver = 2.0 ** -50                # (the distances are formed in fp64, good to 2^-52: inside the sliver decimal decides)
    for gi, cs in enumerate(cdfs):
        cf = np.array([float(c) for c in cs])
        s = slice(start[gi], start[gi + 1])
        u = I.p_u[s]
        want[s] = np.searchsorted(cf, u, side="left")               # the smallest x with u <= C_x
        margin = np.abs(u[:, None] - cf[None, :]) - (2.0 ** -40 * (np.arange(cf.size) + 1.0) + extra[gi])[None, :]
        f = (margin > 0).all(axis=1)
        for j in np.nonzero((np.abs(margin) <= sliver).any(axis=1))[0]:
            with decimal.localcontext(CTX):
                f[j] = all(abs(Decimal(float(u[j])) - c) > Decimal(2) ** -40 * (kk + 1) + Decimal(float(extra[gi])) for kk, c in enumerate(cs))
        far[s] = f
    return far, want


def check_inversion_truth(gibbs):
    """Away from every exact boundary (farther than 2^-40 (k + 1) from C_k) the fp64 search finds the x of the exact CDF: the search is
    right wherever rounding cannot matter.  The exact CDF is that of the search's own sum, which starts from the double q = 1 - p
    (exact_cdf); against Binomial(n, p) with 1 - p exact, the rounding of q moves every boundary by up to n 2^-54 (the term of the STEP
    comment; 2.4e-7 = n 2^-54 at n = 2^32 - 1, p = 2^-54, where the double is 1), so there the distance is 2^-40 (k + 1) + n 2^-54."""
    I = inversion(gibbs)
    far, want = _truth(I, I.cdf, np.zeros(len(I.grid)))
    assert far.sum() > I.p_u.size // 3
    bad = np.nonzero(far & (I.host["x"] != want))[0]
    assert bad.size == 0, "fp64 search differs from its exact CDF away from the boundaries: " + _cases(
        (I.p_n[i], I.p_p[i], I.p_u[i], I.host["x"][i], want[i]) for i in bad)
    far_b, want_b = _truth(I, I.cdf_bin, np.array([n * 2.0 ** -54 for n, _ in I.grid]))
    assert far_b.sum() > I.p_u.size // 3
    bad = np.nonzero(far_b & (I.host["x"] != want_b))[0]
    assert bad.size == 0, "fp64 search differs from the CDF of Binomial(n, p) by more than the rounding of 1 - p: " + _cases(
        (I.p_n[i], I.p_p[i], I.p_u[i], I.host["x"][i], want_b[i]) for i in bad)
    shift = max((abs(float(a - b)), n, p) for (n, p), ca, cb in zip(I.grid, I.cdf, I.cdf_bin) for a, b in zip(ca, cb))
    return int(far.sum()), int(far_b.sum()), int(I.p_u.size), shift


# ----------------------------------------------------------------------------------------------------------------- BTRS
def btrs_constants(n, p):
    dn = n.astype(np.float64)
    qq = 1.0 - p
    spq = np.sqrt(dn * p * qq)
    bb = 1.15 + 2.53 * spq
    aa = -0.0873 + 0.0248 * bb + 0.01 * p
    cc = dn * p + 0.5
    vr = 0.92 - 4.2 / bb
    return dn, spq, aa, bb, cc, vr


def btrs_try(n, p, u, v):
    """BSET and TRY of k_sample_bigk in numpy: IEEE operations and sqrt only, rounded once each like the library's"""
    dn, spq, aa, bb, cc, vr = btrs_constants(n, p)
    uu = u - 0.5
    us = 0.5 - np.abs(uu)
    with np.errstate(divide="ignore", invalid="ignore"):
        kf = np.floor((2.0 * aa / us + bb) * uu + cc)
    reach = np.where((kf < 0.0) | (kf > dn), 0, np.where((us >= 0.07) & (v <= vr), 1, 2)).astype(np.int32)
    return kf, reach, us


def btrs_grid():
    g = []
    for n in N_GRID:
        if n < 21:
            continue
        lo = 10.0 / n
        while float(n) * lo < 10.0:
            lo = float(np.nextafter(lo, 1.0))
        ps = set(float(v) for v in np.exp(np.linspace(np.log(lo), np.log(0.5), 8)))
        ps |= {lo, 0.4, 0.45, 0.49, 0.5}
        g += [(n, p) for p in sorted(ps) if lo <= p <= 0.5 and float(n) * p >= 10.0]
    return g


def _u_for_candidate(n, p, k):
    """the first uniform whose candidate is k (bisection on the restated, increasing map u -> (2 a / us + b) (u - 1/2) + c at k + 1/2)"""
    dn, spq, aa, bb, cc, vr = btrs_constants(n, p)
    lo, hi = np.full(n.size, 2.0 ** -40), np.full(n.size, 1.0 - 2.0 ** -40)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        uu = mid - 0.5
        val = (2.0 * aa / (0.5 - np.abs(uu)) + bb) * uu + cc
        below = val < k + 0.5
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return lo


class Btrs:
    """cases: n, p, u with the largest accepted second uniform v* (bisected on the host instantiation); pts: the points around it"""


def btrs(gibbs):
    if "btrs" in _CACHE:
        return _CACHE["btrs"]
    B = Btrs()
    grid = btrs_grid()
    cn, cp, cu = [], [], []
    for n, p in grid:
        m = np.floor((n + 1.0) * p)
        sd = np.sqrt(n * p * (1.0 - p))
        ks = {m, m - 1, m + 1, np.floor(m - 3 * sd), np.floor(m + 3 * sd), np.floor(m - 6 * sd), np.floor(m + 6 * sd), 0.0, float(n)}
        ks = sorted(k for k in ks if 0.0 <= k <= n)
        nn, pp = np.full(len(ks), n, np.uint32), np.full(len(ks), p)
        us = list(_u_for_candidate(nn, pp, np.array(ks)))
        # us = 1/2 - |u - 1/2| just below and just above the squeeze's 0.07
        us += [0.07, float(np.nextafter(0.07, 0)), float(np.nextafter(0.07, 1)), 0.07 - 1e-9, 0.07 + 1e-9,
               0.93, float(np.nextafter(0.93, 0)), float(np.nextafter(0.93, 1)), 0.93 - 1e-9, 0.93 + 1e-9]
        cn += [n] * len(us); cp += [p] * len(us); cu += us
    cn, cp, cu = np.array(cn, np.uint32), np.array(cp), np.array(cu)
    kf, reach, us = btrs_try(cn, cp, cu, np.full(cn.size, 0.999))
    B.all_n, B.all_p, B.all_u = cn, cp, cu
    assert ((us >= 0.07) & (us < 0.0701)).any() and ((us < 0.07) & (us > 0.0699)).any()
    assert (kf == 0).any() and (kf == cn).any() and (kf == np.floor((cn + 1.0) * cp)).any()
    ok = reach != 0
    cn, cp, cu = cn[ok], cp[ok], cu[ok]

    def accepted(v):
        r = gibbs.selftest_bigk_btrs(cn, cp, cu, v, device=-1)
        return (r["reach"] == 1) | ((r["reach"] == 2) & (r["exact"] == 1))
    bl = _bits(np.full(cn.size, 2.0 ** -33)).copy()
    bh = _bits(np.full(cn.size, 1.0 - 2.0 ** -53)).copy()
    ok = accepted(_of_bits(bl)) & ~accepted(_of_bits(bh))
    while (bh - bl > 1)[ok].any():
        mid = bl + (bh - bl) // 2
        acc = accepted(_of_bits(mid))
        bl, bh = np.where(acc, mid, bl), np.where(acc, bh, mid)
    vs = _of_bits(bl)
    at = gibbs.selftest_bigk_btrs(cn, cp, cu, vs, device=-1)
    ok &= (vs > 2.0 ** -32) & (vs < 1.0) & (at["reach"] == 2)          # (a v* inside the squeeze's range is the squeeze's, not the test's)
    B.n, B.p, B.u, B.vstar = cn[ok], cp[ok], cu[ok], vs[ok]
    pts = _around(B.vstar, rel=list(range(1, 41)), wide=(1, 2, 3, 4))
    w = pts.shape[1]
    pn, pp, pu, pv = np.repeat(B.n, w), np.repeat(B.p, w), np.repeat(B.u, w), pts.ravel()
    keep = (pv > 0.0) & (pv < 1.0)
    B.p_n, B.p_p, B.p_u, B.p_v = pn[keep], pp[keep], pu[keep], pv[keep]
    B.host = gibbs.selftest_bigk_btrs(B.p_n, B.p_p, B.p_u, B.p_v, device=-1)
    for a in (B.p_n, B.p_p, B.p_u, B.p_v, *B.host.values()):
        a.setflags(write=False)
    _CACHE["btrs"] = B
    return B


def check_btrs_host(gibbs):
    """out_exact == (out_diff >= 0); out_reach and out_kf equal the restatement -- on the points around v* and on every (n, p, u) of the
    grid, the candidates outside [0, n] included"""
    B = btrs(gibbs)
    assert B.n.size > 1500 and B.p_v.size > 100_000
    for lo, hi in STRATA:
        s = (B.n >= lo) & (B.n < hi)
        assert s.sum() > 100 and (B.p[s] == 0.5).any(), (lo, hi)
    assert ((B.n >= 2 ** 24) & (B.p >= 0.4)).sum() > 100              # p in [0.4, 0.5] at n >= 2^24
    for n, p, u, v, got in ((B.p_n, B.p_p, B.p_u, B.p_v, B.host),
                            (B.all_n, B.all_p, B.all_u, np.full(B.all_n.size, 0.75), None), (B.all_n, B.all_p, B.all_u, np.full(B.all_n.size, 2.0 ** -20), None)):
        if got is None:
            got = gibbs.selftest_bigk_btrs(n, p, u, v, device=-1)
        kf, reach, _ = btrs_try(n, p, u, v)
        bad = np.nonzero((got["kf"] != kf) | (got["reach"] != reach))[0]
        assert bad.size == 0, "candidate or reach differ from the restatement: " + _cases((n[i], p[i], u[i], v[i], got["kf"][i], kf[i], got["reach"][i], reach[i]) for i in bad)
        r2 = got["reach"] == 2
        assert set(np.unique(got["reach"])) <= {0, 1, 2} and r2.any()
        bad = np.nonzero(r2 & (got["exact"] != (got["diff"] >= 0)))[0]
        assert bad.size == 0, "exact test and its difference disagree: " + _cases((n[i], p[i], u[i], v[i], got["exact"][i], got["diff"][i]) for i in bad)
        assert (got["exact"][~r2] == -1).all() and (got["diff"][~r2] == 0).all()
        assert (got["pre"] == 0).all() and (got["d32"] == 0).all() and (got["e32"] == 0).all()       # the host has no fp32 estimate
    # v* is a boundary of the fp64 test
    a = gibbs.selftest_bigk_btrs(B.n, B.p, B.u, B.vstar, device=-1)
    b = gibbs.selftest_bigk_btrs(B.n, B.p, B.u, _of_bits(_bits(B.vstar) + 1), device=-1)
    assert (a["exact"] == 1).all() and (b["exact"] == 0).all()


# ----------------------------------------------------------------------------------------------------------------- the device
def e_x(c, x):
    """binv_pretest's bound on the fp32 cumulative sum c~_x (mmg_math.h)"""
    return c * (2.0 ** -14 + x * 2.0 ** -19) + 2.0 ** -22


class Device:
    pass


def device_run(gibbs, device):
    """everything the device checks look at, computed once: the input conditions first, on the host"""
    key = ("dev", device)
    if key in _CACHE:
        return _CACHE[key]
    I = check_inversion_inputs(gibbs)
    B = btrs(gibbs)
    D = Device()
    D.inv = gibbs.selftest_bigk_inversion(I.p_n, I.p_p, I.p_u, slack=1.0, device=device)
    D.btrs = gibbs.selftest_bigk_btrs(B.p_n, B.p_p, B.p_u, B.p_v, device=device)
    _CACHE[key] = D
    return D


def check_device_fp64_equals_host(gibbs, device):
    I, B, D = inversion(gibbs), btrs(gibbs), device_run(gibbs, device)
    def differ(a, b):                                            # bit for bit: -0.0 is not 0.0, a NaN equals only its own pattern
        assert a.dtype == b.dtype and a.shape == b.shape
        return np.nonzero((_bits(a) != _bits(b)) if a.dtype == np.float64 else (a != b))[0]
    for k in ("bound", "x"):
        bad = differ(D.inv[k], I.host[k])
        assert bad.size == 0, "inversion %s differs from the host: " % k + _cases((I.p_n[i], I.p_p[i], I.p_u[i], D.inv[k][i], I.host[k][i]) for i in bad)
    for k in ("kf", "reach", "exact", "diff"):
        bad = differ(D.btrs[k], B.host[k])
        assert bad.size == 0, "BTRS %s differs from the host: " % k + _cases((B.p_n[i], B.p_p[i], B.p_u[i], B.p_v[i], D.btrs[k][i], B.host[k][i]) for i in bad)


def check_device_binv_pretest(gibbs, device):
    """slack 1: a decided point equals the fp64 search (and none is decided where that fell short); the points the bound leaves room
    for ARE decided.  Returns (decided, points, assessed for non-vacuity)."""
    I, D = inversion(gibbs), device_run(gibbs, device)
    pre, x = D.inv["pre"], I.host["x"]
    bad = np.nonzero((pre != -1) & (pre != x))[0]
    assert bad.size == 0, "binv_pretest decides differently from the fp64 search, (n, p, u, pre, x): " + _cases((I.p_n[i], I.p_p[i], I.p_u[i], pre[i], x[i]) for i in bad)
    assert (pre >= -1).all() and not ((pre >= 0) & (x == -1)).any()
    # non-vacuity: 8 e_x of room to both neighbouring boundaries of the fp64 code (the exact C_k where that one was not bisected)
    room = np.zeros(x.size, bool)
    start = np.searchsorted(I.p_g, np.arange(len(I.grid) + 1))
    for gi, (cf, bnd) in enumerate(zip(I.cf, I.bnd)):
        s = slice(start[gi], start[gi + 1])
        b = np.where(np.isnan(bnd), cf, bnd)
        u, xs = I.p_u[s], x[s]
        hi = b[np.minimum(xs, b.size - 1)]
        lo = np.where(xs > 0, b[np.maximum(xs - 1, 0)], 0.0)
        r = (xs <= 40) & (xs < b.size) & (hi - u >= 8 * e_x(hi, xs))
        r &= (xs == 0) | (u - lo >= 8 * e_x(lo, xs - 1))
        room[s] = r
    assert room.sum() > x.size // 50
    bad = np.nonzero(room & (pre < 0))[0]
    assert bad.size == 0, "undecided with 8 e_x of room: the fp32 sum erred by more than its bound, (n, p, u, x): " + _cases((I.p_n[i], I.p_p[i], I.p_u[i], x[i]) for i in bad)
    und = pre < 0
    assert und.sum() > I.b_u.size                                 # and the points at the boundaries are left to the fp64 search
    return int((pre >= 0).sum()), int(x.size), int(room.sum())


def check_device_btrs_pretest(gibbs, device):
    """a decided test equals the fp64 test; the estimate's error is within its bound on EVERY reach-2 point; every stratum of n holds
    decided-accept, decided-reject and undecided points.  Returns the largest |d32 - diff| / e32 per stratum with its case."""
    B, D = btrs(gibbs), device_run(gibbs, device)
    pre, r2, exact, diff = D.btrs["pre"], B.host["reach"] == 2, B.host["exact"], B.host["diff"]
    d32, e32 = D.btrs["d32"].astype(np.float64), D.btrs["e32"].astype(np.float64)
    assert (pre[~r2] == 0).all() and set(np.unique(pre)) <= {-1, 0, 1}

    def case(i):
        return (B.p_n[i], B.p_p[i], B.p_u[i], B.p_v[i], "kf", B.host["kf"][i], "pre", pre[i], "exact", exact[i], "diff", diff[i], "d32", d32[i], "e32", e32[i])
    bad = np.nonzero(r2 & (pre != 0) & ((pre > 0) != (exact == 1)))[0]
    assert bad.size == 0, "btrs_pretest decides differently from the fp64 test: " + _cases(case(i) for i in bad)
    assert np.isfinite(d32[r2]).all() and (e32[r2] > 0).all()
    share = np.where(r2, np.abs(d32 - diff) / np.where(r2, e32, 1.0), 0.0)
    bad = np.nonzero(share > 1.0)[0]
    assert bad.size == 0, "the fp32 estimate errs by more than its bound: " + _cases(case(i) for i in bad)
    worst = []
    for lo, hi in STRATA:
        s = r2 & (B.p_n >= lo) & (B.p_n < hi)
        assert (pre[s] > 0).any() and (pre[s] < 0).any() and (pre[s] == 0).any(), (lo, hi)     # a condition on the inputs
        i = int(np.argmax(np.where(s, share, -1.0)))
        worst.append((lo, hi, float(share[i]), int(s.sum()), int((pre[s] != 0).sum()), case(i)))
    return worst


def check_device_margins(gibbs, device):
    """measured, not asserted: the largest slack of 1/2 ... 1/64 at which a decided inversion differs from the fp64 search"""
    I = inversion(gibbs)
    x = I.host["x"]
    out = []
    for j in range(1, 7):
        pre = gibbs.selftest_bigk_inversion(I.p_n, I.p_p, I.p_u, slack=2.0 ** -j, device=device)["pre"]
        bad = np.nonzero((pre != -1) & (pre != x))[0]
        first = (I.p_n[bad[0]], I.p_p[bad[0]], I.p_u[bad[0]], pre[bad[0]], x[bad[0]]) if bad.size else None
        out.append((2.0 ** -j, int(bad.size), int((pre >= 0).sum()), first))
    return out


def check_device_rerun(gibbs, device):
    I, B, D = inversion(gibbs), btrs(gibbs), device_run(gibbs, device)
    again = gibbs.selftest_bigk_inversion(I.p_n, I.p_p, I.p_u, slack=1.0, device=device)
    assert all(same(again[k], D.inv[k]) for k in D.inv)
    again = gibbs.selftest_bigk_btrs(B.p_n, B.p_p, B.p_u, B.p_v, device=device)
    assert all(same(again[k], D.btrs[k]) for k in D.btrs)
