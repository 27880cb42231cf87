"""The checks of mmg_selftest_keyed (the keyed streams over their whole key space, the scalar functions and the word-to-uniform
maps pointwise), written once and run on both instantiations of the library's inline code: tests/test_key_space.py passes
device = -1 (the host instantiation, no GPU needed), tests/test_gpu_key_space.py device = 0 (the kernels).

The expected values come from the CPU oracle (oracle/mmseq_oracle.c), from restatements of the key derivation in Python integers
 and from numpy transcriptions; every comparison is exact equality, NaN in the same places."""
import math
from fractions import Fraction

import numpy as np

M32 = 0xFFFFFFFF
TAG_ROW, TAG_GAMMA, TAG_SIMU, TAG_DIFF_PERM = 1, 2, 5, 8

SEEDS = [0, 1234, 2 ** 32, 2 ** 32 + 1234, 2 ** 63, 2 ** 64 - 7, 0x9E3779B97F4A7C15]
CHAINS = [0, 1, 2 ** 24 - 1]
IDS = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 1, 2 ** 64 - 1]
ITERS = [0, 16383, 2 ** 31, 2 ** 32 - 1]
GRID_SHAPES = [0.1, 0.6, 1.0, 7.3, 1234.1]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ----------------------------------------------------------------------------- the key derivation, in Python integers
def u52_exact(a, b):
    v = ((int(a) >> 6) << 26) | (int(b) >> 6)
    return Fraction(2 * v + 1, 2 ** 53)                                  # (v + 1/2) 2^-52


def u32_exact(x):
    return Fraction(2 * int(x) + 1, 2 ** 33)                             # (x + 1/2) 2^-32


def exact_float(fr):
    f = float(fr)                                                        # correctly rounded; the maps are specified to be exact
    assert Fraction(f) == fr, fr
    return f


def stream_key(seed, chain, tag):
    return seed & M32, ((seed >> 32) ^ (chain & 0x00FFFFFF) ^ (tag << 24)) & M32


def stream_uniforms(orc, seed, chain, tag, ident, it):
    """the first two pairs of Stream(seed, chain, tag, ident, it): Philox4x32-10 blocks c3 = 0, 1"""
    out = []
    for c3 in (0, 1):
        r = orc.philox([ident & M32, ident >> 32, it, c3], list(stream_key(seed, chain, tag)))
        out += [exact_float(u52_exact(r[0], r[1])), exact_float(u52_exact(r[2], r[3]))]
    return out


def stream2_key(seed, chain, tag, q_hi):
    return ((seed & M32) ^ (((seed >> 32) * 0x9E3779B1) & M32) ^ ((chain * 0x85EBCA6B) & M32) ^ ((tag << 28) & M32)
            ^ ((q_hi * 0xC2B2AE35) & M32))


def stream2_words(orc, seed, chain, tag, ident, it):
    """the first three words of Stream2(seed, chain, tag, ident, it): block q = ident >> 1, output word ident & 1, key + b 0xBB67AE85"""
    q = ident >> 1
    key = stream2_key(seed, chain, tag, q >> 32)
    return [int(orc.philox2x32([q & M32, it], (key + b * 0xBB67AE85) & M32)[ident & 1]) for b in range(3)]


def _grid():
    g = [(s, c, TAG_GAMMA, i, t) for s in SEEDS for c in CHAINS for i in IDS for t in ITERS]
    # the other tags the library draws with, at the corners of the grid
    g += [(s, c, tag, i, t) for tag in (TAG_ROW, TAG_SIMU, TAG_DIFF_PERM) for s in (SEEDS[3], SEEDS[5]) for c in (0, CHAINS[2])
          for i in (IDS[1], IDS[3]) for t in (0, ITERS[3])]
    return g


def check_streams(gibbs, orc, device):
    g = _grid()
    seed, chain, tag, ident, it = [np.array(col, dt) for col, dt in zip(zip(*g), (np.uint64, np.uint32, np.uint32, np.uint64, np.uint32))]
    shape = np.array([GRID_SHAPES[j % len(GRID_SHAPES)] for j in range(len(g))])
    got = gibbs.selftest_keyed_streams(seed, chain, tag, ident, it, shape=shape, scale=1.5, device=device)
    exp_u = np.array([stream_uniforms(orc, *k) for k in g])
    exp_w = np.array([stream2_words(orc, *k) for k in g], np.uint32)
    assert same(got["uniforms"], exp_u)
    assert same(got["words"], exp_w)
    L = orc.lib()
    exp_g = np.array([L.orc_gamma_draw(s, c, t, i, float(a), 1.5) if tg == TAG_GAMMA else
                      (orc.simu_gamma_trace_keyed(s, c, tg, i, float(a), 1.5, 1)[0] if t == 0 else np.nan)
                      for (s, c, tg, i, t), a in zip(g, shape)])
    known = ~np.isnan(exp_g)
    assert known.sum() >= len(SEEDS) * len(CHAINS) * len(IDS) * len(ITERS) + 24
    assert same(got["gamma"][known], exp_g[known])
    # no two keys of the grid collide in the row stream; in the Philox4x32 stream exactly those that the key derivation identifies do
    # ((seed + 2^32, chain 0) and (seed, chain 1): check_stream_identities)
    assert np.unique(got["words"], axis=0).shape[0] == len(g)
    n_keys = len({stream_key(s, c, tg) + (i, t) for s, c, tg, i, t in g})
    assert np.unique(got["uniforms"], axis=0).shape[0] == n_keys < len(g)


def check_stream_identities(gibbs, device):
    """What the key derivation implies, written down: both streams see the high seed word and the high id word; the Philox4x32 stream
    XORs the high seed word and the chain into one key word, the row stream multiplies them by different constants."""
    def run(keys):
        seed, chain, ident, it = [np.array(col, dt) for col, dt in zip(zip(*keys), (np.uint64, np.uint32, np.uint64, np.uint32))]
        return gibbs.selftest_keyed_streams(seed, chain, TAG_GAMMA, ident, it, shape=2.5, device=device)

    for s in (0, 1234, 2 ** 63 + 99):
        for i in (0, 7, 2 ** 31 + 3):
            hi = (s + 2 ** 32) & (2 ** 64 - 1)
            r = run([(s, 0, i, 5), (hi, 0, i, 5), (s, 0, i + 2 ** 32, 5), (s, 1, i, 5)])
            u, w, g = r["uniforms"], r["words"], r["gamma"]
            assert not (u[0] == u[1]).any() and not (w[0] == w[1]).any() and g[0] != g[1]      # seed, seed + 2^32: both streams differ
            assert not (u[0] == u[2]).any() and g[0] != g[2]                                    # id, id + 2^32: the Philox4x32 stream differs
            assert same(u[1], u[3]) and g[1] == g[3]                                             # (seed + 2^32, chain 0) IS (seed, chain 1) there
            assert not (w[1] == w[3]).any()                                                      # ... and is not in the row stream
    # the row stream keys rows in pairs: id + 2^32 is block q + 2^31 of the same key, id + 2^33 changes the key
    r = run([(1234, 0, 6, 5), (1234, 0, 6 + 2 ** 32, 5), (1234, 0, 6 + 2 ** 33, 5)])
    assert not (r["words"][0] == r["words"][1]).any() and not (r["words"][0] == r["words"][2]).any()


# ----------------------------------------------------------------------------- Gamma shapes, binomials, normals
GAMMA_SHAPES = [0.01, 0.1, 1.0 - 2.0 ** -53, 1.0, 1.1, 1e6 + 0.1, 5e7 + 0.1]
GAMMA_N = 50000                  # gamma_unit's device branch resolves four Philox blocks per pass: most lanes take one, the unluckiest several
BINOMIALS = [(2 ** 32 - 1, 0.5), (2 ** 31, 3e-9), (1000, math.nextafter(0.01, 0.0)), (1000, 0.01), (1000, math.nextafter(0.01, 1.0)),
             (50, 1.0 - 2.0 ** -53), (7, 5e-324)]
BINOMIAL_N = 20000


def check_gamma_shape(gibbs, orc, device, shape):
    ref = np.empty(GAMMA_N)
    orc.lib().orc_keyed_gamma_v(77, shape, 1.0, GAMMA_N, ref)
    if shape == 0.01:
        # Gamma(a + 1) U^(1/a): U^100 underflows for U < 8e-4 -- the draw ends in the subnormal range or at 0
        assert ((ref > 0) & (ref < 2.0 ** -1022)).sum() >= 3 and (ref == 0).sum() >= 3
    assert np.isfinite(ref).all() and (ref >= 0).all()
    assert same(gibbs.selftest_gamma(77, shape, 1.0, GAMMA_N, device), ref)


def check_binomial(gibbs, orc, device, nn, p):
    assert (1000 * math.nextafter(0.01, 0.0) < 10.0) and (1000 * math.nextafter(0.01, 1.0) >= 10.0)   # inversion on one side, BTRS on the other
    ref = np.empty(BINOMIAL_N, np.uint32)
    orc.lib().orc_keyed_binomial_v(2 ** 32 + 8, nn, p, BINOMIAL_N, ref)
    assert same(gibbs.selftest_binomial(2 ** 32 + 8, nn, p, BINOMIAL_N, device), ref)


def check_normal(gibbs, orc, device):
    n, seed = 20000, 2 ** 32 + 5
    ref = np.empty(n)
    orc.lib().orc_keyed_normal_v(seed, n, ref)
    assert same(gibbs.selftest_keyed_math(np.zeros(n), normal_seed=seed, device=device)["normal"], ref)


# ----------------------------------------------------------------------------- probit: AS 241 (PPND16), transcribed
_A = [3.3871328727963666080e0, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4, 4.5921953931549871457e4,
      6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3]
_B = [1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3, 2.1213794301586595867e4, 3.9307895800092710610e4,
      2.8729085735721942674e4, 5.2264952788528545610e3]
_C = [1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0, 1.27045825245236838258e0,
      2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4]
_D = [1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9]
_E = [6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1, 2.65321895265761230930e-2,
      1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7]
_F = [1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15]


def _horner(c, r):
    acc = c[7] * r + c[6]
    for j in range(5, -1, -1):
        acc = acc * r + c[j]
    return acc


def probit_as241(p, log=None):
    """Wichura (1988), algorithm AS 241, PPND16, operation for operation as mmg_math.h's dprobit (fp64, no contraction): bit-identical
    to it when `log` is the library's logarithm (the oracle's log_v)."""
    if log is None:
        from oracle import binding
        log = binding.log_v
    p = np.asarray(p, np.float64)
    shp = p.shape
    p = p.ravel()
    q = p - 0.5
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        mid = np.abs(q) <= 0.425
        r = 0.180625 - q[mid] * q[mid]
        out[mid] = q[mid] * _horner(_A, r) / _horner(_B, r)
        tail = ~mid
        neg = q[tail] < 0
        r = np.where(neg, p[tail], 1.0 - p[tail])
        val = np.empty_like(r)
        edge = r <= 0.0
        val[edge] = np.inf
        rr = np.sqrt(-log(r[~edge]))
        near = rr <= 5.0
        v = np.empty_like(rr)
        rn = rr[near] - 1.6
        v[near] = _horner(_C, rn) / _horner(_D, rn)
        rf = rr[~near] - 5.0                                              # (a NaN lands here, as in the C code)
        v[~near] = _horner(_E, rf) / _horner(_F, rf)
        val[~edge] = v
        out[tail] = np.where(neg, -val, val)
    return out.reshape(shp)


def probit_grid():
    lo = np.geomspace(1e-300, 0.5, 20000)
    edges = []
    for e in (0.075, 0.925, math.exp(-25.0)):
        edges += [math.nextafter(e, 0.0), e, math.nextafter(e, 1.0)]
    return np.concatenate([lo, 1.0 - lo, edges, [0.0, 1.0, 5e-324, 1.0 - 2.0 ** -53, np.nan, -0.1]])


def check_probit(gibbs, orc, device):
    x = probit_grid()
    ref = probit_as241(x, orc.log_v)
    # every branch, both signs, and the specials
    r = np.sqrt(-np.log(np.minimum(x[:20000], 0.5)))
    assert (x[:20000] >= 0.075).any() and ((x[:20000] < 0.075) & (r <= 5)).any() and (r > 5).sum() > 1000
    assert ref[-6] == -np.inf and ref[-5] == np.inf and np.isfinite(ref[-4]) and np.isfinite(ref[-3]) and np.isnan(ref[-2]) and ref[-1] == -np.inf
    assert same(gibbs.selftest_keyed_math(x, device=device)["probit"], ref)


# ----------------------------------------------------------------------------- lgamma, Stirling remainder, ilogb
def lgamma_grid():
    xs = np.concatenate([np.linspace(0.1, 10, 997), np.geomspace(10, 1e6, 500), [0.5, 1.0, 1.5, 2.0, 3.0, 7.999, 8.0]])   # tests/test_mmdiff_ref.py
    extra = [1.0, 2.0, math.nextafter(8.0, 0.0), 8.0, math.nextafter(8.0, 9.0), 1e-300, 1e300, 0.0, -1.0, np.nan, np.inf]
    return np.concatenate([xs, extra])


def check_lgamma(gibbs, device):
    import mmdiff_ref as R
    x = lgamma_grid()
    ref = R.dlgamma(x)
    assert np.isnan(ref[-4:-1]).all() and ref[-1] == np.inf and np.isfinite(ref[:-4]).all()
    assert same(gibbs.selftest_keyed_math(x, device=device)["lgamma"], ref)


STIRLING_K = [float(k) for k in range(13)] + [1e9, 4.29e9]
_STIRLING_TAB = [0.0810614667953272, 0.0413406959554092, 0.0276779256849983, 0.02079067210376509, 0.0166446911898211, 0.0138761288230707,
                 0.0118967099458917, 0.0104112652619720, 0.00925546218271273, 0.00833056343336287]


def stirling_tail_ref(k):
    """mmg_math.h's stirling_tail, transcribed: a table up to 9, three terms of the series in 1 / (k + 1) above"""
    k = np.asarray(k, np.float64)
    kp1sq = (k + 1.0) * (k + 1.0)
    f = (1.0 / 12.0 - (1.0 / 360.0 - 1.0 / 1260.0 / kp1sq) / kp1sq) / (k + 1.0)
    return np.where(k <= 9.0, np.array(_STIRLING_TAB)[np.minimum(k, 9).astype(int)], f)


def stirling_tail_mp(k):
    """log(k!) - [(k + 1/2) log(k + 1) - (k + 1) + log(2 pi) / 2] at 50 digits"""
    import mpmath as mp
    with mp.workdps(50):
        k = mp.mpf(k)
        return mp.loggamma(k + 1) - ((k + mp.mpf(0.5)) * mp.log(k + 1) - (k + 1) + mp.log(2 * mp.pi) / 2)


def check_stirling(gibbs, device):
    x = np.array(STIRLING_K + [9.5, 2.0 ** 32 - 1, -1.0, 2.0 ** 32, np.nan])
    got = gibbs.selftest_keyed_math(x, device=device)["stirling"]
    assert same(got[:-3], stirling_tail_ref(x[:-3])) and np.isnan(got[-3:]).all()
    return got[:len(STIRLING_K)]


def check_ilogb(gibbs, device):
    rng = np.random.default_rng(5)
    sub = rng.integers(1, 2 ** 52, 2000, dtype=np.uint64).view(np.float64)             # subnormals of every magnitude
    few = (np.uint64(1) << rng.integers(0, 52, 200).astype(np.uint64)).view(np.float64)   # ... with a single bit
    x = np.concatenate([sub, few, [5e-324, 1e-310, 2.0 ** -1022 - 2.0 ** -1074, 2.0 ** -1022, 1.0, 1.5, 1e300, 1.7976931348623157e308,
                                   0.0, -1.0, np.inf, np.nan]])
    assert (x[:2200] > 0).all() and (x[:2200] < 2.0 ** -1022).all()
    exp = np.array([math.frexp(v)[1] - 1 for v in x[:-4]] + [-2 ** 31] * 4, np.int32)
    assert exp[2200] == -1074 and exp[2202] == -1023
    assert same(gibbs.selftest_keyed_math(x, device=device)["ilogb"], exp)


# ----------------------------------------------------------------------------- words to uniforms
WORDS = [0, 1, 2 ** 31, 2 ** 32 - 1]
TOTALS = [5e-324, 1e-310, 1.0, 1e300, np.inf]


def check_word_maps(gibbs, device):
    cases = [(a, b, t) for a in WORDS for b in WORDS for t in TOTALS]
    w0, w1, t = [np.array(c, dt) for c, dt in zip(zip(*cases), (np.uint32, np.uint32, np.float64))]
    got = gibbs.selftest_keyed_words(w0, w1, t, device=device)
    assert same(got["u32"], [exact_float(u32_exact(a)) for a, _, _ in cases])
    assert same(got["u52"], [exact_float(u52_exact(a, b)) for a, b, _ in cases])
    assert 0.0 < got["u32"].min() and got["u32"].max() < 1.0 and 0.0 < got["u52"].min() and got["u52"].max() < 1.0
    exp = []
    for a, _, tt in cases:
        ts = tt * 2.0 ** -32            # the two products the kernels form (t 2^-32 underflows to 0 for the subnormal totals)
        hs = ts * 0.5
        if math.isinf(tt):
            exp.append(np.nan if a == 0 else np.inf)                    # fma(0, inf, inf)
        else:
            exp.append(float(Fraction(a) * Fraction(ts) + Fraction(hs)))  # the real number (x + 1/2) ts, rounded once
    assert same(got["target"], exp)
