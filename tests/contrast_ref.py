"""The specification of mmg_contrast_* (include/mmgibbs.h) in numpy.

A contrast has an ordered numerator list and an ordered denominator list of members, rows of `traces` (n_series, S): a member < n is
the caller's transcript, n + v isoform without hits v, whose trace is the simulated one (the caller stacks them below the transcripts,
the convention of mmg_summary_desc's groups).  Both lists are non-empty; a member may be on both sides, not twice on one.

Per kept sample s:  N_s = 0; N_s += traces[num_j, s] for j ascending (each fp64 addition rounded once), D_s alike;
                    r_s = log(N_s) - log(D_s) -- never log(N_s / D_s): mu of a transcript without reads is routinely below 1e-38 and
                    the quotient underflows where the difference does not; non-finite values propagate, nothing is clamped;
                    gt_s = N_s > D_s, on the sums.
Per contrast:       log_ratio = (r_0 + r_1 + ... in sample order) / S;  var, tau, rc = Sokal's estimator on r with the radix-2
                    transform on bit-reversed input and the twiddle table of the library; the order statistics of r at the caller's
                    indices, sorted by the library's integer key (NaN last);  p_gt = (number of s with gt_s) / S.
`log` is np.log by default; the device tests pass the library's own logarithm (mmg_selftest_math) for bit identity.
"""
import numpy as np


def check_contrasts(contrasts, n_series):
    if len(contrasts) == 0:
        raise ValueError("no contrasts")
    for c, (num, den) in enumerate(contrasts):
        for side, ms in (("numerator", num), ("denominator", den)):
            if len(ms) == 0:
                raise ValueError("empty %s of contrast %d" % (side, c))
            if len(set(int(m) for m in ms)) != len(ms):
                raise ValueError("a member twice in the %s of contrast %d" % (side, c))
            if min(ms) < 0 or max(ms) >= n_series:
                raise ValueError("%s member out of range of contrast %d" % (side, c))


def side_sum(traces, members):
    acc = np.zeros(traces.shape[1])
    for m in members:
        acc = acc + traces[int(m)]                      # one rounding per addition, in list order, from 0.0
    return acc


def series(traces, contrasts, log=np.log):
    """R (n_contrasts, S) and gt (n_contrasts, S, bool)"""
    traces = np.asarray(traces, np.float64)
    check_contrasts(contrasts, traces.shape[0])
    N = np.stack([side_sum(traces, c[0]) for c in contrasts])
    D = np.stack([side_sum(traces, c[1]) for c in contrasts])
    with np.errstate(divide="ignore", invalid="ignore"):
        R = log(N.ravel()).reshape(N.shape) - log(D.ravel()).reshape(D.shape)
    return R, N > D


def sort_key(x):
    """the library's order-preserving map of doubles onto unsigned integers (mmg_series.h: order_key): NaN of either sign bit set... sorts
    by its bits; the positive NaNs come last"""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def sort_unkey(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def sorted_series(r):
    return sort_unkey(np.sort(sort_key(r)))


def twiddles(S):
    """tw[half + j] = exp(-2 pi i j / (2 half)) as (cos, sin) of the host's libm (post.hip: twiddles)"""
    import math
    tw = np.zeros((max(S, 1), 2))
    ln = 2
    while ln <= S:
        ang = -2.0 * math.pi / ln
        half = ln // 2
        for j in range(half):
            tw[half + j] = (math.cos(ang * j), math.sin(ang * j))
        ln *= 2
    return tw


def _fft_bitrev(re, im, tw):
    """in-place radix-2 decimation in time on bit-reversed input: the butterflies of host/numerics.hpp:fft_pow2, a stage at a time"""
    S = re.size
    ln = 2
    while ln <= S:
        half = ln // 2
        b = np.arange(S // 2)
        j = b & (half - 1)
        i = (b // half) * ln + j
        q = i + half
        wr, wi = tw[half + j, 0], tw[half + j, 1]
        xr = re[q] * wr - im[q] * wi
        xi = re[q] * wi + im[q] * wr
        ar, ai = re[i].copy(), im[i].copy()
        re[q] = ar - xr; im[q] = ai - xi
        re[i] = ar + xr; im[i] = ai + xi
        ln *= 2


def _bitrev(S):
    lg = S.bit_length() - 1
    idx = np.arange(S)
    out = np.zeros(S, np.int64)
    for k in range(lg):
        out |= ((idx >> k) & 1) << (lg - 1 - k)
    return out


def sokal(y):
    """(rc, var, tau) of src/sokal.cc:33-87 as k_series_summary computes it: rc 100 beyond 2^21 samples, 200 below 4, 201 for a length
    that is no power of two (var = tau = 0 then)"""
    y = np.asarray(y, np.float64)
    S = y.size
    if S > (2 << 20):
        return 100, 0.0, 0.0
    if S < 4:
        return 200, 0.0, 0.0
    if S & (S - 1):
        return 201, 0.0, 0.0
    tw = twiddles(S)
    br = _bitrev(S)
    with np.errstate(all="ignore"):
        re, im = np.empty(S), np.zeros(S)
        re[br] = y
        _fft_bitrev(re, im, tw)
        pw = re * re + im * im
        pw[0] = 0.0                                     # removes the mean
        re[br] = pw
        im[:] = 0.0
        _fft_bitrev(re, im, tw)
        n = float(S)
        r0 = re[0]
        var = r0 / (n * (n - 1.0))
        c = np.float64(1.0) / r0
        total = np.float64(-0.333333333333333333333)
        m = S + 1
        for i in range(S):
            total = total + (re[i] * c - 0.166666666666666666666)
            if total < 0:
                m = i + 1
                break
        tau = 2 * (total + (m - 1.0) / 6.0)
    return 0, float(var), float(tau)


def contrast_ref(traces, contrasts, percentile_index=(), log=np.log):
    """dict of R, gt, log_ratio, var, tau, rc, p_gt, percentiles -- what mmg_contrast_get and _get_rows return"""
    R, gt = series(traces, contrasts, log)
    C, S = R.shape
    out = dict(R=R, gt=gt, log_ratio=np.empty(C), var=np.empty(C), tau=np.empty(C), rc=np.empty(C, np.int32), p_gt=np.empty(C),
               percentiles=np.full((C, len(percentile_index)), np.nan))
    for c in range(C):
        acc = np.float64(0.0)
        with np.errstate(invalid="ignore"):
            for s in range(S):
                acc = acc + R[c, s]                     # sequential, sample order
        out["log_ratio"][c] = acc / S
        out["rc"][c], out["var"][c], out["tau"][c] = sokal(R[c])
        srt = sorted_series(R[c])
        for q, idx in enumerate(percentile_index):
            if 0 <= idx < S:
                out["percentiles"][c, q] = srt[idx]
        out["p_gt"][c] = int(gt[c].sum()) / S
    return out
