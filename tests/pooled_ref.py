"""The specification of mmg_pooled_* (include/mmgibbs.h) in numpy.

A series has C >= 1 chains of S >= 1 draws x[c][s]; N = C S.  Every operation is one IEEE double operation rounded once; sums over the
chains run with c ascending, sums over the samples of a chain in sample order.

Log mode (transcripts, isoforms without hits, identical sets, genes), y = log x:
  per chain   m_c = (y_0 + y_1 + ...) / S;  rc_c, var_c, tau_c = Sokal's estimator on y (contrast_ref.sokal: the radix-2 transform on
              bit-reversed input with the library's twiddle table; rc 200 / 201 / 100 outside the powers of two in [4, 2^21], var = tau = 0)
  pooled      log_mean = (sum m_c) / C
              var      = ((S - 1) sum var_c + S sum (m_c - log_mean)^2) / (N - 1)          the sample variance of the N logged draws
              mcse2    = (sum tau_c var_c) / S / (C C)                                     the variance of the mean of C independent chain means
              tau      = (sum tau_c var_c) / (sum var_c)                                   so that mcse2 = tau W / N, W the mean within-chain variance
              rc       = the first non-zero rc_c, else 0;  rc != 0: tau = mcse2 = 0 (var: the formula on the zeros it was given)
  C = 1       the chain's own columns, copied: no arithmetic but mcse2 = tau_0 var_0 / S
  percentiles the order statistics of the N pooled draws of x itself at the caller's positions, in order_key order (NaNs last);
              a position outside [0, N) gives NaN
Non-finite values propagate; nothing is clamped.

Proportion mode (transcripts, isoforms without hits), p[c][s] = x / (the gene's sum in the same chain and sample):
  per chain   sp_c = sum p, s1_c = sum z, s2_c = sum z z in sample order, z = probit(min(max(p, 1e-9), 1 - 1e-9)), +inf when the gene has
              one member (multi false)
  pooled      mean = (sum sp_c) / N;  probit_mean = (sum s1_c) / N;  probit_sd = sqrt((sum s2_c - (sum s1_c)^2 / N) / (N - 1))
  percentiles the order statistics of the pooled proportions

`log` is np.log by default; the device tests pass the library's own logarithm (mmg_selftest_math) for bit identity.  `probit` is
scipy's ndtri by default: the library evaluates AS 241 itself, so against ndtri the two probit columns agree to that algorithm's
accuracy; the device tests pass the transcription of AS 241 on the library's logarithm (tests/key_space_checks.py: probit_as241),
against which they are bit-identical (the sums run in sample order on both sides).
"""
import numpy as np

import contrast_ref as CR


def _seq_sum(a):
    """the sum along the last axis, one addition after the other from the left (np.add.accumulate does not pair up)"""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        return np.add.accumulate(a, axis=-1)[..., -1]


def _fft_bitrev(re, im, tw):
    """contrast_ref._fft_bitrev over the last axis of a batch: the same butterflies, a stage at a time"""
    S = re.shape[-1]
    ln = 2
    while ln <= S:
        half = ln // 2
        b = np.arange(S // 2)
        j = b & (half - 1)
        i = (b // half) * ln + j
        q = i + half
        wr, wi = tw[half + j, 0], tw[half + j, 1]
        xr = re[..., q] * wr - im[..., q] * wi
        xi = re[..., q] * wi + im[..., q] * wr
        ar, ai = re[..., i].copy(), im[..., i].copy()
        re[..., q] = ar - xr; im[..., q] = ai - xi
        re[..., i] = ar + xr; im[..., i] = ai + xi
        ln *= 2


def sokal_batch(Y):
    """contrast_ref.sokal of every row of Y (B, S): (rc, var, tau) as arrays -- the same operations in the same order, vectorised"""
    Y = np.asarray(Y, np.float64)
    B, S = Y.shape
    rc = 100 if S > (2 << 20) else 200 if S < 4 else 201 if S & (S - 1) else 0
    if rc:
        return np.full(B, rc, np.int32), np.zeros(B), np.zeros(B)
    tw = CR.twiddles(S)
    br = CR._bitrev(S)
    with np.errstate(all="ignore"):
        re, im = np.empty((B, S)), np.zeros((B, S))
        re[:, br] = Y
        _fft_bitrev(re, im, tw)
        pw = re * re + im * im
        pw[:, 0] = 0.0
        re[:, br] = pw
        im[:] = 0.0
        _fft_bitrev(re, im, tw)
        n = float(S)
        r0 = re[:, 0]
        var = r0 / (n * (n - 1.0))
        c = np.float64(1.0) / r0
        terms = re * c[:, None] - 0.166666666666666666666
        tot = np.add.accumulate(np.concatenate([np.full((B, 1), -0.333333333333333333333), terms], axis=1), axis=1)[:, 1:]
        neg = tot < 0
        stop = neg.any(axis=1)
        first = np.argmax(neg, axis=1)
        m = np.where(stop, first + 1, S + 1).astype(np.float64)
        total = np.where(stop, tot[np.arange(B), first], tot[:, -1])
        tau = 2 * (total + (m - 1.0) / 6.0)
    return np.zeros(B, np.int32), var, tau


def chain_columns(x, log=np.log):
    """(m, var, tau, rc), each (C,), of the chains x (C, S): what k_series_summary<., true> gives for each chain alone"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        y = log(np.ascontiguousarray(x).ravel()).reshape(x.shape)
        m = _seq_sum(y) / x.shape[1]
    rc, var, tau = sokal_batch(y)
    return m, var, tau, rc


def combine(m, var, tau, rc, S):
    """the pooled columns (log_mean, var, tau, mcse2, rc) of one series from its chains' columns"""
    C = len(m)
    with np.errstate(all="ignore"):
        if C == 1:
            r = int(rc[0])
            return m[0], var[0], (0.0 if r else tau[0]), (0.0 if r else tau[0] * var[0] / np.float64(S)), r
        sm = sv = stv = np.float64(0.0)
        r = 0
        for c in range(C):
            sm = sm + m[c]
            sv = sv + var[c]
            stv = stv + tau[c] * var[c]
            if r == 0:
                r = int(rc[c])
        dS, dC, dN = np.float64(S), np.float64(C), np.float64(C * S)
        mean = sm / dC
        sb = np.float64(0.0)
        for c in range(C):
            e = m[c] - mean
            sb = sb + e * e
        v = ((dS - 1.0) * sv + dS * sb) / (dN - 1.0)
        if r:
            return mean, v, 0.0, 0.0, r
        return mean, v, stv / sv, stv / dS / (dC * dC), r


def order_statistics(x, percentile_index):
    """the order statistics of the draws x (any shape) at the given positions; NaN outside [0, x.size)"""
    srt = CR.sorted_series(np.ascontiguousarray(x, np.float64).ravel())
    out = np.full(len(percentile_index), np.nan)
    for q, idx in enumerate(percentile_index):
        if 0 <= idx < srt.size:
            out[q] = srt[idx]
    return out


def pooled_of_traces(traces, percentile_index=(), log=np.log):
    """traces (C, S, count) -> dict of log_mean, var, tau, mcse2, rc, percentiles (count, np) and the chains' columns c_mean, c_var,
    c_tau, c_rc (count, C): what mmg_pooled_of_traces / mmg_pooled_get / mmg_pooled_get_chain return"""
    tr = np.asarray(traces, np.float64)
    C, S, count = tr.shape
    xs = np.ascontiguousarray(tr.transpose(2, 0, 1))                    # (count, C, S)
    m, var, tau, rc = chain_columns(xs.reshape(count * C, S), log)
    m, var, tau, rc = (a.reshape(count, C) for a in (m, var, tau, rc))
    out = dict(log_mean=np.empty(count), var=np.empty(count), tau=np.empty(count), mcse2=np.empty(count), rc=np.empty(count, np.int32),
               percentiles=np.empty((count, len(percentile_index))), c_mean=m, c_var=var, c_tau=tau, c_rc=rc)
    for i in range(count):
        out["log_mean"][i], out["var"][i], out["tau"][i], out["mcse2"][i], out["rc"][i] = combine(m[i], var[i], tau[i], rc[i], S)
        out["percentiles"][i] = order_statistics(xs[i], percentile_index)
    return out


def pooled_proportions(props, multi, percentile_index=(), probit=None):
    """props (C, S, count), multi (count,) bool -> dict of mean, probit_mean, probit_sd, percentiles (count, np)"""
    if probit is None:
        from scipy.special import ndtri as probit
    p = np.asarray(props, np.float64)
    C, S, count = p.shape
    multi = np.asarray(multi, bool)
    ps = np.ascontiguousarray(p.transpose(2, 0, 1))                     # (count, C, S)
    with np.errstate(all="ignore"):
        z = probit(np.clip(ps, 1e-9, 1 - 1e-9))
        z[~multi] = np.inf
        sp, s1, s2 = _seq_sum(ps), _seq_sum(z), _seq_sum(z * z)         # (count, C)
        tp = t1 = t2 = np.zeros(count)
        for c in range(C):
            tp = tp + sp[:, c]
            t1 = t1 + s1[:, c]
            t2 = t2 + s2[:, c]
        N = np.float64(C * S)
        out = dict(mean=tp / N, probit_mean=t1 / N, probit_sd=np.sqrt((t2 - t1 * t1 / N) / (N - 1.0)),
                   percentiles=np.empty((count, len(percentile_index))))
    for i in range(count):
        out["percentiles"][i] = order_statistics(ps[i], percentile_index)
    return out
