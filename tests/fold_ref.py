"""The specification of mmg_fold_* (include/mmgibbs.h) and of the mmfold CLI in numpy, brute force.  No device.

Input: per feature f the draws a[f] (Sa of them) of sample A and b[f] (Sb) of sample B on the mu scale, an offset `off` on the
natural-log scale, and zero-based ranks.

Valid:       every draw of both sides finite and > 0.  Otherwise status bit 0 (a draw of A) and / or bit 1 (a draw of B), every
             output NaN, both counts 0.
Logs:        x_i = log(a_i), y_j = log(b_j) + off, d_ij = x_i - y_j, each rounded once; `log` is the library's dlog (through the
             oracle's log_v, as tests/mmdiff_ref.py takes it), so bits can be compared.  -0.0 counts as +0.0.
Counts:      n_gt = #{(i, j): x_i > y_j}, n_eq = #{(i, j): x_i == y_j}: explicit comparisons of x with y, never through d.
Ranks:       result r = np.sort(np.subtract.outer(x, y), axis=None)[ranks[r]]: the full Sa x Sb matrix, sorted.  A rank >= Sa Sb
             gives NaN for that rank alone.
Sums (lsum): over the series in the caller's sample order; lane l of 64 adds its samples l, l + 64, ... ascending from 0.0 (a lane
             without samples holds 0.0), the 64 partial sums are folded by halving, x[:32] + x[32:], then 16, 8, 4, 2, 1
             (pairs_ref.lsum).  mean_a = lsum(x) / Sa, ss_a = lsum((x - mean_a) * (x - mean_a)), each square rounded, then added;
             mean_b and ss_b likewise from y (offset included).
Derived:     lfc = mean_a - mean_b, sd = sqrt(ss_a / (Sa - 1) + ss_b / (Sb - 1)), p_gt = (n_gt + n_eq / 2) / (Sa Sb).

`bisect_rank` writes out the method the kernel uses for the ranks -- a bisection over the 64-bit key space of d with a count per
round -- so that tests/test_fold_ref.py can hold it against the sort on the CPU.

The CLI's rules: `offset_rule` (the median of log_mu_A - log_mu_B over the features with unique_hits >= uhmin and a finite log_mu in
both tables; the mean of the two middle values for an even count), `percentile_rank` (mmseq -percentiles' index rule with
Sa Sb - 1 for trace_len - 1: C's round), `gfold_of`, and `table`, the text mmfold writes.
"""
import struct

import numpy as np

from mmdiff_ref import dlog
from pairs_ref import lsum

DEVICE_COLUMNS = ("mean_a", "mean_b", "ss_a", "ss_b", "n_gt", "n_eq", "quantiles", "status")
BAD_A, BAD_B, NO_TRACE = 1, 2, 4


def _valid(v):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isfinite(v) & (v > 0)))


def logs(a, b, off, log=dlog):
    """x, y of one valid feature"""
    x = np.asarray(log(np.ascontiguousarray(a, np.float64)), np.float64) + 0.0
    y = (np.asarray(log(np.ascontiguousarray(b, np.float64)), np.float64) + np.float64(off)) + 0.0
    return x, y


def fold_ref(a, b, off, ranks, log=dlog):
    """a: (F, Sa), b: (F, Sb) -> the device columns; quantiles (F, len(ranks))"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    F, Sa = a.shape
    Sb = b.shape[1]
    assert b.shape[0] == F and Sa >= 1 and Sb >= 1
    ranks = [int(k) for k in ranks]
    out = dict(mean_a=np.full(F, np.nan), mean_b=np.full(F, np.nan), ss_a=np.full(F, np.nan), ss_b=np.full(F, np.nan),
               n_gt=np.zeros(F, np.uint32), n_eq=np.zeros(F, np.uint32), quantiles=np.full((F, len(ranks)), np.nan),
               status=np.zeros(F, np.uint8))
    for f in range(F):
        st = (0 if _valid(a[f]) else BAD_A) | (0 if _valid(b[f]) else BAD_B)
        out["status"][f] = st
        if st:
            continue
        x, y = logs(a[f], b[f], off, log)
        with np.errstate(all="ignore"):
            out["mean_a"][f] = lsum(x) / float(Sa)
            out["mean_b"][f] = lsum(y) / float(Sb)
            da, db = x - out["mean_a"][f], y - out["mean_b"][f]
            out["ss_a"][f] = lsum(da * da)
            out["ss_b"][f] = lsum(db * db)
        out["n_gt"][f] = int((x[:, None] > y[None, :]).sum())
        out["n_eq"][f] = int((x[:, None] == y[None, :]).sum())
        if ranks:
            d = np.sort(np.subtract.outer(x, y), axis=None)
            for r, k in enumerate(ranks):
                if k < Sa * Sb:
                    out["quantiles"][f, r] = d[k]
    return out


def derived(dev, Sa, Sb):
    with np.errstate(all="ignore"):
        p = (dev["n_gt"].astype(np.float64) + dev["n_eq"].astype(np.float64) / 2.0) / np.float64(Sa * Sb)
        return dict(lfc=dev["mean_a"] - dev["mean_b"], sd=np.sqrt(dev["ss_a"] / np.float64(Sa - 1) + dev["ss_b"] / np.float64(Sb - 1)),
                    p_gt=np.where(dev["status"] != 0, np.nan, p))


def summary_ref(a, b, off, ranks, log=dlog):
    dev = fold_ref(a, b, off, ranks, log)
    dev.update(derived(dev, np.asarray(a).shape[1], np.asarray(b).shape[1]))
    return dev


# ---- the kernel's method for the ranks, written out
def key_of(v):
    """order-preserving map of a double onto a 64-bit unsigned integer"""
    u = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    return (~u) & 0xffffffffffffffff if u >> 63 else u | 0x8000000000000000


def unkey(k):
    u = k & 0x7fffffffffffffff if k >> 63 else (~k) & 0xffffffffffffffff
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def count_le(xs, ys, c):
    """#{(i, j): xs[i] - ys[j] <= c} over sorted xs, ys: row i of the differences falls as j grows, so it is Sb - (the first j
    with xs[i] - ys[j] <= c), found by a binary search per row"""
    total = 0
    Sb = len(ys)
    for xi in xs:
        lo, hi = 0, Sb
        while lo < hi:
            mid = (lo + hi) >> 1
            if xi - ys[mid] <= c:
                hi = mid
            else:
                lo = mid + 1
        total += Sb - lo
    return total


def bisect_rank(x, y, k):
    """the k-th smallest (zero-based) of x_i - y_j: the smallest key c with #{d_ij <= c} >= k + 1, in at most 64 rounds"""
    xs, ys = np.sort(np.asarray(x, np.float64) + 0.0), np.sort(np.asarray(y, np.float64) + 0.0)
    if k >= len(xs) * len(ys):
        return np.nan
    lo, hi = key_of((xs[0] - ys[-1]) + 0.0), key_of((xs[-1] - ys[0]) + 0.0)
    rounds = 0
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if count_le(xs, ys, np.float64(unkey(mid))) >= k + 1:
            hi = mid
        else:
            lo = mid + 1
        rounds += 1
    assert rounds <= 64
    return unkey(lo) + 0.0


# ---- the CLI's rules
def offset_rule(log_mu_a, log_mu_b, uh_a, uh_b, uhmin=1):
    """(offset, the number of features that set it); (None, 0) when no feature qualifies"""
    la, lb = np.asarray(log_mu_a, np.float64), np.asarray(log_mu_b, np.float64)
    ok = (np.asarray(uh_a) >= uhmin) & (np.asarray(uh_b) >= uhmin) & np.isfinite(la) & np.isfinite(lb)
    d = np.sort(la[ok] - lb[ok])
    n = d.size
    if n == 0:
        return None, 0
    return (float(d[n // 2]) if n % 2 else float((d[n // 2 - 1] + d[n // 2]) / 2.0)), n


def percentile_rank(p, n_pairs):
    """C's round(p / 100 * (n_pairs - 1)): halves away from zero"""
    v = float(p) / 100.0 * float(n_pairs - 1)
    fl = np.floor(v)
    return int(fl) + (1 if v - fl >= 0.5 else 0)


def cli_ranks(percentiles, c, n_pairs):
    return [percentile_rank(p, n_pairs) for p in percentiles] + [percentile_rank(100.0 * c, n_pairs), percentile_rank(100.0 * (1.0 - c), n_pairs)]


def gfold_of(lo, hi):
    if np.isnan(lo) or np.isnan(hi):
        return np.nan
    return lo if lo > 0 else hi if hi < 0 else 0.0


def fmt(v):
    """printf's %g; NaN as "nan" """
    return "nan" if np.isnan(v) else "%g" % v


def table(base_a, base_b, level, ids, have, dev, Sa, Sb, off, n_off, percentiles, c):
    """The text mmfold writes.  ids: the table's features; have[f]: feature f has a column in both trace files; dev: the device
    columns of the features with have[f], in order, for the ranks cli_ranks(percentiles, c, Sa Sb)."""
    nP = len(percentiles)
    L = ["# mmfold: posterior log fold change of A against B from all pairs of their draws, given the reads of these two libraries",
         "# A: %s" % base_a, "# B: %s" % base_b, "# level: %s" % level, "# Sa: %d" % Sa, "# Sb: %d" % Sb, "# offset: %s" % fmt(off),
         "# offset_features: %d" % n_off,
         "feature_id\tlog_mu_a\tlog_mu_b\tlfc\tsd\tp_gt\tn_gt\tn_eq\tgfold\tpercentiles" + ",".join(fmt(p) for p in percentiles) + "\tstatus"]
    d = derived(dev, Sa, Sb)
    at = 0
    for f, name in enumerate(ids):
        st = int(dev["status"][at]) if have[f] else NO_TRACE
        if st:
            cells = ["nan"] * 5 + ["0", "0", "nan", ",".join(["nan"] * nP)]
        else:
            q = dev["quantiles"][at]
            cells = [fmt(dev["mean_a"][at]), fmt(dev["mean_b"][at]), fmt(d["lfc"][at]), fmt(d["sd"][at]), fmt(d["p_gt"][at]),
                     str(int(dev["n_gt"][at])), str(int(dev["n_eq"][at])), fmt(gfold_of(q[nP], q[nP + 1])), ",".join(fmt(v) for v in q[:nP])]
        L.append("\t".join([name] + cells + [str(st)]))
        if have[f]:
            at += 1
    return ("\n".join(L) + "\n").encode()
