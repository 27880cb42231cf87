"""The specification of mmg_pairs_* (include/mmgibbs.h) in numpy.  No device.

Input: a transcript-major trace tr (n, S), S >= 1, and P >= 1 ordered pairs (a, b) of its rows, a != b.  The same pair may occur
twice, (a, b) and (b, a) may both occur, a member may be in any number of pairs.

Per sample s:    u_s = log(x_a[s]),  v_s = log(x_b[s]),  w_s = log(x_a[s] + x_b[s])        `log` is np.log by default; the device
                 tests pass the library's own logarithm (mmg_selftest_math) for bit identity.
Sums (`lsum`):   the order of assign_ref.row_probabilities: lane l of 64 adds its samples l, l + 64, ... ascending from 0.0 (a lane
                 without samples holds 0.0), the 64 partial sums are folded by halving, x[:32] + x[32:], then 16, 8, 4, 2, 1.
Pass 1:          mean_a = lsum(u) / S,  mean_b = lsum(v) / S,  mean_sum = lsum(w) / S
Pass 2:          du = u - mean_a, dv = v - mean_b, dw = w - mean_sum;
                 saa = lsum(du * du), sbb = lsum(dv * dv), sab = lsum(du * dv), sss = lsum(dw * dw)
                 -- each product rounded, then added: no fused multiply-add.
Count:           n_gt = #{s : x_a[s] > x_b[s]}, on the values themselves.
Non-finite values propagate, nothing is clamped: a trace value of 0 gives -inf, then NaN.

mean_a and saa depend on a alone: they carry the same bits in every pair a is in, and (b, a) returns (a, b)'s numbers with the sides
swapped and n_gt counted again.  Two passes because log mu of a well-covered transcript sits near -10 with an sd of a few
thousandths: the one-pass form would cancel six digits.

Derived on the host (IEEE sqrt and division):
    cor = sab / (sqrt(saa) * sqrt(sbb)),  sd_a = sqrt(saa / (S - 1)) (sd_b, sd_sum alike),  p_gt = n_gt / S
S = 1 and constant traces give NaN by the arithmetic, not by a special case.
"""
import numpy as np

from assign_ref import LANES, _fold

DEVICE_COLUMNS = ("mean_a", "mean_b", "mean_sum", "saa", "sbb", "sab", "sss", "n_gt")


def check_pairs(pairs, n):
    if len(pairs) == 0:
        raise ValueError("no pairs")
    for p, (a, b) in enumerate(pairs):
        if a == b:
            raise ValueError("pair %d: a == b" % p)
        if not (0 <= a < n and 0 <= b < n):
            raise ValueError("pair %d: member out of range" % p)


def lsum(x):
    """x: (..., S) -> (...): the sum in the order of a wave with one lane per sample"""
    x = np.asarray(x, np.float64)
    S = x.shape[-1]
    nb = (S + LANES - 1) // LANES
    with np.errstate(all="ignore"):
        A = np.zeros(x.shape[:-1] + (LANES,))
        for b in range(nb):                 # lane l: its samples in ascending order; the lanes past S keep what they hold
            blk = x[..., b * LANES:min(S, (b + 1) * LANES)]
            A[..., :blk.shape[-1]] = A[..., :blk.shape[-1]] + blk
        return _fold(A)


def _log_of(log, x):
    with np.errstate(all="ignore"):
        return np.asarray(log(np.ascontiguousarray(x, np.float64).ravel()), np.float64).reshape(np.shape(x))


def member_stats(x, log=np.log):
    """x: (m, S) -> mean (m,), the centred series (m, S), saa (m,)"""
    x = np.asarray(x, np.float64)
    S = x.shape[-1]
    with np.errstate(all="ignore"):
        u = _log_of(log, x)
        mean = lsum(u) / float(S)
        du = u - mean[..., None]
        return mean, du, lsum(du * du)


def pairs_ref(tr, pairs, log=np.log):
    """The eight device columns per pair, in the caller's pair order."""
    tr = np.asarray(tr, np.float64)
    n, S = tr.shape
    assert S >= 1
    pairs = [(int(a), int(b)) for a, b in pairs]
    check_pairs(pairs, n)
    a = np.array([p[0] for p in pairs])
    b = np.array([p[1] for p in pairs])
    members = np.unique(np.concatenate([a, b]))
    slot = {int(m): i for i, m in enumerate(members)}
    mean, cen, sq = member_stats(tr[members], log)          # once per member, whatever the number of its pairs
    sa = np.array([slot[int(m)] for m in a])
    sb = np.array([slot[int(m)] for m in b])
    with np.errstate(all="ignore"):
        xa, xb = tr[a], tr[b]
        w = _log_of(log, xa + xb)
        mean_sum = lsum(w) / float(S)
        dw = w - mean_sum[:, None]
        sss = lsum(dw * dw)
        sab = lsum(cen[sa] * cen[sb])
        n_gt = (xa > xb).sum(axis=1).astype(np.uint32)
    return dict(mean_a=mean[sa], mean_b=mean[sb], mean_sum=mean_sum, saa=sq[sa], sbb=sq[sb], sab=sab, sss=sss, n_gt=n_gt)


def derived(dev, S):
    """cor, sd_a, sd_b, sd_sum, p_gt from the device columns: what the Python wrapper and the CLI compute"""
    with np.errstate(all="ignore"):
        d = np.float64(S - 1)
        return dict(cor=dev["sab"] / (np.sqrt(dev["saa"]) * np.sqrt(dev["sbb"])), sd_a=np.sqrt(dev["saa"] / d), sd_b=np.sqrt(dev["sbb"] / d),
                    sd_sum=np.sqrt(dev["sss"] / d), p_gt=dev["n_gt"].astype(np.float64) / np.float64(S))


def summary_ref(tr, pairs, log=np.log):
    dev = pairs_ref(tr, pairs, log)
    dev.update(derived(dev, np.asarray(tr).shape[1]))
    return dev


# ---- the six-transcript problem of the statistical checks (tests/test_pairs_ref.py on the oracle's chain, tests/test_gpu_pairs.py
#      on the device's)
STAT_ROWS = [[0, 1], [2], [3], [4, 5], [4], [5]]
STAT_K = [1000, 300, 500, 400, 200, 200]
STAT_PAIRS = [(2, 3), (4, 5), (0, 1)]


def stat_problem():
    rp = np.concatenate([[0], np.cumsum([len(r) for r in STAT_ROWS])]).astype(np.uint64)
    ci = np.concatenate(STAT_ROWS).astype(np.uint32)
    return rp, ci, np.array(STAT_K, np.uint32), np.full(6, 1e-3)


def stat_rule(s, S=1024):
    """s: the summary of STAT_PAIRS over a chain of S kept samples.  (2, 3) have unique reads only, so their draws are independent
    and cor is about N(0, 1 / S); (4, 5) share 400 reads and are anchored by 200 unique each; (0, 1) share everything."""
    z = 5.0 / np.sqrt(S - 1.0)
    assert abs(s["cor"][0]) < z, s["cor"][0]
    assert s["cor"][1] < -z and s["sd_sum"][1] < min(s["sd_a"][1], s["sd_b"][1]), (s["cor"][1], s["sd_sum"][1], s["sd_a"][1], s["sd_b"][1])
    assert s["sd_sum"][2] < 0.1 * min(s["sd_a"][2], s["sd_b"][2]), (s["sd_sum"][2], s["sd_a"][2], s["sd_b"][2])
