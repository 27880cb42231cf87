"""The specification of mmg_isoform_* (include/mmgibbs.h) in numpy, by brute force.  No device.

Input: a series-major trace tr (n, S), 1 <= S <= 4096, and groups: ordered lists of K >= 1 distinct rows of tr.  A member may be in
several groups, not twice in one.  Up to 8 thresholds in [0, 1), up to 64 zero-based ranks.

Per sample s of a group, with x_j = tr[m_j, s], every operation one IEEE double operation rounded once, in this order:
    valid      every x_j finite and >= 0, T_s finite and > 0.  One sample that is not valid makes the group invalid: status 1, every
               floating-point output NaN (its top / second rows NONE), every count 0, major 0.  Other groups are unaffected.
    T_s        ((0.0 + x_0) + x_1) + ... in list order
    top_s      the smallest j with x_j = the maximum (the draws are compared, never the proportions)
    second_s   the smallest j != top_s with x_j = the maximum over j != top_s; NONE = 0xffffffff when K = 1
    p_j        x_j / T_s;   P_s = x_top / T_s
    H_s        a = 0.0; for j ascending: if p_j > 0: a = a + p_j * log(p_j);  H_s = (-a) + 0.0   (-0.0 becomes +0.0)
               `log` is np.log by default; the device tests pass the library's own logarithm (mmg_selftest_math) for bit identity.
    above      x_j > theta_q * T_s
Per member of a group (flat order of the lists): n_top, n_second, n_above[q]: exact counts over the samples.
Per group: major = the smallest j with the largest n_top; n_distinct = #{j: n_top[j] > 0}; mean_H = lsum(H) / S,
ss_H = lsum((H - mean_H)^2), mean_P, ss_P alike, with pairs_ref.lsum (lane l of 64 adds its samples l, l + 64, ..., the 64 partial sums
folded by halving); q_H, q_P = the sorted series at the ranks, NaN for a rank >= S.

Derived on the host: p_top = n_top / S, sd = sqrt(ss / (S - 1)), eff_isoforms = exp(mean_H).  Two samples are independent given their
reads: P(major isoforms differ) = 1 - sum_j nA_top[j] nB_top[j] / (S_A S_B) (switch_probability_brute counts the pairs one by one).
"""
import numpy as np

from pairs_ref import lsum, _log_of

NONE = 0xffffffff
MAX_S, MAX_THRESHOLDS, MAX_RANKS = 4096, 8, 64


def check(groups, n, S, thresholds, ranks):
    if not 1 <= S <= MAX_S:
        raise ValueError("S")
    if len(groups) == 0:
        raise ValueError("no groups")
    if len(thresholds) > MAX_THRESHOLDS or len(ranks) > MAX_RANKS:
        raise ValueError("too many thresholds or ranks")
    for t in thresholds:
        if not (np.isfinite(t) and 0.0 <= t < 1.0):
            raise ValueError("threshold")
    for g, mem in enumerate(groups):
        if len(mem) == 0:
            raise ValueError("empty group %d" % g)
        if len(set(mem)) != len(mem):
            raise ValueError("duplicate in group %d" % g)
        if min(mem) < 0 or max(mem) >= n:
            raise ValueError("member out of range in group %d" % g)


def group_rows(x, log=np.log):
    """x: (K, S) the members' traces in list order -> valid (bool), T, top, second, H, P, each (S,)"""
    K, S = x.shape
    with np.errstate(all="ignore"):
        T = np.zeros(S)
        for j in range(K):
            T = T + x[j]
        ok = np.isfinite(x).all(axis=0) & (x >= 0).all(axis=0) & np.isfinite(T) & (T > 0)
        top = np.zeros(S, np.int64)
        second = np.full(S, NONE, np.int64)
        # from the definition: the first position that equals the maximum; then the same over the positions other than the top
        top = np.argmax(x == x.max(axis=0), axis=0)
        if K > 1:
            is_top = np.arange(K)[:, None] == top[None, :]
            rest = np.where(is_top, -np.inf, x)
            second = np.argmax((rest == rest.max(axis=0)) & ~is_top, axis=0)
        p = x / T[None, :]
        pos = p > 0
        term = p * _log_of(log, np.where(pos, p, 1.0))       # (one call of `log` per group: the device's costs a round trip)
        a = np.zeros(S)
        for j in range(K):
            a = np.where(pos[j], a + term[j], a)
        H = (-a) + 0.0
        P = x[top, np.arange(S)] / T
    return bool(ok.all()), T, top, second, H, P


def order_stats(v, ranks):
    srt = np.sort(v)
    return np.array([srt[r] if r < v.size else np.nan for r in ranks], np.float64)


def isoforms_ref(tr, groups, thresholds=(), ranks=(), log=np.log):
    """Every output of the device, in its layout: rows (G, S), member counts in the flat order of the lists, group columns (G,)"""
    tr = np.asarray(tr, np.float64)
    n, S = tr.shape
    groups = [[int(m) for m in g] for g in groups]
    thresholds = [float(t) for t in thresholds]
    ranks = [int(r) for r in ranks]
    check(groups, n, S, thresholds, ranks)
    G, nq, nr = len(groups), len(thresholds), len(ranks)
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    out = dict(ptr=ptr, top=np.empty((G, S), np.uint32), second=np.empty((G, S), np.uint32), H=np.empty((G, S)), P=np.empty((G, S)),
               status=np.zeros(G, np.uint8), major=np.zeros(G, np.uint32), n_distinct=np.zeros(G, np.uint32),
               n_top=np.zeros(ptr[-1], np.uint32), n_second=np.zeros(ptr[-1], np.uint32), n_above=np.zeros((ptr[-1], nq), np.uint32))
    for k in ("mean_H", "ss_H", "mean_P", "ss_P"):
        out[k] = np.full(G, np.nan)
    out["q_H"] = np.full((G, nr), np.nan)
    out["q_P"] = np.full((G, nr), np.nan)
    for g, mem in enumerate(groups):
        x = tr[mem]
        K = len(mem)
        valid, T, top, second, H, P = group_rows(x, log)
        if not valid:
            out["status"][g] = 1
            out["top"][g] = NONE
            out["second"][g] = NONE
            out["H"][g] = np.nan
            out["P"][g] = np.nan
            continue
        out["top"][g], out["second"][g], out["H"][g], out["P"][g] = top, second, H, P
        sl = slice(ptr[g], ptr[g + 1])
        out["n_top"][sl] = [(top == j).sum() for j in range(K)]
        out["n_second"][sl] = [(second == j).sum() for j in range(K)]
        with np.errstate(all="ignore"):
            for q, th in enumerate(thresholds):
                out["n_above"][sl, q] = [(x[j] > th * T).sum() for j in range(K)]
            nt = out["n_top"][sl]
            out["major"][g] = min(j for j in range(K) if nt[j] == nt.max())
            out["n_distinct"][g] = (nt > 0).sum()
            for name, v in (("H", H), ("P", P)):
                mean = lsum(v) / float(S)
                d = v - mean
                out["mean_" + name][g] = mean
                out["ss_" + name][g] = lsum(d * d)
                out["q_" + name][g] = order_stats(v, ranks)
    return out


def switch_probability_brute(top_a, top_b):
    """top_a (S_a,), top_b (S_b,): the top series of one group in two samples; the share of the S_a S_b pairs of draws whose tops differ"""
    differ = sum(1 for i in top_a for j in top_b if int(i) != int(j))
    return differ / float(len(top_a) * len(top_b))
