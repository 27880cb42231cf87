"""The specification of the posterior assignment probabilities (mmg_assign_*), restated in numpy.  No device.

For a hit j of row i (columns c_0 .. c_{L-1} in stored order) and the samples s of a range of a transcript-major trace tr[t, s]:

    D = 0; for j ascending: D += tr[c_j, s]                    one rounding per addition
    D > 0 and D < inf:  r = 1.0 / D;  p_j = tr[c_j, s] * r
    otherwise:          p_j = 1.0 / (double)L                   (the oracle's degenerate case, orc_categorical)

A row of one hit has p = 1.0 whatever the trace holds: the sample kernel draws nothing for it either, and the product above would
miss 1 by a rounding for one value in seven.

The sum over the samples runs in the order of a wave with one lane per sample: the range is padded to a multiple of 64 with p = 0,
lane l adds its samples l, l + 64, ... in ascending order, and the 64 partial sums are folded by halving, x[:32] + x[32:], then 16, 8,
4, 2, 1.  P_j = A_j / (double)S.  Every operation is an IEEE double operation rounded once.
"""
import numpy as np

LANES = 64


def _fold(x):
    """x: (..., 64) -> (...): the halving order."""
    w = LANES
    while w > 1:
        w //= 2
        x = x[..., :w] + x[..., w:2 * w]
    return x[..., 0]


def conditional_probabilities(v):
    """v: (L, S) trace values of one row's hits -> p (L, S), the assignment probabilities given each sample."""
    v = np.ascontiguousarray(v, np.float64)
    L, S = v.shape
    if L == 1:                              # nothing to divide: v * (1 / v) is not 1 for one double in seven (49.0 * (1.0 / 49.0) < 1)
        return np.ones((1, S))
    with np.errstate(all="ignore"):
        D = np.zeros(S)
        for j in range(L):                  # sequential, one rounding per addition
            D = D + v[j]
        ok = (D > 0) & (D < np.inf)
        r = 1.0 / np.where(ok, D, 1.0)
        return np.where(ok[None, :], v * r[None, :], 1.0 / float(L))


def row_probabilities(v):
    """v: (L, S) trace values of one row's hits over the samples of the range -> P (L,)."""
    p = conditional_probabilities(v)
    L, S = p.shape
    with np.errstate(all="ignore"):
        nb = (S + LANES - 1) // LANES
        pad = np.zeros((L, nb * LANES))
        pad[:, :S] = p
        pad = pad.reshape(L, nb, LANES)
        A = np.zeros((L, LANES))
        for b in range(nb):                 # lane l: its samples in ascending order
            A = A + pad[:, b, :]
        return _fold(A) / float(S)


def sample_probabilities(row_ptr, col_idx, mu):
    """The conditional assignment probabilities of ONE sample mu[t] (no sum over samples): p per hit."""
    row_ptr = np.asarray(row_ptr).astype(np.int64)
    col_idx = np.asarray(col_idx).astype(np.int64)
    out = np.empty(col_idx.size)
    for i in range(row_ptr.size - 1):
        b, e = row_ptr[i], row_ptr[i + 1]
        if e > b:
            out[b:e] = row_probabilities(mu[col_idx[b:e], None])
    return out


def assign_ref(row_ptr, col_idx, tr, first=0, count=None):
    """P per hit, in hit order.  tr: (n_tx, trace_len) transcript-major; the samples [first, first + count)."""
    row_ptr = np.asarray(row_ptr).astype(np.int64)
    col_idx = np.asarray(col_idx).astype(np.int64)
    tr = np.asarray(tr, np.float64)
    count = tr.shape[1] - first if count is None else count
    assert 0 <= first and count >= 1 and first + count <= tr.shape[1]
    sub = tr[:, first:first + count]
    out = np.empty(col_idx.size)
    for i in range(row_ptr.size - 1):
        b, e = row_ptr[i], row_ptr[i + 1]
        if e > b:
            out[b:e] = row_probabilities(sub[col_idx[b:e]])
    return out


def expected_hits(row_ptr, col_idx, P, n_tx, k=None):
    """expected_hits[t] = sum of k_i P_j over the hits with c_j = t, in ascending hit index."""
    row_ptr = np.asarray(row_ptr).astype(np.int64)
    L = np.diff(row_ptr)
    kk = np.ones(L.size) if k is None else np.asarray(k, np.float64)
    w = np.repeat(kk, L) * np.asarray(P, np.float64)
    out = np.zeros(n_tx)
    np.add.at(out, np.asarray(col_idx).astype(np.int64), w)
    return out


# ---- the statistical check that P is the probability of what the sampler draws (tests/test_assign_ref.py on the oracle's chain,
#      tests/test_gpu_assign.py on the device's)
def stat_problem():
    """400 rows over 60 transcripts with multiplicities; some transcripts only have rows of their own"""
    rng = np.random.default_rng(2024)
    n_tx = 60
    lengths = rng.integers(1, 6, 400)
    rows = []
    for i, l in enumerate(lengths):
        if i < 12:
            rows.append(np.array([48 + i]))                 # transcripts 48 .. 59: unique hits only
        else:
            t0 = rng.integers(0, 48)
            rows.append(np.sort(rng.choice(np.arange(max(0, t0 - 4), min(48, t0 + 5)), min(l, 5), replace=False)))
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint64)
    ci = np.concatenate(rows).astype(np.uint32)
    k = rng.integers(1, 40, 400).astype(np.uint32)
    k[::50] = 900                                            # rows on the conditional-binomial chain
    l = rng.uniform(0.5, 3.0, n_tx) * 1e-3
    return rp, ci, k, l, n_tx


def stat_rule(rp, ci, k, trace, counts):
    """counts[s]: the reads per transcript drawn in iteration s (from the mu of sample s - 1).  d_s = counts[s + 1] - E_s with
    E_s[t] = sum_i k_i p_it given sample s has conditional mean zero given the past, so the d_s are uncorrelated and sd / sqrt(n) is
    the standard error of their mean.  Every transcript: |mean d| <= 5 sd / sqrt(n); sd = 0 only with d = 0 throughout."""
    n_tx, S = trace.shape
    E = np.zeros((n_tx, S))
    rpi = np.asarray(rp).astype(np.int64)
    for i in range(rpi.size - 1):
        cols = np.asarray(ci[rpi[i]:rpi[i + 1]]).astype(np.int64)
        np.add.at(E, cols, float(k[i]) * conditional_probabilities(trace[cols]))
    d = np.asarray(counts, np.float64)[1:].T - E[:, :-1]     # (n_tx, S - 1)
    n = d.shape[1]
    mean, sd = d.mean(axis=1), d.std(axis=1, ddof=1)
    worst = 0.0
    for t in range(n_tx):
        if sd[t] == 0.0:
            assert np.all(d[t] == 0.0), t
        else:
            z = abs(mean[t]) / (sd[t] / np.sqrt(n))
            worst = max(worst, z)
            assert z <= 5.0, (t, z)
    return worst, int((sd == 0.0).sum()), E
