"""numpy restatement of mmg_qvalues (include/mmgibbs.h), written from the definition and not from the kernels:
with m and m0 the observed and null values that are not NaN, -0.0 equal to 0.0, R(t) the observed values >= t, V(t) the null values
>= t,

    fdr(t) = min(1, (V(t) m) / (m0 R(t))),    q_f = min { fdr(t') : t' an observed value, t' <= obs_f },    null_ge_f = V(obs_f).

An observed NaN gets q = NaN and null_ge = 0 and counts in no R; with m0 = 0 every q is NaN.  Every quantity is an integer count or one
IEEE division of two products of counts, so the device must agree bit for bit.  `qvalues_loops` is the definition in plain loops (for
small inputs); `qvalues` counts with searchsorted (for large ones); tests/test_qvalue_ref.py holds them against each other."""
import numpy as np


def qvalues_loops(obs, null):
    obs = [float(x) for x in np.asarray(obs, np.float64).ravel()]
    null = [float(x) for x in np.asarray(null, np.float64).ravel()]
    seen = [t for t in obs if t == t]
    nulls = [t for t in null if t == t]
    m, m0 = len(seen), len(nulls)

    def fdr(t):
        V = sum(1 for x in nulls if x >= t)
        R = sum(1 for x in seen if x >= t)
        return min(1.0, (float(V) * float(m)) / (float(m0) * float(R))) if m0 else float("nan")

    q, ge = [], []
    for t in obs:
        if t != t:
            q.append(float("nan"))
            ge.append(0)
            continue
        ge.append(sum(1 for x in nulls if x >= t))
        best = fdr(t)
        for u in seen:
            if u <= t:
                v = fdr(u)
                best = v if v < best else best
        q.append(best)
    return np.array(ge, np.uint64), np.array(q, np.float64)


def qvalues(obs, null):
    obs = np.asarray(obs, np.float64).ravel()
    null = np.asarray(null, np.float64).ravel()
    ok = ~np.isnan(obs)
    o = obs[ok] + 0.0                       # (-0.0 + 0.0 is 0.0: the two zeros are one value)
    n = np.sort(null[~np.isnan(null)] + 0.0)
    m, m0 = o.size, n.size
    ge = np.zeros(obs.size, np.uint64)
    q = np.full(obs.size, np.nan)
    if m == 0:
        return ge, q
    V = m0 - np.searchsorted(n, o, side="left")
    R = m - np.searchsorted(np.sort(o), o, side="left")
    ge[ok] = V.astype(np.uint64)
    if m0 == 0:
        return ge, q
    fdr = np.minimum(1.0, (V.astype(np.float64) * float(m)) / (float(m0) * R.astype(np.float64)))
    up = np.argsort(o, kind="stable")       # ascending: the minimum over t' <= t runs along it (equal values have equal fdr)
    qs = np.empty(m)
    qs[up] = np.minimum.accumulate(fdr[up])
    q[ok] = qs
    return ge, q
