"""numpy restatement of mmdiff -lrt (mmseq_amd/csrc/diff_lrt_kernels.h, host/lrt_stats.hpp), vectorised over
features: the same fp64 operations in the same order, dlog / dexp through the oracle (tests/mmdiff_ref.py), so the device's
results are compared with `==`.  A lane that has left (status 2, or done) waits behind a mask while the others go on.

Per feature and model: y_i ~ N((X theta)_i, v_i), v_i = e_i^2 + sigma^2_{C(i)}, l = -1/2 sum_i [log 2 pi + log v_i + r_i^2 / v_i].
theta is weighted least squares for fixed sigma^2 (Cholesky of X'WX); sigma^2 moves by projected Fisher scoring, the step halved
while l does not increase."""
import math

import numpy as np

from mmdiff_ref import dexp, dlgamma, dlog, fmt, is_nil

MAX_ITERS, MAX_HALVINGS, TOL, PIVOT_TOL = 200, 30, 1e-12, 1e-10
LOG2PI = 1.8378770664093453
ST_CAP, ST_SINGULAR, ST_BOUNDARY = 1, 2, 4
GAMMA_ITMAX, GAMMA_EPS, GAMMA_FPMIN = 100000, 1e-16, 1e-300


def design_matrix(M, P, fixalpha):
    """X = [1 unless fixalpha | M unless nil | P unless nil], (N, p)."""
    M, P = np.asarray(M, np.float64), np.asarray(P, np.float64)
    cols = [] if fixalpha else [np.ones((M.shape[0], 1))]
    if not is_nil(M):
        cols.append(M)
    if not is_nil(P):
        cols.append(P)
    return np.concatenate(cols, 1) if cols else np.zeros((M.shape[0], 0))


def _tri(j, k):
    return j * (j + 1) // 2 + k


def evaluate(X, cls, y, esq, sig):
    """theta (p, F), l (F,) and ok (F,) at the variances sig (nc, F); y, esq (N, F)."""
    N, p = X.shape
    F = y.shape[1]
    A = np.zeros((p * (p + 1) // 2, F))
    T = np.zeros((p, F))
    ok = np.ones(F, bool)
    with np.errstate(all="ignore"):
        for i in range(N):
            v = esq[i] + sig[cls[i]]
            w = 1.0 / v
            ok &= (v > 0.0) & (v < np.inf) & (w < np.inf)
            for j in range(p):
                xw = X[i, j] * w
                T[j] = T[j] + xw * y[i]
                o = _tri(j, 0)         # row j of the triangle is contiguous: every A[j, k] += xw * X[i, k], k <= j, at once
                A[o:o + j + 1] = A[o:o + j + 1] + xw[None, :] * X[i, :j + 1, None]
        for j in range(p):
            for k in range(j):
                s = A[_tri(j, k)].copy()
                for q in range(k):
                    s -= A[_tri(j, q)] * A[_tri(k, q)]
                A[_tri(j, k)] = s / A[_tri(k, k)]
            ajj = A[_tri(j, j)].copy()
            d = ajj.copy()
            for q in range(j):
                d -= A[_tri(j, q)] * A[_tri(j, q)]
            ok &= d > PIVOT_TOL * ajj
            A[_tri(j, j)] = np.sqrt(d)
        for j in range(p):
            s = T[j].copy()
            for k in range(j):
                s -= A[_tri(j, k)] * T[k]
            T[j] = s / A[_tri(j, j)]
        for j in range(p - 1, -1, -1):
            s = T[j].copy()
            for k in range(j + 1, p):
                s -= A[_tri(k, j)] * T[k]
            T[j] = s / A[_tri(j, j)]
        acc = np.zeros(F)
        for i in range(N):
            v = esq[i] + sig[cls[i]]
            m = np.zeros(F)
            for j in range(p):
                m += X[i, j] * T[j]
            r = y[i] - m
            acc += (LOG2PI + dlog(np.where(ok, v, 1.0))) + r * r / v
    return T, -0.5 * acc, ok


def fit(X, cls, y, e, max_iters=0):
    """One model of every feature: y, e (F, N).  dict(loglik (F,), theta (p, F), sigmasq (nc, F), iters, status (F,) uint32)."""
    X = np.asarray(X, np.float64)
    cls = np.asarray(cls, np.int64)
    yT = np.ascontiguousarray(np.asarray(y, np.float64).T)
    e = np.asarray(e, np.float64)
    with np.errstate(over="ignore"):
        esq = np.ascontiguousarray((e * e).T)
    N, p = X.shape
    F = yT.shape[1]
    nc = int(cls.max()) + 1
    cap = int(max_iters) if max_iters else MAX_ITERS
    sig = np.zeros((nc, F))
    for c in range(nc):
        sm, n = np.zeros(F), 0.0
        for i in range(N):
            if cls[i] == c:
                sm = sm + esq[i]
                n += 1.0
        sig[c] = sm / n
    theta, l, ok = evaluate(X, cls, yT, esq, sig)
    singular = ~ok
    active = ok.copy()                 # lanes still in the scoring loop
    converged = np.zeros(F, bool)
    iters = np.zeros(F, np.uint32)
    it = 0
    with np.errstate(all="ignore"):
        while it < cap and active.any():
            it += 1
            iters[active] = it
            step = np.zeros((nc, F))
            cand = np.zeros((nc, F))
            move = np.zeros(F, bool)
            finite = np.ones(F, bool)
            for c in range(nc):
                U, I = np.zeros(F), np.zeros(F)
                for i in range(N):
                    if cls[i] == c:
                        v = esq[i] + sig[c]
                        w = 1.0 / v
                        m = np.zeros(F)
                        for j in range(p):
                            m += X[i, j] * theta[j]
                        r = yT[i] - m
                        w2 = w * w
                        U += r * r * w2 - w
                        I += w2
                dl = U / I
                finite &= np.abs(dl) < np.inf
                s1 = sig[c] + dl
                sc = np.where(s1 > 0.0, s1, 0.0)
                step[c], cand[c] = dl, sc
                move |= sc != sig[c]
            bad = active & ~finite
            singular |= bad
            active &= finite
            still = active & ~move
            converged |= still
            active &= move
            # the halving loop of the lanes that move
            trying = active.copy()
            accepted = np.zeros(F, bool)
            lnew = l.copy()
            tnew = theta.copy()
            h = 1.0
            for hv in range(MAX_HALVINGS + 1):
                if not trying.any():
                    break
                if hv > 0:
                    h = h * 0.5
                    s1 = sig + h * step
                    cand = np.where(trying, np.where(s1 > 0.0, s1, 0.0), cand)
                t_, l_, ok_ = evaluate(X, cls, yT, esq, cand)
                bad = trying & ~ok_
                singular |= bad
                active &= ~bad
                trying &= ~bad
                up = trying & (l_ > l)
                lnew = np.where(up, l_, lnew)
                tnew = np.where(up, t_, tnew)
                accepted |= up
                trying &= ~up
            # no halved step raised l: the current point stands (theta fitted there again gives what it was)
            stuck = active & ~accepted
            converged |= stuck
            active &= accepted
            gain = lnew - l
            sig = np.where(active, cand, sig)
            theta = np.where(active, tnew, theta)
            l = np.where(active, lnew, l)
            done = active & (gain <= TOL)
            converged |= done
            active &= ~done
    status = np.where(converged, 0, ST_CAP).astype(np.uint32)
    status |= np.where((sig == 0.0).any(0), ST_BOUNDARY, 0).astype(np.uint32)
    status[singular] = ST_SINGULAR
    iters[singular] = 0
    l = np.where(singular, np.nan, l)
    theta = np.where(singular, np.nan, theta)
    sig = np.where(singular, np.nan, sig)
    return dict(loglik=l, theta=theta, sigmasq=sig, iters=iters, status=status)


# ----------------------------------------------------------------------------- the derived statistics (host/lrt_stats.hpp)
def _f(x):
    return float(np.asarray(x).ravel()[0])


def gamma_q(a, x):
    if not (a > 0.0) or not (x >= 0.0) or not (a < math.inf):
        return math.nan
    if x == 0.0:
        return 1.0
    if x == math.inf:
        return 0.0
    pre = _f(dexp((-x + a * _f(dlog(x))) - _f(dlgamma(a))))
    if x < a + 1.0:
        ap, dl = a, 1.0 / a
        sm = dl
        for _ in range(GAMMA_ITMAX):
            ap = ap + 1.0
            dl = dl * x / ap
            sm = sm + dl
            if abs(dl) < abs(sm) * GAMMA_EPS:
                break
        return 1.0 - sm * pre
    b, c = (x + 1.0) - a, 1.0 / GAMMA_FPMIN
    d = 1.0 / b
    h = d
    for i in range(1, GAMMA_ITMAX + 1):
        an = -float(i) * (float(i) - a)
        b = b + 2.0
        d = an * d + b
        if abs(d) < GAMMA_FPMIN:
            d = GAMMA_FPMIN
        c = b + an / c
        if abs(c) < GAMMA_FPMIN:
            c = GAMMA_FPMIN
        d = 1.0 / d
        dl = d * c
        h = h * dl
        if abs(dl - 1.0) < GAMMA_EPS:
            break
    return pre * h


def chi2_sf(df, stat):
    if df <= 0 or stat != stat:
        return math.nan
    return gamma_q(0.5 * float(df), 0.5 * (stat if stat > 0.0 else 0.0))


def bh_qvalues(p):
    p = np.asarray(p, np.float64)
    q = np.full(p.shape, np.nan)
    idx = [i for i in range(len(p)) if p[i] == p[i]]
    idx.sort(key=lambda i: p[i])          # (stable: ties keep the input order)
    m = float(len(idx))
    run = 1.0
    for r in range(len(idx) - 1, -1, -1):
        v = p[idx[r]] * m / float(r + 1)
        if v < run:
            run = v
        q[idx[r]] = run
    return q


def lrt(y, e, M, P0, P1, C, fixalpha=False, max_iters=0):
    """What DiffLrt(...).results() returns."""
    C = np.asarray(C, np.int64)
    X = [design_matrix(M, P, fixalpha) for P in (P0, P1)]
    r = [fit(X[m], C[:, m], y, e, max_iters) for m in range(2)]
    nc = [int(C[:, m].max()) + 1 for m in range(2)]
    df = (X[1].shape[1] + nc[1]) - (X[0].shape[1] + nc[0])
    ll = np.stack([r[0]["loglik"], r[1]["loglik"]])
    stat = 2.0 * (ll[1] - ll[0])
    p = np.array([chi2_sf(df, float(s)) for s in stat])
    return dict(loglik=ll, stat=stat, p_value=p, q_value=bh_qvalues(p), df=df, theta0=r[0]["theta"], theta1=r[1]["theta"],
                sigmasq0=r[0]["sigmasq"], sigmasq1=r[1]["sigmasq"], iters=np.stack([r[0]["iters"], r[1]["iters"]]),
                status=np.stack([r[0]["status"], r[1]["status"]]), n_cols=(X[0].shape[1], X[1].shape[1]), n_classes=tuple(nc))


def lrt_file(feats, r, M, P0, P1, fixalpha):
    """The text of `mmdiff -lrt FILE` for the results r of `lrt` (or of DiffLrt)."""
    M, P = np.asarray(M, np.float64), [np.asarray(P0, np.float64), np.asarray(P1, np.float64)]
    Mnil, Pnil, K, L = is_nil(M), [is_nil(P[0]), is_nil(P[1])], M.shape[1], [P[0].shape[1], P[1].shape[1]]
    nc = [r["sigmasq0"].shape[0], r["sigmasq1"].shape[0]]
    hdr = ["feature_id", "loglik0", "loglik1", "lrt_stat", "df", "p_value", "q_value", "alpha0", "alpha1"]
    hdr += ["beta%d_%d" % (m, k) for m in range(2) for k in range(K)]
    hdr += ["eta%d_%d" % (m, l) for m in range(2) for l in range(L[m])]
    hdr += ["sigmasq%d_%d" % (m, c) for m in range(2) for c in range(nc[m])]
    hdr += ["iters0", "iters1", "status0", "status1"]
    out = ["\t".join(hdr) + "\n"]
    th = [r["theta0"], r["theta1"]]
    sg = [r["sigmasq0"], r["sigmasq1"]]
    for f in range(len(feats)):
        row = [feats[f], fmt(r["loglik"][0, f]), fmt(r["loglik"][1, f]), fmt(r["stat"][f]), "%d" % r["df"], fmt(r["p_value"][f]), fmt(r["q_value"][f])]
        a_of = [0, 0]
        for m in range(2):
            row.append("NA" if fixalpha else fmt(th[m][0, f]))
            a_of[m] = 0 if fixalpha else 1
        for m in range(2):
            row += ["NA" if Mnil else fmt(th[m][a_of[m] + k, f]) for k in range(K)]
        for m in range(2):
            o = a_of[m] + (0 if Mnil else K)
            row += ["NA" if Pnil[m] else fmt(th[m][o + l, f]) for l in range(L[m])]
        for m in range(2):
            row += [fmt(sg[m][c, f]) for c in range(nc[m])]
        row += ["%d" % r["iters"][0, f], "%d" % r["iters"][1, f], "%d" % r["status"][0, f], "%d" % r["status"][1, f]]
        out.append("\t".join(row) + "\n")
    return "".join(out)
