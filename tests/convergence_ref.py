"""numpy / scipy restatement of the convergence diagnostics of mmg_convergence_* (DESIGN.md section 11): the rank-normalized split
R-hat and the bulk and tail effective sample sizes of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), ESS as ArviZ's _ess.

A series is x[c, s]: C chains of S >= 4 draws.  Not a test module: tests import it."""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata


def split(x):
    """(M, N) split chains: chain c's first N and last N draws, N = S // 2 (for odd S the middle draw is dropped)."""
    x = np.asarray(x, np.float64)
    C, S = x.shape
    N = S // 2
    out = np.empty((2 * C, N))
    out[0::2] = x[:, :N]
    out[1::2] = x[:, S - N:]
    return out


def z_scores(y):
    """normal scores of the average ranks among all pooled draws, same shape as y"""
    P = y.size
    r = rankdata(y.ravel(), method="average").reshape(y.shape)
    return ndtri((r - 0.375) / (P + 0.25))


def rhat_split(y):
    """R-hat of the (M, N) split chains y, in IEEE arithmetic as written"""
    M, N = y.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        m = y.mean(axis=1)
        v = y.var(axis=1, ddof=1)
        W = v.mean()
        B = N * m.var(ddof=1)
        return float(np.sqrt(((N - 1) / N * W + B / N) / W))


def autocov(yj):
    """biased autocovariance of one chain at every lag: (1/N) sum_{n < N - t} (y[n] - m)(y[n + t] - m)"""
    N = yj.size
    d = yj - yj.mean()
    return np.correlate(d, d, mode="full")[N - 1:] / N


def ess_split(y, margin=False):
    """ArviZ's _ess over the (M, N) split chains y.  margin: also return the smallest |value| among the quantities Geyer's truncation
    compares with 0 (a device whose sums round differently may decide such a comparison the other way)"""
    M, N = y.shape
    P = M * N
    with np.errstate(divide="ignore", invalid="ignore"):
        acov = np.array([autocov(y[j]) for j in range(M)])
        chain_mean = y.mean(axis=1)
        mean_var = np.mean(acov[:, 0]) * N / (N - 1.0)
        var_plus = mean_var * (N - 1.0) / N
        var_plus += np.var(chain_mean, ddof=1)
        rho = np.zeros(N)
        rho[0] = 1.0
        even = 1.0
        odd = 1.0 - (mean_var - np.mean(acov[:, 1])) / var_plus
        rho[1] = odd
        t = 1
        near = [abs(even + odd)]
        while t < N - 3 and even + odd > 0:
            even = 1.0 - (mean_var - np.mean(acov[:, t + 1])) / var_plus
            odd = 1.0 - (mean_var - np.mean(acov[:, t + 2])) / var_plus
            near += [abs(even + odd), abs(even)]
            if even + odd >= 0:
                rho[t + 1] = even
                rho[t + 2] = odd
            t += 2
        max_t = t - 2
        if even > 0:
            rho[max_t + 1] = even
        t = 1
        while t <= max_t - 2:
            if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
                rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0
                rho[t + 2] = rho[t + 1]
            t += 2
        tau = -1.0 + 2.0 * np.sum(rho[: max_t + 1]) + rho[max_t + 1]
        tau = max(tau, 1.0 / np.log10(P))
        ess = float("nan") if np.isnan(rho).any() else float(P / tau)
        return (ess, float(np.nanmin(near + [np.inf]))) if margin else ess


def diagnostics(x):
    """dict(rhat, ess_bulk, ess_tail, rhat_bulk, rhat_tail, margin_bulk, margin_tail) of one series x[c, s] (margins: see ess_split)"""
    y = split(x)
    if np.all(y == y.flat[0]):
        nan = float("nan")
        return dict(rhat=nan, ess_bulk=nan, ess_tail=nan, rhat_bulk=nan, rhat_tail=nan, margin_bulk=np.inf, margin_tail=np.inf)
    P = y.size
    srt = np.sort(y.ravel())
    med = (srt[P // 2 - 1] + srt[P // 2]) / 2.0
    z = z_scores(y)
    zf = z_scores(np.abs(y - med))
    rb, rt = rhat_split(z), rhat_split(zf)
    q05, q95 = np.quantile(y, 0.05), np.quantile(y, 0.95)
    e_lo, n_lo = ess_split((y <= q05).astype(np.float64), margin=True)
    e_hi, n_hi = ess_split((y <= q95).astype(np.float64), margin=True)
    e_b, n_b = ess_split(z, margin=True)
    return dict(rhat=float(np.fmax(rb, rt)), ess_bulk=e_b, ess_tail=float(np.fmin(e_lo, e_hi)), rhat_bulk=rb, rhat_tail=rt,
                margin_bulk=n_b, margin_tail=min(n_lo, n_hi))


def diagnostics_of_traces(traces):
    """traces[c, s, i]: the three columns over the series i, as mmg_convergence_of_traces returns them"""
    traces = np.asarray(traces, np.float64)
    out = dict(rhat=[], ess_bulk=[], ess_tail=[], margin_bulk=[], margin_tail=[])
    for i in range(traces.shape[2]):
        d = diagnostics(traces[:, :, i])
        for k in out:
            out[k].append(d[k])
    return {k: np.array(v) for k, v in out.items()}
