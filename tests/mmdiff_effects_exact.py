"""The exact within-model marginal posterior of mmdiff's alpha, beta and eta, by the quadrature of tests/mmdiff_exact.py.

numpy and scipy only; no sampler and no random number.  Given lambda and sigma^2 (one grid node of mmdiff_exact._Model) the
coefficients c = (alpha, beta, eta) are jointly Gaussian: precision A = X' W X + V0^-1 with W = diag(1 / (e^2 + sigma^2_C)) and
V0 = diag(25, v_beta, .., lambda_1, ..), mean A^-1 X' W y (mmdiff_exact._Model.cond_means).  Coefficient i at that node is
N(mean_i, (A^-1)_ii).  Weighted by the nodes' posterior weights exp(log_terms - logsumexp(log_terms)) the marginal posterior of
coefficient i is a mixture of Gaussians, which gives its mean, its standard deviation
    sd^2 = sum_b w_b (var_b + mean_b^2) - (sum_b w_b mean_b)^2,
its distribution function F(x) = sum_b w_b Phi((x - mean_b) / sqrt(var_b)) and P(> 0) = 1 - F(0).

moments() streams over the grid and keeps nothing per node: it is what the refinement test runs on the refined grid.  mixture() keeps
the nodes, without the lightest ones whose weights add up to less than 1e-12, so that F can be evaluated later at many points.
"""
import numpy as np
from scipy.special import logsumexp, ndtr

from mmdiff_exact import DEFAULT_GRID, _Model


def names(m):
    return (["alpha"] if m.has_alpha else []) + ["beta_%d" % k for k in range(m.K)] + ["eta_%d" % l for l in range(m.L)]


def _node_gaussians(m, lo, hi):
    """Means (B, p) and variances (B, p) of the coefficients at grid points lo .. hi - 1: the A of _Model.cond_means."""
    lam, sig, _ = m.chunk(lo, hi)
    X = np.concatenate([m.Xf, m.P], 1)
    w = 1.0 / (m.e2 + sig[:, m.cl])
    A = np.einsum("ia,bi,ic->bac", X, w, X)
    prec = np.concatenate([np.broadcast_to(1.0 / m.vf, (hi - lo, m.vf.size)), 1.0 / lam], 1)
    p = X.shape[1]
    A[:, np.arange(p), np.arange(p)] += prec
    var = np.diagonal(np.linalg.inv(A), axis1=1, axis2=2)
    return m.cond_means(lo, hi), var


def moments(y, e, M, P, classes, d=1.4, s=2.0, fixalpha=False, grid=DEFAULT_GRID, at=()):
    """names, mean (p,), sd (p,) and cdf (p, len(at)) of the coefficients' marginal posteriors under one model."""
    m = _Model(y, e, M, P, classes, d, s, fixalpha, grid)
    at = np.asarray(at, np.float64).ravel()
    p = m.Xf.shape[1] + m.L
    lt = m.log_terms()
    w = np.exp(lt - logsumexp(lt))
    m1, m2, cdf = np.zeros(p), np.zeros(p), np.zeros((p, at.size))
    for lo in range(0, m.size, m.batch()):
        hi = min(lo + m.batch(), m.size)
        mu, var = _node_gaussians(m, lo, hi)
        wb = w[lo:hi]
        m1 += wb @ mu
        m2 += wb @ (var + mu * mu)
        if at.size:
            z = (at[None, None, :] - mu[:, :, None]) / np.sqrt(var)[:, :, None]
            cdf += np.einsum("b,bpa->pa", wb, ndtr(z))
    return dict(names=names(m), mean=m1, sd=np.sqrt(m2 - m1 * m1), cdf=cdf)


class Mixture:
    """The marginal posteriors of one model's coefficients as Gaussian mixtures over the grid nodes that carry 1 - 1e-12 of the weight."""

    def __init__(self, nm, w, mu, var):
        self.names, self.w, self.mu, self.var = nm, w, mu, var

    def index(self, name):
        return self.names.index(name)

    def mean(self, name):
        return float(self.w @ self.mu[:, self.index(name)])

    def sd(self, name):
        i = self.index(name)
        m1 = self.w @ self.mu[:, i]
        return float(np.sqrt(self.w @ (self.var[:, i] + self.mu[:, i] ** 2) - m1 * m1))

    def cdf(self, name, x, block=4000):
        i = self.index(name)
        x = np.asarray(x, np.float64)
        flat = x.ravel()
        out = np.zeros(flat.size)
        sd = np.sqrt(self.var[:, i])
        for lo in range(0, self.w.size, block):
            sl = slice(lo, lo + block)
            out += self.w[sl] @ ndtr((flat[None, :] - self.mu[sl, i, None]) / sd[sl, None])
        return out.reshape(x.shape)

    def p_gt0(self, name):
        return 1.0 - float(self.cdf(name, 0.0))


def mixture(y, e, M, P, classes, d=1.4, s=2.0, fixalpha=False, grid=DEFAULT_GRID, drop=1e-12):
    m = _Model(y, e, M, P, classes, d, s, fixalpha, grid)
    lt = m.log_terms()
    w = np.exp(lt - logsumexp(lt))
    order = np.argsort(w)
    light = order[np.cumsum(w[order]) < drop]
    keep = np.ones(w.size, bool)
    keep[light] = False
    mus, vars_ = [], []
    for lo in range(0, m.size, m.batch()):
        hi = min(lo + m.batch(), m.size)
        k = keep[lo:hi]
        if not k.any():
            continue
        mu, var = _node_gaussians(m, lo, hi)
        mus.append(mu[k])
        vars_.append(var[k])
    wk = w[keep]
    return Mixture(names(m), wk / wk.sum(), np.concatenate(mus), np.concatenate(vars_))
