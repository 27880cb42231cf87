"""Exact marginal likelihoods of mmdiff's two models, by quadrature: the answer mmdiff's chain estimates, from the model alone.

numpy and scipy only.  Nothing here comes from tests/mmdiff_ref.py, the package or the oracle, and nothing restates
mmseq_amd/csrc/diff_kernels.h: there is no sampler, no pseudoprior and no random number in this file.

The model of one feature (y_i the estimate of sample i, e_i its standard deviation), model j of the two:

    alpha ~ N(0, 25)                                 absent with fixalpha (alpha = 0, no prior)
    beta ~ N(0, v_beta I)                            v_beta = 4, or 25 with fixalpha; absent when M is nil
    eta_l | lambda_l ~ N(0, lambda_l)                one per column of P; absent when P is nil
    lambda_l ~ InvGamma(d, s)
    sigma^2_c | rho ~ InvGamma(k / 2, k rho / 2)     one per variance class, k = 4
    rho ~ Gamma(q, rate r)                           q = 1.2, r = 2
    y_i ~ N(alpha + (M beta)_i + (P eta)_i, e_i^2 + sigma^2_{C(i)})

A design matrix is *nil* when it has one column and that column is constant (max - min < 1e-5): it stands for "no such term",
and the model then has no beta (for M) or no eta and no lambda (for P).  This is the rule of src/bms.cpp:1154-1156, and it is part
of the model, not of the sampler: `-de 3 3` writes P0 as a column of ones, which is nil, so model 0 of `-de` is alpha, one sigma^2
and rho, and only model 1 carries an eta.  (Reading that column of ones as a design column gives model 0 a second intercept with
a heavy-tailed prior and moves log BF by about +0.08 on the fixture rows of tests/test_mmdiff_exact.py.)

Under the Carlin-Chib scheme of src/bms.cpp the stationary odds of gamma are p' / (1 - p') * m1 / m0 for any pseudoprior, m_j the
marginal likelihood of model j, so logit(mean gamma) - logit(p') estimates log_bf().  The sampler's target (log_target_posterior)
omits the (2 pi)^(-1/2) of every Gaussian factor: N of the likelihood and one per alpha, beta and eta.  Its pseudoprior density
(log_target_pseudo) omits the one per alpha, beta and eta of the same model.  The log odds are
[post_1 - pseudo_1] - [post_0 - pseudo_0], so per model the alpha, beta and eta factors cancel inside the bracket whatever the
numbers of columns are, and the N of the likelihood cancel between the brackets.  Checked once against both functions; m_j below
carries every constant, so log_marginal() is the true log marginal likelihood.

The integral.  Given lambda and sigma^2, alpha, beta and eta integrate out as a Gaussian:
    y ~ N(0, diag(e^2 + sigma^2_C) + X V0 X'),  X = [1 | M | P],  V0 = diag(25, v_beta, .., lambda_1, ..),
evaluated through the determinant lemma (the covariance itself is too ill-conditioned at the far end of the lambda axis).
rho integrates out of the sigma^2 prior in closed form:
    p(sigma^2_1..n) = (k/2)^(n k/2) / Gamma(k/2)^n * prod_c sigma^2_c^-(k/2+1) * r^q / Gamma(q)
                      * Gamma(q + n k/2) / (r + (k/2) sum_c 1/sigma^2_c)^(q + n k/2).
What remains is a trapezoid grid over (log lambda_l, log sigma^2_c), one dimension per eta column and per variance class, with
the Jacobian lambda * sigma^2 of the change of variables.  The integrand is analytic and decays at both ends of every axis, so
the trapezoid rule converges geometrically in the step; tests/test_mmdiff_exact.py records how little a finer, wider grid moves it.

Out of reach: more than 4 grid dimensions.  A design with three groups has 3 eta columns and 3 variance classes, 6 dimensions;
that needs another method and is out of scope here.  The functions refuse such a design; they do not fall back to Monte Carlo.
"""
import math

import numpy as np
from scipy.special import gammaln, logsumexp

K_SIG, Q_RHO, R_RHO = 4.0, 1.2, 2.0
V_ALPHA = 25.0
MAX_DIMS = 4
LOG2PI = math.log(2.0 * math.pi)


class Grid:
    """Trapezoid grid over log lambda in `lam` and log sigma^2 in `sig`.  Points per axis: `n_small` = (lambda, sigma^2) when the
    model has at most 2 grid dimensions, `n_large` when it has 3 or 4.  `pin` = (lambda, sigma^2) collapses the grid to that one
    point: the result is then the integrand as a density in (lambda, sigma^2) there -- log N(y; 0, Sigma) plus the log priors of
    lambda and sigma^2 -- with no Jacobian and no weight.

    The default: log lambda in [-10, 30] with 240 / 160 points, log sigma^2 in [-18, 12] with 150 / 113 points (a step of 0.17 to
    0.27).  The lower end of log sigma^2 matters: with two variance classes and replicates that agree within their e_i, the
    likelihood peaks at sigma^2 -> 0 while prior * Jacobian falls only as sigma^2^1.2 along sigma^2_1 = sigma^2_2, and a lower
    end of -12 left 2.7e-5 of log m_1 outside the grid on the second fixture row.  -18 leaves under 1e-7."""

    def __init__(self, lam=(-10.0, 30.0), sig=(-18.0, 12.0), n_small=(240, 150), n_large=(160, 113), pin=None):
        self.lam, self.sig, self.n_small, self.n_large, self.pin = tuple(lam), tuple(sig), tuple(n_small), tuple(n_large), pin

    def refined(self, widen=5.0):
        """Half the step, both ranges wider by `widen` at each end."""
        def n2(n, r):
            step = (r[1] - r[0]) / (n - 1) / 2.0
            return int(math.ceil((r[1] - r[0] + 2.0 * widen) / step)) + 1
        lam, sig = (self.lam[0] - widen, self.lam[1] + widen), (self.sig[0] - widen, self.sig[1] + widen)
        return Grid(lam, sig, (n2(self.n_small[0], self.lam), n2(self.n_small[1], self.sig)),
                    (n2(self.n_large[0], self.lam), n2(self.n_large[1], self.sig)))

    def coarsened(self, factor=0.75):
        """`factor` times the points on the same ranges."""
        c = lambda n: max(int(n * factor), 2)
        return Grid(self.lam, self.sig, tuple(map(c, self.n_small)), tuple(map(c, self.n_large)))

    def axis(self, which, dims):
        """(points, log weights) of one axis in the log variable."""
        n = (self.n_small if dims <= 2 else self.n_large)[0 if which == "lam" else 1]
        lo, hi = self.lam if which == "lam" else self.sig
        x = np.linspace(lo, hi, n)
        w = np.full(n, (hi - lo) / (n - 1))
        w[0] *= 0.5
        w[-1] *= 0.5
        return x, np.log(w)


DEFAULT_GRID = Grid()


def is_nil(X):
    """One constant column (or no matrix at all): the term is absent from the model."""
    if X is None:
        return True
    X = np.asarray(X, np.float64)
    return X.shape[1] == 0 or (X.shape[1] == 1 and X.max() - X.min() < 0.00001)


def log_prior_lambda(lam, d, s):
    """log InvGamma(lam; d, s)."""
    lam = np.asarray(lam, np.float64)
    return d * math.log(s) - gammaln(d) - (d + 1.0) * np.log(lam) - s / lam


def log_prior_sigmasq(sig):
    """log p(sigma^2_1..n), rho integrated out; sig (..., n)."""
    sig = np.asarray(sig, np.float64)
    n = sig.shape[-1]
    h = K_SIG / 2.0
    a = Q_RHO + n * h
    return (n * (h * math.log(h) - gammaln(h)) - (h + 1.0) * np.log(sig).sum(-1) + Q_RHO * math.log(R_RHO) - gammaln(Q_RHO)
            + gammaln(a) - a * np.log(R_RHO + h * (1.0 / sig).sum(-1)))


def rho_integrand(rho, sig):
    """prod_c InvGamma(sigma^2_c; k/2, k rho/2) * Gamma(rho; q, rate r): what log_prior_sigmasq integrates over rho."""
    sig = np.asarray(sig, np.float64)
    h = K_SIG / 2.0
    lp = (h * math.log(h * rho) - gammaln(h) - (h + 1.0) * np.log(sig) - h * rho / sig).sum()
    lp += Q_RHO * math.log(R_RHO) - gammaln(Q_RHO) + (Q_RHO - 1.0) * math.log(rho) - R_RHO * rho
    return math.exp(lp)


def eta_marginal(eta, d, s, grid=DEFAULT_GRID):
    """p(eta) = int N(eta; 0, lambda) InvGamma(lambda; d, s) d lambda on the grid's lambda axis."""
    u, lw = grid.axis("lam", 1)
    lam = np.exp(u)
    return float(np.exp(logsumexp(lw + u + log_prior_lambda(lam, d, s) - 0.5 * (LOG2PI + u) - 0.5 * eta * eta / lam)))


class _Model:
    def __init__(self, y, e, M, P, classes, d, s, fixalpha, grid):
        self.y = np.asarray(y, np.float64).ravel()
        self.e2 = np.asarray(e, np.float64).ravel() ** 2
        N = self.N = self.y.size
        self.cl = np.asarray(classes, np.int64).ravel()
        if self.e2.size != N or self.cl.size != N:
            raise ValueError("y, e and classes must have one entry per sample")
        self.nc = int(self.cl.max()) + 1
        self.d, self.s, self.grid = float(d), float(s), grid
        v_beta = 25.0 if fixalpha else 4.0
        cols, v = [], []
        self.has_alpha = not fixalpha
        if self.has_alpha:
            cols.append(np.ones(N))
            v.append(V_ALPHA)
        self.K = 0
        if not is_nil(M):
            M = np.asarray(M, np.float64)
            self.K = M.shape[1]
            cols += [M[:, j] for j in range(self.K)]
            v += [v_beta] * self.K
        self.Xf = np.stack(cols, 1) if cols else np.zeros((N, 0))       # the columns with a fixed prior variance
        self.vf = np.array(v)
        self.P = np.zeros((N, 0)) if is_nil(P) else np.asarray(P, np.float64)
        self.L = self.P.shape[1]
        self.dims = self.L + self.nc
        if self.dims > MAX_DIMS:
            raise ValueError("%d eta columns and %d variance classes need a grid of %d dimensions; at most %d are supported"
                             % (self.L, self.nc, self.dims, MAX_DIMS))
        if grid.pin is None:
            ax = [grid.axis("lam", self.dims)] * self.L + [grid.axis("sig", self.dims)] * self.nc
        else:
            ax = [(np.array([math.log(grid.pin[0])]), np.zeros(1))] * self.L + [(np.array([math.log(grid.pin[1])]), np.zeros(1))] * self.nc
        self.ax = ax
        self.shape = tuple(a[0].size for a in ax)
        self.size = int(np.prod(self.shape))

    def chunk(self, lo, hi):
        """lambda (B, L), sigma^2 (B, nc) and the log of weight * Jacobian * prior of grid points lo .. hi - 1."""
        idx = np.unravel_index(np.arange(lo, hi), self.shape)
        logv = np.stack([self.ax[a][0][idx[a]] for a in range(self.dims)], 1)
        lw = sum(self.ax[a][1][idx[a]] for a in range(self.dims))
        lam, sig = np.exp(logv[:, :self.L]), np.exp(logv[:, self.L:])
        if self.grid.pin is None:
            lw = lw + logv.sum(1)
        lw = lw + log_prior_sigmasq(sig)
        if self.L:
            lw = lw + log_prior_lambda(lam, self.d, self.s).sum(1)
        return lam, sig, lw

    def batch(self):
        return max(1000, int(3e6 / (self.N * 4)))

    def log_terms(self):
        """log of every grid point's contribution to the marginal likelihood, in batches.  log N(y; 0, D + X V0 X'), D the diagonal
        e^2 + sigma^2, through the determinant lemma and the Woodbury identity on A = V0^-1 + X' D^-1 X (p x p, p the number of coefficients, 5 at the most in the designs tested):
        log det = sum log D + sum log V0 + log det A, y' Sigma^-1 y = y' D^-1 y - t' A^-1 t with t = X' D^-1 y.  The N x N covariance
        itself has a condition number of 1e17 at lambda = e^30 and loses its sign to rounding at e^35; the p x p form stays exact
        there.  test_gaussian_only_model holds it to scipy's density of the N x N covariance."""
        out = np.empty(self.size)
        N = self.N
        X = np.concatenate([self.Xf, self.P], 1)
        p = X.shape[1]
        for lo in range(0, self.size, self.batch()):
            hi = min(lo + self.batch(), self.size)
            lam, sig, lw = self.chunk(lo, hi)
            w = 1.0 / (self.e2 + sig[:, self.cl])                         # (B, N)
            logdet = -np.log(w).sum(1)
            quad = (w * self.y * self.y).sum(1)
            if p:
                v0 = np.concatenate([np.broadcast_to(self.vf, (hi - lo, self.vf.size)), lam], 1)
                A = np.einsum("ia,bi,ic->bac", X, w, X)
                A[:, np.arange(p), np.arange(p)] += 1.0 / v0
                t = np.einsum("ia,bi,i->ba", X, w, self.y)
                sign, ld = np.linalg.slogdet(A)
                if not np.all(sign > 0):
                    raise FloatingPointError("precision matrix not positive definite on the grid")
                logdet = logdet + np.log(v0).sum(1) + ld
                quad = quad - (t * np.linalg.solve(A, t[:, :, None])[:, :, 0]).sum(1)
            out[lo:hi] = lw - 0.5 * (N * LOG2PI + logdet + quad)
        return out

    def cond_means(self, lo, hi):
        """E[alpha, beta, eta | y, lambda, sigma^2] = (X'WX + V0^-1)^-1 X'W y at grid points lo .. hi - 1: (B, p)."""
        lam, sig, _ = self.chunk(lo, hi)
        X = np.concatenate([self.Xf, self.P], 1)
        w = 1.0 / (self.e2 + sig[:, self.cl])                             # (B, N)
        A = np.einsum("ia,bi,ic->bac", X, w, X)
        prec = np.concatenate([np.broadcast_to(1.0 / self.vf, (hi - lo, self.vf.size)), 1.0 / lam], 1)
        p = X.shape[1]
        A[:, np.arange(p), np.arange(p)] += prec
        t = np.einsum("ia,bi,i->ba", X, w, self.y)
        return np.linalg.solve(A, t[:, :, None])[:, :, 0]


def log_marginal(y, e, M, P, classes, d=1.4, s=2.0, fixalpha=False, grid=DEFAULT_GRID):
    """log m of one model for one feature.  y, e (N,); M (N, K) or None; P (N, L) or None; classes (N,) this model's variance class
    of each sample."""
    return float(logsumexp(_Model(y, e, M, P, classes, d, s, fixalpha, grid).log_terms()))


def log_bf(y, e, M, P0, P1, classes, d=1.4, s=2.0, fixalpha=False, grid=DEFAULT_GRID):
    """log m1 - log m0; classes (N, 2), column j the classes under model j."""
    classes = np.asarray(classes)
    return (log_marginal(y, e, M, P1, classes[:, 1], d, s, fixalpha, grid)
            - log_marginal(y, e, M, P0, classes[:, 0], d, s, fixalpha, grid))


def posterior_mean(y, e, M, P, classes, d=1.4, s=2.0, fixalpha=False, grid=DEFAULT_GRID):
    """E[alpha | y, model], E[beta | y, model] (K,), E[eta | y, model] (L,): the conditional Gaussian mean weighted by the grid's
    posterior weights.  alpha is None with fixalpha; beta and eta are empty when M or P is nil.  The same pass gives the log marginal
    likelihood, returned as "log_marginal"."""
    m = _Model(y, e, M, P, classes, d, s, fixalpha, grid)
    p = m.Xf.shape[1] + m.L
    lt = m.log_terms()
    lse = float(logsumexp(lt))
    acc = np.zeros(p)
    if p:
        w = np.exp(lt - lse)
        for lo in range(0, m.size, m.batch()):
            hi = min(lo + m.batch(), m.size)
            acc += w[lo:hi] @ m.cond_means(lo, hi)
    a = 1 if m.has_alpha else 0
    return dict(alpha=float(acc[0]) if m.has_alpha else None, beta=acc[a:a + m.K].copy(), eta=acc[a + m.K:].copy(), log_marginal=lse)
