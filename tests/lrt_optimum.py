"""An independent maximum of mmdiff -lrt's likelihood, for tests/test_mmdiff_lrt_ref.py and
tests/test_gpu_mmdiff_lrt.py: no scoring, no Cholesky of our own, numpy's log.

For one feature and one model the profile log likelihood  pl(s) = max_theta l(theta, s)  over the class variances s (1 or 2 of
them) is evaluated on a dense grid -- 0, then log-spaced from 1e-12 to 1e6 times the data's scale, per class -- with theta from
numpy's batched solve of the weighted normal equations; the best grid point is polished with scipy's bounded optimiser (L-BFGS-B,
s >= 0, the analytic gradient of the profile).  The grid also answers whether pl has a single local maximum.

FIXTURES are the designs and data both tests use, drawn from fixed seeds."""
import functools

import numpy as np
from scipy import ndimage, optimize

import mmdiff_lrt_ref as L
import mmdiff_ref as R

LOG2PI = float(np.log(2.0 * np.pi))
DECADES = (-12.0, 6.0)
MODE_EPS = 1e-12         # grid values closer than this (the rounding of a sum of N terms of size 10) count as equal


def profile(X, cls, y, esq, S):
    """pl at the rows of S (G, nc): (G,)."""
    v = esq[None, :] + S[:, cls]                       # (G, N)
    w = 1.0 / v
    if X.shape[1]:
        A = np.einsum("ij,gi,ik->gjk", X, w, X)
        b = np.einsum("ij,gi,i->gj", X, w, y)
        theta = np.linalg.solve(A, b[:, :, None])[:, :, 0]
        r = y[None, :] - theta @ X.T
    else:
        r = np.broadcast_to(y[None, :], v.shape)
    return -0.5 * np.sum(LOG2PI + np.log(v) + r * r / v, 1)


def profile_grad(X, cls, y, esq, s):
    """(pl, d pl / d s_c) at one point: by the envelope theorem the gradient is U_c = 1/2 sum_{i in c} (r_i^2 / v_i^2 - 1 / v_i)."""
    v = esq + s[cls]
    w = 1.0 / v
    if X.shape[1]:
        theta = np.linalg.solve((X.T * w) @ X, (X.T * w) @ y)
        r = y - X @ theta
    else:
        r = y
    g = 0.5 * (r * r * w * w - w)
    return -0.5 * np.sum(LOG2PI + np.log(v) + r * r * w), np.array([g[cls == c].sum() for c in range(len(s))])


def count_modes(pl):
    """Local maxima of a grid of values (8 neighbours in 2-D).  Points not below any neighbour by more than MODE_EPS are candidates;
    touching candidates form one plateau, and a plateau is a local maximum if no grid point next to it is higher than its top
    (so the flat start of a rising slope, where steps are below MODE_EPS, is not one)."""
    structure = np.ones((3,) * pl.ndim)
    cand = pl >= ndimage.maximum_filter(pl, size=3, mode="nearest") - MODE_EPS
    labels, n = ndimage.label(cand, structure=structure)
    modes = 0
    for k in range(1, n + 1):
        mask = labels == k
        ring = ndimage.binary_dilation(mask, structure=structure) & ~mask
        if not ring.any() or pl[ring].max() <= pl[mask].max():
            modes += 1
    return modes


def optimum(X, cls, y, e, per_decade=10, polish_tol=1e-13):
    """dict(loglik, sigmasq (nc,), modes): the grid-plus-polish maximum of one feature and model, and the number of local maxima of
    the profile on the grid.  per_decade: grid points per decade; polish_tol: L-BFGS-B's ftol (relative) and gtol."""
    X, cls, y = np.asarray(X, np.float64), np.asarray(cls), np.asarray(y, np.float64)
    esq = np.asarray(e, np.float64) ** 2
    nc = int(cls.max()) + 1
    assert nc in (1, 2), "the grid is 1-D or 2-D"
    scale = max(float(np.var(y)), float(esq.mean()))
    n = int(round((DECADES[1] - DECADES[0]) * per_decade)) + 1
    axis = np.concatenate([[0.0], scale * 10.0 ** np.linspace(DECADES[0], DECADES[1], n)])
    if nc == 1:
        S = axis[:, None]
        shape = (len(axis),)
    else:
        a, b = np.meshgrid(axis, axis, indexing="ij")
        S = np.stack([a.ravel(), b.ravel()], 1)
        shape = (len(axis), len(axis))
    pl = np.concatenate([profile(X, cls, y, esq, S[i:i + 65536]) for i in range(0, len(S), 65536)]).reshape(shape)
    modes = count_modes(pl)
    best = S[int(np.argmax(pl))]
    res = optimize.minimize(lambda s: tuple(-t for t in profile_grad(X, cls, y, esq, s)), best, jac=True, method="L-BFGS-B",
                            bounds=[(0.0, None)] * nc, options=dict(ftol=polish_tol, gtol=polish_tol, maxiter=1000))
    ll = max(float(pl.max()), -float(res.fun))
    sig = res.x if -float(res.fun) >= float(pl.max()) else best
    return dict(loglik=ll, sigmasq=np.asarray(sig, float), modes=int(modes))


# ----------------------------------------------------------------------------- fixtures
def _data(seed, F, P1, fixalpha, e_range):
    """F features: features 0 and 1 have identical replicates (at 0 under -fixalpha, where no model has a level), features 2 and 3 a
    spread of 100 e, feature 4 an effect between the groups of model 1; e uniform in e_range.  Under -fixalpha the data are
    centred, as the option expects: no feature level, the effect symmetric."""
    rng = np.random.default_rng(seed)
    N = P1.shape[0]
    group0 = P1[:, 0] > 0.0           # the first group of -de: P1 is 0.5 / -0.5, or the groups' indicator columns
    y = (0.0 if fixalpha else rng.normal(2.0, 1.0, (F, 1))) + rng.normal(0.0, 0.3, (F, N))
    y[4] += np.where(group0, 0.75, -0.75)
    e = rng.uniform(e_range[0], e_range[1], (F, N))
    y[0] = 0.0 if fixalpha else 1.75
    y[1] = 0.0 if fixalpha else -0.5
    e[2:4] = rng.uniform(0.05, 0.1, (2, N))
    y[2:4] = (0.0 if fixalpha else 1.0) + 100.0 * e[2:4] * rng.normal(0.0, 1.0, (2, N))
    return y, e


COV6 = np.array([[0.3], [1.1], [-0.4], [0.9], [0.0], [-1.2]])


def _fixture(name):
    if name == "de33":
        d, fix = R.de_design((3, 3)), False
    elif name == "de222":
        d, fix = R.de_design((2, 2, 2)), False
    elif name == "covariate":
        d, fix = R.de_design((3, 3)), False
        d = (COV6.copy(),) + tuple(d[1:])
    elif name == "fixalpha":
        d, fix = R.de_design((3, 3)), True
    elif name == "classes2":            # two variance classes in model 1 that are not its groups: 4 + 3 samples, -de 3 4
        d, fix = R.de_design((3, 4)), False
        d = d[:3] + (np.stack([np.zeros(7, np.int64), np.array([0, 0, 1, 1, 0, 1, 0])], 1),)
    else:
        raise KeyError(name)
    M, P0, P1, C = d
    y, e = _data(SEEDS[name], 8, P1, fix, E_RANGE)
    return dict(M=M, P0=P0, P1=P1, C=C, fixalpha=fix, y=y, e=e)


# (a draw whose profile has two local maxima on the grid is replaced by changing its seed here, never by masking a feature)
E_RANGE = (0.05, 0.5)
SEEDS = dict(de33=101, de222=102, covariate=103, fixalpha=201, classes2=200)
FIXTURES = tuple(sorted(SEEDS))
# the models the grid covers: up to two classes, a design of full column rank (-de 2 2 2 without -fixalpha has the intercept and
# three indicator columns in model 1: status 2, checked as such)
MODELS = {"de33": (0, 1), "de222": (0,), "covariate": (0, 1), "fixalpha": (0, 1), "classes2": (0, 1)}


@functools.lru_cache(maxsize=None)
def fixture(name):
    return _fixture(name)


@functools.lru_cache(maxsize=None)
def reference(name, fine=False):
    """{model: list over features of optimum(...)} for a fixture; fine: the grid step halved, the polish 100 times tighter."""
    fx = fixture(name)
    out = {}
    for m in MODELS[name]:
        X = L.design_matrix(fx["M"], fx["P1"] if m else fx["P0"], fx["fixalpha"])
        out[m] = [optimum(X, fx["C"][:, m], fx["y"][f], fx["e"][f], 20 if fine else 10, 1e-15 if fine else 1e-13)
                  for f in range(fx["y"].shape[0])]
    return out
