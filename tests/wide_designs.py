"""Named mmdiff designs (M, P0, P1, classes) beyond `-de`: several covariate columns, a fitted model 0 with its own variance
classes, and the sizes at the host's caps.  Fixed literal or seeded values, no device; tests/test_wide_designs.py checks ranks, what
is nil, the class labels and the slot counts, and tests/test_gpu_mmdiff_wide.py and the exact cases f, g, h of
tests/test_mmdiff_exact.py run them.

The twelve samples of the N = 12 designs are those of test_mmdiff_exact.ROWS12: condition 1 is samples 0-5, condition 2 samples
6-11.  Samples 3-5 are a second batch of condition 1 (condition 2 was run in the first batch only), so batch and condition are not
confounded and the design has three cells.  That is what lets the matrices file of the CLI state it: there a row of P belongs to a
variance class, so P1 with its three distinct rows needs the three cells as the classes of model 1 (`k3_batch`).  `batch` keeps the same
matrices with the condition's two classes in model 1; that handle is built through the library, which takes P per sample."""
import numpy as np

# column 0 starts with the covariate of test_gpu_mmdiff's "covariate" case (test_mmdiff_exact.M_COV)
M3 = np.array([[0.3, -0.6, 0.5],
               [1.1, 0.4, -0.9],
               [-0.4, 1.2, 0.2],
               [0.9, -1.0, 0.6],
               [0.0, 0.1, -1.3],
               [-1.2, 0.8, 0.4],
               [0.7, -0.3, 1.1],
               [-0.8, 0.9, -0.2],
               [0.2, -1.1, -0.6],
               [-0.5, 0.5, 0.0],
               [1.0, 0.0, 0.8],
               [-0.1, -0.7, -0.4]])
CONDITION = np.array([0] * 6 + [1] * 6)
BATCH = np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0])
CELL = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2])


def _contrast(labels):
    return np.where(np.asarray(labels) == 0, 0.5, -0.5)[:, None]


def _k(K):
    return M3[:, :K].copy(), np.ones((12, 1)), _contrast(CONDITION), np.stack([np.zeros(12, np.int64), CONDITION], 1)


def _batch(M, classes1):
    P0 = _contrast(BATCH)
    P1 = np.concatenate([_contrast(BATCH), _contrast(CONDITION)], 1)
    return M, P0, P1, np.stack([BATCH, classes1], 1).astype(np.int64)


def _caps():
    """N = 40, K = 8, L0 = L1 = 16, 16 classes in both models: every size the host accepts at its largest.  Model 0's classes are
    i mod 16 (three samples in classes 0-7, two in 8-15), model 1's (i // 2) mod 16 (four in classes 0-3, two in the others)."""
    rng = np.random.default_rng(4016)
    i = np.arange(40)
    M = np.round(rng.normal(0.0, 0.7, (40, 8)), 3)
    P0 = np.round(rng.normal(0.0, 0.5, (40, 16)), 3)
    P1 = np.round(rng.normal(0.0, 0.5, (40, 16)), 3)
    return M, P0, P1, np.stack([i % 16, (i // 2) % 16], 1).astype(np.int64)


def _two_groups(N, M):
    first = np.arange(N) < N // 2
    return M, np.ones((N, 1)), np.where(first, 0.5, -0.5)[:, None], np.stack([np.zeros(N, np.int64), (~first).astype(np.int64)], 1)


DESIGNS = {
    "k2": lambda: _k(2),
    "k3": lambda: _k(3),
    "batch": lambda: _batch(np.zeros((12, 1)), CONDITION),
    "k3_batch": lambda: _batch(M3.copy(), CELL),
    "caps": _caps,
    "n512": lambda: _two_groups(512, np.round(np.random.default_rng(512).normal(0.0, 1.0, (512, 1)), 3)),
    "n2": lambda: _two_groups(2, np.zeros((2, 1))),
}


def design(name):
    """(M (N, K), P0 (N, L0), P1 (N, L1), classes (N, 2)) of a named design; a fresh copy on every call."""
    return DESIGNS[name]()


def shape(name):
    """dict(N, K, L0, L1, nc0, nc1, Mnil, Pnil) of a design, from its matrices alone (the nil rule of src/bms.cpp:1154-1156)."""
    M, P0, P1, C = design(name)
    nil = lambda X: X.shape[1] == 1 and X.max() - X.min() < 0.00001
    return dict(N=M.shape[0], K=M.shape[1], L0=P0.shape[1], L1=P1.shape[1], nc0=int(C[:, 0].max()) + 1, nc1=int(C[:, 1].max()) + 1,
                Mnil=nil(M), Pnil=(nil(P0), nil(P1)))


def data(name, F, seed):
    """y, e (F, N) for a design: a feature level, noise, and for the first fifth of the features an effect of 1.5 on the samples
    whose class under model 1 is 0 -- some features then prefer either model, so gamma moves."""
    M, P0, P1, C = design(name)
    N = M.shape[0]
    rng = np.random.default_rng(seed)
    y = rng.normal(2.0, 1.0, (F, 1)) + rng.normal(0.0, 0.3, (F, N))
    y[:F // 5, C[:, 1] == 0] += 1.5
    e = rng.uniform(0.05, 0.5, (F, N))
    return y, e


def matrices_text(name):
    """The `-m` file of a design whose P matrices are functions of the model's class: blocks M, classes, P0, P1, separated by empty
    lines, a row of P per class."""
    M, P0, P1, C = design(name)
    blocks = ["".join(" ".join("%r" % float(v) for v in row) + "\n" for row in M), "".join("%d %d\n" % tuple(c) for c in C)]
    for m, P in enumerate((P0, P1)):
        rows = []
        for c in range(int(C[:, m].max()) + 1):
            mine = P[C[:, m] == c]
            assert np.all(mine == mine[0]), "P%d is not a function of the class" % m
            rows.append(" ".join("%r" % float(v) for v in mine[0]) + "\n")
        blocks.append("".join(rows))
    return "# %s\n" % name + "\n".join(blocks)
