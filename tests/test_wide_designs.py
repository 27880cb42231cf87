"""The designs of tests/wide_designs.py, without a device: they pass the CLI's collinearity checks, the matrices meant to be nil are
nil and no other, the class labels have no gaps, and the slot count of each is DESIGN.md section 10's formula written out."""
import numpy as np
import pytest

import mmdiff_poly_ref as PR
import mmdiff_ref as R
import wide_designs as W

#          N,  K, L0, L1, nc0, nc1, Mnil,  P0nil, P1nil
SHAPES = {
    "k2": (12, 2, 1, 1, 1, 2, False, True, False),
    "k3": (12, 3, 1, 1, 1, 2, False, True, False),
    "batch": (12, 1, 1, 2, 2, 2, True, False, False),
    "k3_batch": (12, 3, 1, 2, 2, 3, False, False, False),
    "caps": (40, 8, 16, 16, 16, 16, False, False, False),
    "n512": (512, 1, 1, 1, 1, 2, False, True, False),
    "n2": (2, 1, 1, 1, 1, 2, True, True, False),
}


def test_every_design_is_listed():
    assert sorted(SHAPES) == sorted(W.DESIGNS)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_and_what_is_nil(name):
    N, K, L0, L1, nc0, nc1, Mnil, P0nil, P1nil = SHAPES[name]
    M, P0, P1, C = W.design(name)
    assert M.shape == (N, K) and P0.shape == (N, L0) and P1.shape == (N, L1) and C.shape == (N, 2)
    assert (R.is_nil(M), R.is_nil(P0), R.is_nil(P1)) == (Mnil, P0nil, P1nil)
    assert W.shape(name) == dict(N=N, K=K, L0=L0, L1=L1, nc0=nc0, nc1=nc1, Mnil=Mnil, Pnil=(P0nil, P1nil))
    assert all(np.isfinite(X).all() for X in (M, P0, P1))
    again = W.design(name)
    assert all(np.array_equal(a, b) for a, b in zip((M, P0, P1, C), again))          # fixed values, fresh copies
    M[0, 0] += 1.0
    assert not np.array_equal(M, W.design(name)[0])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_class_labels_have_no_gaps(name):
    N, K, L0, L1, nc0, nc1 = SHAPES[name][:6]
    C = W.design(name)[3]
    for m, nc in enumerate((nc0, nc1)):
        assert sorted(set(C[:, m].tolist())) == list(range(nc))
    if name == "caps":
        assert min(np.bincount(C[:, m]).min() for m in range(2)) >= 2


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_collinearity_checks_pass(name):
    """check_design of host/mmdiff_main.cpp: [1 | M] (a nil M left out) and that with the model's P appended (a nil P left out) have
    full column rank, and so has P alone.  The caps design is the one with least room: 1 + 8 + 16 = 25 columns on 40 samples."""
    M, P0, P1, C = W.design(name)
    N = M.shape[0]
    Z = np.ones((N, 1)) if R.is_nil(M) else np.concatenate([np.ones((N, 1)), M], 1)
    assert np.linalg.matrix_rank(Z) == Z.shape[1]
    for P in (P0, P1):
        if R.is_nil(P):
            continue
        full = np.concatenate([Z, P], 1)
        assert np.linalg.matrix_rank(P) == P.shape[1]
        assert np.linalg.matrix_rank(full) == full.shape[1] <= N
        assert np.linalg.cond(full) < 1e3                     # far from collinear, not merely of full rank in floating point


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_slot_count_is_the_documented_formula(name):
    """2 (11 + 6 K) + 11 (L0 + L1) + 5 (classes) + 3 state slots, a workspace of 5 K^2 + 2 K slots when M is not nil, and
    2 max(classes) slots for the sigma^2 walk (Memory)."""
    N, K, L0, L1, nc0, nc1, Mnil = SHAPES[name][:7]
    want = 2 * (11 + 6 * K) + 11 * (L0 + L1) + 5 * (nc0 + nc1) + 3 + (0 if Mnil else 5 * K * K + 2 * K) + 2 * max(nc0, nc1)
    assert PR.nslot(K, L0, L1, nc0, nc1, Mnil) == want
    F = 130
    assert PR.single_device_bytes(F, N, K, L0, L1, nc0, nc1, Mnil) == 8 * (2 * F * N + F * want + N * (K + L0 + L1)) + 4 * (2 * N + 2 * F + 1)


def test_slot_counts_written_out():
    """The figures themselves, so that a change of the formula and of this file's copy of it together would still show."""
    got = {name: PR.nslot(*SHAPES[name][1:7]) for name in SHAPES}
    assert got == {"k2": 114, "k3": 153, "batch": 94, "k3_batch": 176, "caps": 1001, "n512": 85, "n2": 78}


def test_the_matrices_file_states_k3_batch():
    """The CLI's matrices file holds a row of P per variance class: k3_batch's P0 and P1 are functions of the model's classes (the
    three cells of batch x condition in model 1), `batch` has the same three rows of P1 on two classes and is built through the library."""
    text = W.matrices_text("k3_batch")
    blocks = [b.strip().split("\n") for b in text.split("\n\n")]
    assert [len(b) for b in blocks] == [13, 12, 2, 3]                     # the comment line and M; classes; P0; P1
    assert blocks[2] == ["0.5", "-0.5"] and blocks[3] == ["0.5 0.5", "-0.5 0.5", "0.5 -0.5"]
    with pytest.raises(AssertionError):
        W.matrices_text("batch")


def test_data_moves_gamma_both_ways():
    y, e = W.data("k3", 130, 5)
    assert y.shape == e.shape == (130, 12) and e.min() > 0
    C = W.design("k3")[3]
    lift = y[:, C[:, 1] == 0].mean(1) - y[:, C[:, 1] == 1].mean(1)
    assert lift[:26].min() > 0.9 and np.abs(lift[26:]).max() < 0.7
