"""The restatement of mmdiff's effect summaries (tests/mmdiff_effects_ref.py) on hand-made rows whose answers are known without it."""
import math

import numpy as np
import pytest

import mmdiff_effects_ref as E


def one_series(x, gamma=None, model=0):
    """rows (S, 2, 1): one parameter of `model` and gamma."""
    x = np.asarray(x, np.float64)
    g = np.full(x.size, float(model)) if gamma is None else np.asarray(gamma, np.float64)
    return np.stack([x, g], 1)[:, :, None]


@pytest.mark.parametrize("n,pct,want", [
    (1, (0, 2.5, 50, 97.5, 100), (0, 0, 0, 0, 0)),
    (2, (0, 49.9, 50, 100), (0, 0, 1, 1)),                      # 0.5 + 0.5 = 1: a half rounds up
    (3, (0, 24.9, 25, 50, 74.9, 75, 100), (0, 0, 1, 1, 1, 2, 2)),
    (5, (0, 2.5, 37.5, 50, 62.5, 97.5, 100), (0, 0, 2, 2, 3, 4, 4)),
    (1024, (2.5, 50, 97.5, 100), (26, 512, 997, 1023)),         # 25.575 + .5, 511.5 + .5, 997.425 + .5
])
def test_quantile_index_on_sorted_ramps(n, pct, want):
    ramp = np.arange(n, dtype=np.float64)
    for x in (ramp, ramp[::-1], np.random.default_rng(n).permutation(ramp)):
        out = E.effects(one_series(x), [0], pct)
        assert out["q"][0, :, 0].tolist() == [float(w) for w in want]
        assert [E.picked_index(p, n) for p in pct] == list(want)
        assert out["n"][:, 0].tolist() == [n, 0]


def test_all_ties():
    out = E.effects(one_series(np.full(37, 1.25)), [0], (0, 2.5, 50, 97.5, 100))
    assert np.all(out["q"] == 1.25) and out["mean"][0, 0] == 1.25 and out["sd"][0, 0] == 0.0 and out["n_gt"][0, 0] == 37


def test_neither_zero_counts_as_positive():
    x = [0.0, -0.0, 1e-300, -1e-300, 0.0, 5e-324, -0.0]
    out = E.effects(one_series(x), [0], (50,))
    assert out["n_gt"][0, 0] == 2 and out["n"][0, 0] == 7
    assert out["q"][0, 0, 0] == 0.0                              # index 3 of (-1e-300, four zeros, 5e-324, 1e-300)


def test_draws_are_the_rows_of_the_parameters_own_model():
    """Two parameters, of models 0 and 1, over the same rows: each keeps the rows whose gamma is its model, in row order."""
    g = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1], np.float64)
    a = np.arange(10, dtype=np.float64)
    b = -a
    rows = np.stack([a, b, g], 1)[:, :, None]
    out = E.effects(rows, [0, 1], (0, 50, 100))
    assert out["n"][:, 0].tolist() == [4, 6]
    assert out["mean"][:, 0].tolist() == [(0 + 3 + 5 + 6) / 4.0, -(1 + 2 + 4 + 7 + 8 + 9) / 6.0]
    assert out["q"][0, :, 0].tolist() == [0.0, 5.0, 6.0]         # floor(1.5 + .5) = 2 of (0, 3, 5, 6)
    assert out["q"][1, :, 0].tolist() == [-9.0, -4.0, -1.0]      # floor(2.5 + .5) = 3 of (-9, -8, -7, -4, -2, -1)
    assert out["n_gt"][:, 0].tolist() == [3, 0]
    assert out["sd"][0, 0] == math.sqrt(((0 - 3.5) ** 2 + (3 - 3.5) ** 2 + (5 - 3.5) ** 2 + (6 - 3.5) ** 2) / 3.0)


def test_no_draw_and_one_draw():
    x = [3.0, 4.0, 5.0]
    out = E.effects(np.stack([x, x, [1.0, 0.0, 1.0]], 1)[:, :, None], [0, 1], (2.5, 50))
    assert out["n"][:, 0].tolist() == [1, 2]
    assert out["mean"][0, 0] == 4.0 and np.isnan(out["sd"][0, 0]) and out["q"][0, :, 0].tolist() == [4.0, 4.0]
    none = E.effects(one_series(x, gamma=[1.0, 1.0, 1.0]), [0], (2.5, 50))
    assert none["n"][:, 0].tolist() == [0, 3] and none["n_gt"][0, 0] == 0
    assert np.isnan(none["mean"][0, 0]) and np.isnan(none["sd"][0, 0]) and np.all(np.isnan(none["q"]))


def test_sums_run_in_row_order():
    """1e16 + 1 + 1 - 1e16 is 0 from left to right (each 1 is lost) and 2 exactly; pairwise it is 0 or 2 depending on the split."""
    out = E.effects(one_series([1e16, 1.0, 1.0, -1e16]), [0], ())
    assert out["mean"][0, 0] == 0.0
    big = np.concatenate([[1e16], np.ones(4094), [-1e16]])
    assert E.effects(one_series(big), [0], ())["mean"][0, 0] == 0.0 and math.fsum(big) == 4094.0
    # the second pass: deviations from the rounded mean, squared and rounded, added from the left
    x = np.array([0.1, 0.2, 0.4, 0.8, 1.6])
    m = ((((0.1 + 0.2) + 0.4) + 0.8) + 1.6) / 5.0
    ss = 0.0
    for v in x:
        ss += (v - m) * (v - m)
    got = E.effects(one_series(x), [0], ())
    assert got["mean"][0, 0] == m and got["sd"][0, 0] == math.sqrt(ss / 4.0)


def test_refusals():
    ok = one_series([1.0, 2.0])
    for bad in ((-0.1,), (100.1,), (float("nan"),), tuple(range(33))):
        with pytest.raises(ValueError):
            E.effects(ok, [0], bad)
    with pytest.raises(ValueError):
        E.effects(one_series([1.0, 2.0], gamma=[0.0, 0.5]), [0], (50,))
    with pytest.raises(ValueError):
        E.effects(ok, [2], (50,))
    with pytest.raises(ValueError):
        E.effects(np.zeros((4097, 2, 1)), [0], (50,))
    with pytest.raises(ValueError):
        E.effects(np.zeros((3, 1, 1)), [], (50,))


def test_models_from_names():
    import mmdiff_trace_ref as TR
    names = TR.param_names(1, (1, 2), (1, 2))
    assert names[:-1] == ["alpha0", "alpha1", "beta0_0", "beta1_0", "eta0_0", "eta1_0", "eta1_1", "lambda0_0", "lambda1_0", "lambda1_1",
                          "sigmasq0_0", "sigmasq1_0", "sigmasq1_1", "rho0", "rho1"]
    assert E.model_of_names(names[:-1]).tolist() == [0, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1]
