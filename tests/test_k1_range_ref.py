"""CPU checks of tests/k1_range_ref.py and of the far-tile columns of ladder_problem.tile_table: the restatement the GPU tests of the
ranges compare the library with must itself be what it says."""
import numpy as np
import pytest

import k1_range_ref as ref
import ladder_problem as lp


def _costs(rng, n, kind):
    if kind == "flat":
        return np.full(n, 7)
    if kind == "zeros":                                                # runs of entries that cost nothing (empty and multiplicity tiles)
        return np.where(rng.random(n) < 0.6, 0, rng.integers(1, 20, n))
    if kind == "dear":                                                 # one entry above total / grid
        c = rng.integers(5, 12, n)
        c[rng.integers(0, n)] = 930
        return c
    return rng.integers(0, 50, n)


@pytest.mark.parametrize("kind", ["flat", "zeros", "dear", "mixed"])
def test_cutter_covers_is_monotone_and_misses_a_share_by_less_than_an_entry(kind):
    """bound c is the first t with cum[t] >= floor(total c / grid), so cum[bound c] <= floor(total c / grid) + dearest - 1 and
    cum[bound c] >= floor(total c / grid): a range costs less than total / grid + the dearest entry.  A property of the cutter."""
    rng = np.random.default_rng(3)
    for n in (1, 2, 17, 64, 500):
        for grid in (1, 2, 3, 16, 40, n, n + 5):
            cost = _costs(rng, n, kind)
            cum = ref.cumulate(cost)
            b = ref.weighted_chunks(cum, grid)
            assert len(b) == grid + 1 and b[0] == 0 and b[-1] == n
            assert all(b[c] <= b[c + 1] for c in range(grid))
            total, dearest = cum[-1], int(cost.max())
            for c in range(grid):
                rc = cum[b[c + 1]] - cum[b[c]]
                assert total == 0 or rc * grid < total + dearest * grid, (n, grid, c, rc)
            for c in range(1, grid):                                   # the definition itself
                target = total * c // grid
                assert cum[b[c]] >= target or b[c] == n
                assert b[c] == 0 or cum[b[c] - 1] < target


def test_cutter_leaves_interior_ranges_empty_beside_a_dear_entry():
    cum = ref.cumulate([7] * 23 + [697])
    b = ref.weighted_chunks(cum, 16)
    assert b == [0, 8, 16, 23] + [24] * 13


def _table(**cols):
    n = len(next(iter(cols.values())))
    t = dict(nnz=np.ones(n, np.int64), qual=np.zeros(n, bool), far_tile=np.zeros(n, bool), far_nf=np.full(n, -1), blk_ng=np.zeros(n, np.int64),
             hask=np.zeros(n, bool), kmax=np.ones(n, np.int64), slow=np.zeros(n, bool), r0=np.arange(n) * 64)
    t.update({k: np.asarray(v) for k, v in cols.items()})
    return t


def test_prices():
    #            empty  register path  far (40 entries)  CSR-walked
    t = _table(nnz=[0, 64, 64, 64], qual=[False, True, False, False], far_tile=[False, False, True, False], far_nf=[-1, -1, 40, -1],
               blk_ng=[0, 5, 2, 0], slow=[False, False, False, True])
    assert ref.tile_prices(t).tolist() == [0, 6 + 5, 6 + 2 + 23 * 40, 24 * 6 + 130]
    assert ref.tile_prices(t, -1).tolist() == ref.tile_prices(t).tolist()
    assert ref.tile_prices(t, 1).tolist() == [0, 1 + 5, 1 + 2 + 13 * 40, 154]
    assert ref.tile_prices(t, 12).tolist() == [0, 12 + 5, 12 + 2 + 35 * 40, 418]
    assert ref.tile_prices(t, 0).tolist() == ref.constant_prices(t).tolist() == [0, 2, 2 + 4 * 40, 48]


def test_multiplicity_tiles_cost_nothing_in_the_main_list_and_leave_it():
    t = _table(qual=[True] * 6, blk_ng=[3] * 6, hask=[False, True, False, True, True, False], kmax=[1, 9, 1, 300, 2, 1])
    ls = ref.lists(t, 2)
    assert ls["main"]["tiles"].tolist() == [0, 2, 5] and ls["main"]["cost"] == [9, 9, 9]
    assert ls["multiplicity"]["tiles"].tolist() == [1, 3, 4] and ls["multiplicity"]["cost"] == [4 + 18, 4 + 128, 4 + 4]
    assert ls["pairs"]["tiles"].tolist() == [0, 2, 5] and ls["far_csr"] is None
    w = ref.main_ranges(t, 2)
    assert w["n_list"] == 3 and w["bound"][-1] == 3 and not w["lean"]
    every = _table(qual=[True] * 3, blk_ng=[3] * 3, hask=[True] * 3, kmax=[5] * 3)
    w = ref.main_ranges(every, 4)
    assert (w["bound"], w["cum_cost"], w["n_list"], w["n_ranges"], w["range_cost_mean"]) == ([0, 1], [0, 0], 1, 0, 0.0)
    assert ref.list_shape(ref.lists(every, 4)["multiplicity"]) == (3, 3, 1)


def test_kernel_choice():
    lean = _table(nnz=[0, 64, 64], qual=[False, True, True], blk_ng=[0, 4, 5])
    assert ref.kernel_choice(lean) == (True, True) and ref.kernel_choice(lean, 0) == (False, True) and ref.kernel_choice(lean, 1) == (True, True)
    assert ref.kernel_choice(_table(qual=[True, True], blk_ng=[5, 5])) == (True, False)               # 5 groups per block: the generic walk
    assert ref.kernel_choice(_table(qual=[True, True], blk_ng=[4, 4], hask=[False, True]))[0] is False
    far = _table(qual=[True, False], far_tile=[False, True], far_nf=[-1, 3], blk_ng=[4, 1])
    assert ref.kernel_choice(far) == (False, False)                                                  # 4 + 1 + 3 / 4 groups on one register-path tile
    assert ref.kernel_choice(_table(qual=[True, False], slow=[False, True], blk_ng=[4, 0])) == (False, True)


def _far_rows():
    """Three rows of home band 10 (window 640 ... 894): four window hits, 15 hits below, 15 above; and 40 near rows of band 2."""
    rng = np.random.default_rng(1)
    cols = [np.concatenate([[128 + int(rng.integers(0, 20))], np.sort(rng.choice(np.arange(150, 300), 2, replace=False))]) for _ in range(40)]
    for j in range(3):
        cols.append(np.concatenate([np.sort(rng.choice(576, 15, replace=False)), [650 + j, 710, 720, 730], np.sort(rng.choice(np.arange(900, 1900), 15, replace=False))]))
    rp = np.zeros(len(cols) + 1, np.uint64)
    rp[1:] = np.cumsum([c.size for c in cols])
    return rp, np.concatenate(cols).astype(np.uint32)


def test_far_tile_columns_of_the_tile_table(orc):
    rp, ci = _far_rows()
    (srp, sci, sk), t = ref.stored_table(orc, rp, ci, None, 1904)
    assert t["qual"].tolist() == [True, False] and t["far_tile"].tolist() == [False, True] and t["far"].tolist() == [False, True]
    assert (int(t["far_wbase"][1]), int(t["far_nn"][1]), int(t["far_nf"][1]), int(t["blk_ng"][1])) == (640, 4, 30, 1)
    assert (sci[int(srp[40]):int(srp[40]) + 4] >= 640).all() and (sci[int(srp[40]):int(srp[40]) + 4] < 895).all()      # stored window-hits-first
    # the same rows kept as given: ascending hits, so a window hit follows hits below the window -- no far tile, walked from the CSR
    _, tk = ref.stored_table(orc, rp, ci, None, 1904, keep_rows=True)
    assert tk["qual"].tolist() == [True, False] and tk["far_tile"].tolist() == [False, False] and tk["slow"].tolist() == [False, True]
    assert int(tk["far_nf"][1]) == -1 and int(tk["blk_ng"][1]) == 0
    # empty rows join the run around them; a tile of nothing else is empty
    rp2 = np.concatenate([np.zeros(70, np.uint64), rp])
    _, te = ref.stored_table(orc, rp2, ci, None, 1904)
    assert te["nnz"].tolist()[0] == 0 and te["nrows"].tolist() == [64, 46, 3] and te["qual"].tolist() == [False, True, False]
    assert ref.tile_prices(te).tolist() == [0, 6 + 1, 6 + 1 + 23 * 30]
    # device numbering by tx_order: reversing the transcripts mirrors the rows
    (xrp, xci, _), tx = ref.stored_table(orc, rp, ci, None, 1904, tx_order=np.arange(1904, 0, -1).astype(np.uint64))
    assert np.array_equal(np.sort(xci), np.sort(ci)) and tx["r0"].size >= 2


def test_run_keys_are_the_oracles(orc):
    q, _ = orc.synth_problem(R=3000, T=3000, avg_hits=8, seed=7, sort=False, far_fraction=0.3)
    rp = np.insert(q.row_ptr, [5, 5, 900], q.row_ptr[[5, 5, 900]])    # three empty rows
    col = orc.sort_hits(rp, q.col_idx)
    key = ref.run_keys(rp, col)
    assert np.array_equal(key, orc.row_keys(rp, col)[0] >> np.uint64(18)) and (key >> np.uint64(45)).sum() > 300 and (key == 0).sum() >= 3


@pytest.mark.parametrize("variant", lp.VARIANTS)
def test_on_the_ladder_the_new_columns_agree_with_the_old(orc, variant):
    rp, ci, l, k, _ = lp.ladder(3, variant, seed=11)
    _, t = lp.stored_tiles(orc, rp, ci, k)
    assert np.array_equal(t["qual"], t["fast"]) and np.array_equal(t["far_tile"], t["far"]) and not t["slow"].any()
    assert np.array_equal(t["far_wbase"][t["far"]], t["wbase"][t["far"]])
    if variant == "far":
        assert t["far"].sum() >= 3 and set(t["far_nf"][t["far"]].tolist()) <= {1, 2} and (t["far_nn"][t["far"]] >= 3).all()
    lean, fixed = ref.kernel_choice(t)
    assert lean == (variant in ("short", "long")) and fixed == (variant == "short")
