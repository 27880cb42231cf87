"""tests/ladder_problem.py builds what tests/test_gpu_stream_ranges.py says it runs: checked here, on the CPU, against the oracle's
canonical_layout and a restatement of the tile cut and the window rule (mmgibbs.hip: problem_build_sell) -- nobody can look at
a workgroup's tiles on the device.  And the oracle's row stream changes its key at row id 2^33, from the Philox block itself."""
import numpy as np
import pytest

import ladder_problem as lp

# one period's tiles in stored order at row_id_base 0: (rows, groups, starts on an odd row id, the window slides in front of it)
_BASE = [(1, 5, False, True), (63, 1, True, True), (64, 2, False, False), (17, 3, False, False), (5, 4, True, True),
         (5, 6, False, True), (6, 7, True, True), (4, 8, True, True), (3, 9, True, True), (3, 12, False, True)]
CENSUS = {
    "short": _BASE + [(3, 2, True, False), (2, 1, False, True), (2, 1, False, True)],
    "long": _BASE + [(3, 8, True, False)],
    "far": _BASE + [(3, 8, True, False)],
    "k": _BASE + [(3, 8, True, False), (64, 2, False, True), (20, 3, False, False), (12, 5, False, True), (2, 2, False, True)],
}
HASK = {"k": [11 + 1, 11 + 2]}          # the period's tiles that hold a row with k != 1


@pytest.fixture(scope="module", params=lp.VARIANTS)
def built(request, orc):
    v = request.param
    rp, ci, l, k, mu0 = lp.ladder(3, v, seed=5)
    stored, tiles = lp.stored_tiles(orc, rp, ci, k)
    return v, (rp, ci, l, k, mu0), stored, tiles


def test_a_period_holds_every_tile_shape_in_the_order_the_recipe_gives(built):
    v, (rp, ci, l, k, mu0), (s_rp, s_ci, s_k), t = built
    B = len(lp.period_bands(v))
    near = ~t["far"]
    band = t["call"] // 64
    assert t["fast"][near].all() and (t["ng"][near] * 4 - t["maxlen"][near] < 4).all()
    per = []
    for p in range(3):
        sel = np.flatnonzero(near & (band >= B * p) & (band < B * (p + 1)))
        per.append([(int(t["nrows"][i]), int(t["ng"][i]), bool(t["odd"][i]), bool(t["slid"][i])) for i in sel])
        assert [i - sel[0] for i in sel if t["hask"][i]] == HASK.get(v, [])
    assert per[0] == per[1] == per[2] == CENSUS[v]                       # (an even number of rows: every period cuts the same way)
    plain = [c for j, c in enumerate(CENSUS[v]) if j not in HASK.get(v, [])]
    P = len(plain)
    assert P == lp.period_tiles(v) and P % 2 == 1
    assert {1, 2, 3, 4, 5, 6, 7, 8, 9, 12} <= {c[1] for c in plain}       # register path 1 ... 8 groups, tails of 1 and 4 groups
    assert {64, 63, 17, 1} <= {c[0] for c in plain}
    assert any(c[2] for c in plain) and any(not c[2] for c in plain)      # ds_bpermute and DPP hand-out of the Philox words
    L = np.diff(s_rp.astype(np.int64))
    assert {32, 33, 48} <= set(L.tolist())
    # three tiles under one window; a slide in front of a single-tile band and in front of the tile behind it
    assert any(plain[j][3] and not plain[j + 1][3] and not plain[j + 2][3] for j in range(P - 2))
    assert any(plain[j][3] and plain[j + 1][3] and plain[j + 2][3] for j in range(P - 2))
    # the window kept over a band boundary: the tile of a8 lies in the band behind a7's and inside a7's window
    kept = [i for i in np.flatnonzero(near) if not t["slid"][i] and t["call"][i] // 64 != t["wbase"][i] // 64]
    assert len(kept) == 3 and all(t["call"][i] // 64 == t["wbase"][i] // 64 + 1 and t["cmax"][i] < t["wbase"][i] + 255 for i in kept)
    # every hit of a near row inside [64 b, 64 b + 240), its smallest in the band's first 64
    rid = np.repeat(np.arange(L.size), L)
    lo = np.minimum.reduceat(s_ci, s_rp[:-1].astype(np.int64))
    nr = np.repeat(np.arange(t["r0"].size), t["nrows"])                   # tile of a row
    off = s_ci.astype(np.int64) - (lo[rid] // 64) * 64
    assert (off[near[nr][rid]] < 240).all()


@pytest.mark.parametrize("base", [0, 1])
def test_an_odd_row_id_base_flips_the_parity_of_every_tile(orc, base):
    rp, ci, l, k, mu0 = lp.ladder(3, "short", seed=5)
    _, t0 = lp.stored_tiles(orc, rp, ci, k, 0)
    _, t = lp.stored_tiles(orc, rp, ci, k, base)
    assert t["odd"].any() and (~t["odd"]).any() and 64 in t["nrows"]
    if base:
        first = np.isin(t["r0"], t0["r0"])                                # the tiles that start where a base-0 tile starts: the runs' first
        assert first.sum() >= 3 * 11 and (t["odd"][first] != t0["odd"][np.isin(t0["r0"], t["r0"])]).all()


def test_padded_slots_fall_on_the_side_the_variant_names(built):
    """mmgibbs.hip: k1_fixed_walk = padded_slots < 5 * 256 * fast_tiles, padded_slots = 256 groups per register-path tile (+ a far
    tile's block and list, which only add)."""
    v, _, _, t = built
    near = ~t["far"]
    slots, n_fast = 256 * int(t["ng"][near].sum()), int(t["fast"].sum())
    assert n_fast == int(near.sum())
    if v == "short":
        assert slots < 5 * 256 * n_fast and slots == 3 * 61 * 256
    else:
        assert slots >= 5 * 256 * n_fast


def test_the_far_and_k_variants_hold_what_they_promise(built, orc):
    v, (rp, ci, l, k, mu0), (s_rp, s_ci, s_k), t = built
    B = len(lp.period_bands(v))
    L = np.diff(s_rp.astype(np.int64))
    if v == "far":
        ft = np.flatnonzero(t["far"])
        assert ft.size == (3 * B + 1) // 2 and set(t["nrows"][ft].tolist()) == {2, 3, 4, 5}          # a far tile per second band
        below = above = 0
        for i in ft:
            for r in range(t["r0"][i], t["r0"][i] + t["nrows"][i]):
                row = s_ci[int(s_rp[r]):int(s_rp[r + 1])].astype(np.int64)
                out = row[(row < t["wbase"][i]) | (row >= t["wbase"][i] + 255)]
                assert 1 <= out.size <= 2 and row.size - out.size >= 3
                below += int((out < t["wbase"][i]).sum()); above += int((out >= t["wbase"][i] + 255).sum())
        assert below >= 10 and above >= 10
    elif v == "k":
        assert s_k is not None and set(np.unique(k).tolist()) == {1, 2, 9, 64, 65, 300, 20000}
        assert 0.05 < (k != 1).mean() < 0.15
        assert s_rp.size - 1 == rp.size - 1 + 3 * (1 + 8 + 63 + 1)       # rows stored k times: k = 2 twice, 9 and 64 once a period
        chain = (L >= 2) & ~orc.draws_categoricals(s_k, np.maximum(L, 1))
        assert chain.sum() == 3 * 9 and set(s_k[chain].tolist()) == {64, 65, 300, 20000}
        assert t["hask"].sum() == 3 * 2 and (t["fast"][t["hask"]]).all()
    else:
        assert not t["far"].any() and not t["hask"].any() and s_k is None


def test_start_values_hold_the_degenerate_rows(built):
    v, (rp, ci, l, k, mu0), (s_rp, s_ci, s_k), t = built
    assert np.gcd(lp.MU_PERIOD, 64) == 1 and np.array_equal(mu0[:-lp.MU_PERIOD], mu0[lp.MU_PERIOD:])
    fin = mu0[np.isfinite(mu0) & (mu0 > 1e-200)]
    assert fin.max() / fin.min() >= 1e12 and (mu0 == 1e-300).any()
    L = np.diff(s_rp.astype(np.int64))
    w = mu0[s_ci]
    with np.errstate(invalid="ignore"):
        tot = np.add.reduceat(w, s_rp[:-1].astype(np.int64))
        top = np.maximum.reduceat(w, s_rp[:-1].astype(np.int64))
        bot = np.minimum.reduceat(w, s_rp[:-1].astype(np.int64))
    many = L >= 2
    assert (many & (top == 0.0)).any()                                     # every weight zero: uniform pick
    assert (many & np.isinf(bot)).any()                                    # every weight infinite
    assert (many & np.isinf(top) & np.isfinite(bot)).any()                 # one infinite weight among finite ones
    assert (many & (tot > 0) & (tot < 2.3e-308)).any()                     # a subnormal total
    assert (many & np.isfinite(tot) & (tot > 1e-3)).mean() > 0.5           # and most rows are ordinary
    live = lp.mu_live(mu0)
    assert np.isfinite(live).all() and (live > 0).all() and np.array_equal(live[(mu0 > 0) & np.isfinite(mu0)], mu0[(mu0 > 0) & np.isfinite(mu0)])


def _row_key(seed, chain, rid, pin=False):
    """mmg_math.h: stream2_key(seed, chain, TAG_ROW, row id >> 33)."""
    hi = 0 if pin else rid >> 33
    return ((seed & 0xffffffff) ^ (((seed >> 32) * 0x9E3779B1) & 0xffffffff) ^ ((chain * 0x85EBCA6B) & 0xffffffff) ^ (1 << 28) ^
            ((hi * 0xC2B2AE35) & 0xffffffff)) & 0xffffffff


@pytest.mark.parametrize("chain", [0, 4])
def test_the_oracle_row_stream_changes_its_key_at_row_id_2_to_the_33(orc, chain):
    """Rows of two hits of weight 1 take hit [x >= 2^31] of their Philox word x (mmseq_oracle.c: pick_index).  Rows 2^33 - 300 ... 2^33 +
    300: the oracle's counts are the ones of key (seed, chain, TAG_ROW, id >> 33) with counter (id >> 1 mod 2^32, iteration), word
    id & 1 -- and not the ones of a key that ignores id >> 33, which differ above 2^33 and only there.  Without this an oracle that
    dropped the term would agree with a kernel that did the same."""
    n, seed, it = 600, (7 << 32) | 99, 3
    base = (1 << 33) - n // 2
    p = orc.Problem(np.arange(0, 2 * n + 1, 2, dtype=np.uint64), np.arange(2 * n, dtype=np.uint32), np.ones(2 * n))
    got = orc.sample_counts(p, np.ones(2 * n), seed, chain, it, row_id_base=base)
    assert np.array_equal(got[0::2] + got[1::2], np.ones(n, np.int32))
    true, pinned = np.empty(n, np.int32), np.empty(n, np.int32)
    for i in range(n):
        rid = base + i
        for out, pin in ((true, False), (pinned, True)):
            w = orc.philox2x32([(rid >> 1) & 0xffffffff, it], _row_key(seed, chain, rid, pin))
            out[i] = 1 if int(w[rid & 1]) >= (1 << 31) else 0
    assert np.array_equal(got[1::2], true)
    assert np.array_equal(true[:n // 2], pinned[:n // 2]) and 100 < int((true[n // 2:] != pinned[n // 2:]).sum()) < 200
