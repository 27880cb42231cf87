"""The ranges of the sample launches over the sliced-ELL tile lists, restated in numpy and Python integers (no GPU): the cutter, the
price of a tile, the five lists, the choice of the kernel.  Spec: mmseq_amd/csrc/mmgibbs.hip (weighted_chunks, problem_build_sell).

A tile is priced from tests/ladder_problem.tile_table, with v = MMG_OPT_K1_RANGE_COST (unset: 6):
    an empty tile                0
    a register-path tile         v + ng                        (ng: the groups of its block)
    a far tile                   v + ng + (2 v + 11) * nf      (ng: the groups of its window hits, nf: the entries of its far list)
    a CSR-walked tile            24 v + 130
    v = 0, the constant model    0, 2, 2 + 4 nf, 48
In the main list a tile with multiplicities costs 0; once a problem has such tiles the main list is the list WITHOUT them and they
are a list of their own, priced in the constant model's units with their draws: 2 c + 2 min(largest k, 64).

Everything here holds under MMG_OPT_K1_RANGES = R (at most R ranges per list, cut by plain weighted_chunks): without it the number of
ranges follows the occupancy the runtime reports."""
import numpy as np

import ladder_problem as lp

K_SMALL = 64
DEFAULT_TILE_COST = 6
LISTS = ("main", "multiplicity", "pairs", "fours", "far_csr")


def weighted_chunks(cum, grid):
    """bound[0 .. grid]: bound c is the first t with cum[t] >= floor(total * c / grid); bound[0] = 0, bound[grid] = the entries."""
    cum = [int(x) for x in cum]
    nt, total, grid = len(cum) - 1, cum[-1], int(grid)
    bound, t = [0] * (grid + 1), 0
    for c in range(1, grid):
        target = total * c // grid
        while t < nt and cum[t] < target:
            t += 1
        bound[c] = t
    bound[grid] = nt
    return bound


def cumulate(cost):
    out = [0]
    for c in cost:
        out.append(out[-1] + int(c))
    return out


def constant_prices(t):
    """The constant model: what the choice of the kernel and the multiplicity list are priced in, and the ranges under v = 0."""
    return np.where(t["nnz"] == 0, 0, np.where(t["qual"], 2, np.where(t["far_tile"], 2 + 4 * np.maximum(t["far_nf"], 0), 48))).astype(np.int64)


def tile_prices(t, v=None):
    """Per tile, whatever its multiplicities.  v: MMG_OPT_K1_RANGE_COST (None or negative: unset)."""
    if v is not None and v == 0:
        return constant_prices(t)
    v = DEFAULT_TILE_COST if v is None or v < 0 else int(v)
    far_entry_cost, slow_tile_cost = 2 * v + 11, 24 * v + 130
    return np.where(t["nnz"] == 0, 0, np.where(t["qual"], v + t["blk_ng"],
                    np.where(t["far_tile"], v + t["blk_ng"] + far_entry_cost * np.maximum(t["far_nf"], 0), slow_tile_cost))).astype(np.int64)


def kernel_choice(t, want_lean=None):
    """(lean, fixed_walk).  lean: every tile with hits is on the register path and none has a row with k != 1 (want_lean = 0: never).
    fixed_walk: fewer than 5 groups per register-path tile -- the blocks of the far tiles and the words of their far lists (a quarter
    of a group each) count among the groups; on a lean problem that is: the groups number fewer than 5 times the blocks."""
    hits = t["nnz"] > 0
    lean = bool((t["qual"][hits] & ~t["hask"][hits]).all()) and want_lean != 0
    n_fast = int(t["qual"].sum())
    slots = 256 * int(t["blk_ng"][t["qual"] | t["far_tile"]].sum()) + 64 * int(t["far_nf"][t["far_tile"]].sum())
    return lean, n_fast > 0 and slots < 5 * 256 * n_fast


def lists(t, ranges, v=None):
    """The five lists under MMG_OPT_K1_RANGES = ranges: {name: dict(tiles: the tile of every entry, cost: per entry, bound)} or None for
    a list the problem does not have.  The main list of a problem whose every tile has multiplicities is one empty entry (tiles = [-1])."""
    nt = t["r0"].size
    ranges = int(ranges)
    assert ranges >= 1 and nt >= 1
    price, const = tile_prices(t, v), constant_prices(t)
    flag_k = t["hask"] & (t["nnz"] > 0)                                  # (an empty tile carries no flag but the empty one)
    any_k = bool(t["hask"].any())
    grid = max(1, min(nt, ranges))
    out = dict.fromkeys(LISTS)

    def cut(tiles, cost, n):
        cost = [int(c) for c in cost]
        return dict(tiles=np.asarray(tiles, np.int64), cost=cost, bound=weighted_chunks(cumulate(cost), n))

    if not any_k:
        out["main"] = cut(np.arange(nt), price, grid)
    else:
        l1, lk = np.flatnonzero(~flag_k), np.flatnonzero(flag_k)
        if l1.size:
            out["main"] = cut(l1, np.where(t["hask"][l1], 0, price[l1]), max(1, min(l1.size, grid)))
        else:
            out["main"] = cut([-1], [0], 1)
        out["multiplicity"] = cut(lk, 2 * const[lk] + 2 * np.minimum(t["kmax"][lk], K_SMALL), max(1, min(lk.size, ranges)))
    plain = (t["nnz"] > 0) & ~flag_k
    lf, lx = np.flatnonzero(plain & t["qual"]), np.flatnonzero(plain & ~t["qual"])
    if lf.size:
        out["pairs"] = cut(lf, price[lf], min(lf.size, ranges))
        out["fours"] = cut(lf, price[lf], min(lf.size, ranges))
    if lx.size:
        out["far_csr"] = cut(lx, price[lx], max(1, min(lx.size, ranges)))
    return out


def list_shape(entry):
    """(entries, ranges, entries of the longest range) as Problem.k1_lists() reports a list."""
    if entry is None:
        return (0, 0, 0)
    b = entry["bound"]
    return (len(entry["cost"]), len(b) - 1, max(b[c + 1] - b[c] for c in range(len(b) - 1)))


def main_ranges(t, ranges, v=None, want_lean=None):
    """What mmg_problem_k1_ranges and mmg_k1_info report about the main list."""
    main = lists(t, ranges, v)["main"]
    b, cost, tiles = main["bound"], main["cost"], main["tiles"]
    groups = [int(t["blk_ng"][e]) if e >= 0 else 0 for e in tiles]
    cum, grp = cumulate(cost), cumulate(groups)
    rc = [cum[b[c + 1]] - cum[b[c]] for c in range(len(b) - 1)]
    work = [c for c in range(len(rc)) if rc[c] > 0]                     # the ranges that hold work
    lean, fixed = kernel_choice(t, want_lean)
    return dict(bound=b, cum_cost=[cum[x] for x in b], cum_groups=[grp[x] for x in b], n_list=len(cost), list_cost=cum[-1],
                n_ranges=len(work), range_cost_max=max([rc[c] for c in work], default=0),
                range_cost_mean=(sum(rc[c] for c in work) / len(work) if work else 0.0),
                range_tiles_max=max([b[c + 1] - b[c] for c in work], default=0), lean=lean, fixed_walk=fixed,
                range_tile_cost=0 if v == 0 else (DEFAULT_TILE_COST if v is None or v < 0 else int(v)))


def total_k_hit(row_ptr, k):
    """What a sweep's counts sum to: the multiplicities of the rows that have a hit (an empty row draws nothing)."""
    L = np.diff(np.asarray(row_ptr).astype(np.int64))
    return int((L > 0).sum()) if k is None else int(np.asarray(k).astype(np.int64)[L > 0].sum())


def run_keys(row_ptr, col_sorted):
    """A row's (near, band) -- its layout key >> 18 (mmg_types.h; oracle.binding.row_keys computes the whole key and the tie hash):
    near when it has at most 255 hits and all lie below offset 240 of its smallest hit's band, the band of its smallest hit then,
    else one below the band of its (lower) median hit; far << 45 | band.  0 for an empty row.  col_sorted: every row's hits ascending."""
    rp = np.asarray(row_ptr).astype(np.int64)
    L = np.diff(rp)
    key = np.zeros(L.size, np.uint64)
    ne = L > 0
    if ne.any():
        col = np.asarray(col_sorted).astype(np.int64)
        starts = rp[:-1][ne]
        lo, hi = col[starts], col[starts + L[ne] - 1]
        band = lo >> 6
        near = (L[ne] <= 255) & (hi - (band << 6) < 240)
        mid = col[starts + (L[ne] - 1) // 2] >> 6
        band = np.where(near, band, np.maximum(mid, 1) - 1)
        key[ne] = ((~near).astype(np.uint64) << np.uint64(45)) | band.astype(np.uint64)
    return key


def internal_ids(tx_order, n):
    """(int_of_ext, ext_of_int): the device numbers transcripts by ascending (key, index)."""
    if tx_order is None:
        return None, None
    ext_of_int = np.lexsort((np.arange(n), np.asarray(tx_order, np.uint64)))
    int_of_ext = np.empty(n, np.int64)
    int_of_ext[ext_of_int] = np.arange(n)
    return int_of_ext, ext_of_int


def stored_table(orc, row_ptr, col_idx, k, n, row_id_base=0, keep_rows=False, tx_order=None):
    """((row_ptr, col_idx, k) as the library stores and downloads the problem -- the caller's transcript numbering --, its tile table).
    Holds while the library keeps the transcript order it was given (MMG_OPT_DERIVE_ORDER = 0): the tiles are cut in the device's
    numbering, ascending (tx_order key, index).  keep_rows: the rows stay as they are, their hits unsorted; a far row's home band is
    then that of its median hit by rank, and the runs of equal (near, band) count only while there are at most max(1024, m / 32)."""
    int_of_ext, ext_of_int = internal_ids(tx_order, n)
    ci = np.asarray(col_idx, np.uint32)
    if int_of_ext is not None:
        ci = int_of_ext[ci].astype(np.uint32)
    if keep_rows:
        rp, kk = np.asarray(row_ptr, np.uint64), (None if k is None else np.asarray(k, np.uint32))
        m = rp.size - 1
        assert m == 0 or int(np.diff(rp.astype(np.int64)).max()) <= 4096     # (longer rows: the median by position)
        max_seg = max(1024, m // 32)
    else:
        rp, ci, kk, _ = orc.canonical_layout(row_ptr, ci, k)
        m = rp.size - 1
        max_seg = min(m, 2 * (int(n) >> 6) + 4)
    t = lp.tile_table(rp, ci, kk, run_keys(rp, orc.sort_hits(rp, ci)), row_id_base, max_seg=max_seg)
    ext = ci if ext_of_int is None else ext_of_int[ci].astype(np.uint32)
    return (rp, ext, kk), t
