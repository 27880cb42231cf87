"""Problems whose sliced-ELL tile sequence is known in advance (plain numpy, no GPU): the input of tests/test_gpu_stream_ranges.py.

The library stores rows by (near / far, band of the smallest hit, multiplicity class, length, tie) and cuts every run of equal
(near, band) into tiles of 64 rows -- 63 where the tile starts on an odd row id (mmgibbs.hip: problem_build_sell).  So the rows a
band is given fix its tiles.  A PERIOD is a run of consecutive bands, each with a recipe of (row length, count); a problem is the
period repeated.  The period's register-path tiles without multiplicities, in stored order, number P (odd) and hold every shape
the stream kernels branch on: a workgroup whose range is 2 P tiles or longer walks each of them as tile A and as tile B of its
unrolled pair, wherever the range was cut.

    band  rows (length x count)                  tiles (rows, groups)            what it is there for
    a0    18 x 1                                 (1, 5)                          one row; leaves the next run on an odd row id
    a1    1..4 x 63, 5..8 x 64, 9..12 x 17       (63, 1) (64, 2) (17, 3)         three tiles in one window; odd start
    a2    13..16 x 5                             (5, 4)                          single-tile bands: a slide in front of each
    a3    21..24 x 5                             (5, 6)
    a4    25..28 x 6                             (6, 7)
    a5    29..32 x 4                             (4, 8)                          32 hits: the last length the register cache holds
    a6    33 x 3                                 (3, 9)                          tail groups from the stream
    a7    45..48 x 3                             (3, 12)
    a8    every hit below offset 191             (3, 8) or (3, 2)                fits a7's window: the window stays in force
    e0 e1 ("short" only) 2 rows each             (2, 1) (2, 1)                   weight towards few groups

Every other row of two hits or more has its last hit at offset 191 ... 239 of its band, which no earlier band's window covers: its
tile slides.  A period has an even number of stored rows, so every period starts on an even row id and cuts the same way.

Variants: "short" (a8 of 2 groups, e0, e1: 61 groups in 13 tiles, below the 5 per tile of k1_fixed_walk), "long" (a8 of 8 groups:
65 groups in 11 tiles, above it), "far" ("long" + 2 ... 5 far rows in every second band, far hits below and above the window),
"k" ("long" + three bands k0, k1, kx whose rows carry k from {2, 9, 64, 65, 300, 20000}: rows stored k times, tiles with
multiplicities, rows on the binomial chain).
"""
import numpy as np

BAND, NEAR_SPAN, WIN = 64, 240, 255
KEEP_BELOW = 191                       # 255 - 64: what the window of the band in front still covers
MU_PERIOD = 251                        # prime: coprime to the band width
ZERO_RUN, INF_RUN, SUB_RUN = (70, 3), (80, 2), (90, 3)     # (first residue, length) of the runs of 0, +inf and subnormal values
N_TEMPLATES = 8

_A1 = [(1, 15), (2, 16), (3, 16), (4, 16), (5, 16), (6, 16), (7, 16), (8, 16), (9, 5), (10, 4), (11, 4), (12, 4)]
_BASE = [
    dict(rows=[(18, 1)]),
    dict(rows=_A1),
    dict(rows=[(13, 2), (15, 2), (16, 1)]),
    dict(rows=[(21, 2), (23, 2), (24, 1)]),
    dict(rows=[(25, 3), (27, 2), (28, 1)]),
    dict(rows=[(29, 2), (31, 1), (32, 1)]),
    dict(rows=[(33, 3)]),
    dict(rows=[(45, 1), (48, 2)]),
]
_KEPT_LONG = dict(rows=[(30, 1), (31, 2)], kept=True)
_KEPT_SHORT = dict(rows=[(5, 1), (6, 2)], kept=True)
_EXTRA_SHORT = [dict(rows=[(2, 1), (3, 1)]), dict(rows=[(1, 1), (4, 1)])]
# (length, count, k): k0 stores 4 + 2 + 9 + 64 rows with k = 1 (a 64-row tile without multiplicities, then a tile with the 5 rows on
# the binomial chain); k1 is one tile with multiplicities; kx one tile without.  98 stored rows in all: even.
_K_BANDS = [
    dict(rows=[(3, 2, 1), (7, 2, 1), (3, 1, 2), (4, 1, 9), (6, 1, 64), (3, 1, 64), (8, 1, 65), (2, 1, 300), (12, 1, 20000), (1, 1, 9)]),
    dict(rows=[(2, 3, 1), (5, 2, 1), (2, 1, 2), (2, 1, 65), (5, 1, 300), (3, 1, 20000), (20, 1, 20000), (4, 1, 64)]),
    dict(rows=[(2, 1, 1), (6, 1, 1)]),
]

VARIANTS = ("short", "long", "far", "k")


def period_bands(variant):
    """The band recipes of one period."""
    if variant == "short":
        return _BASE + [_KEPT_SHORT] + _EXTRA_SHORT
    if variant in ("long", "far"):
        return _BASE + [_KEPT_LONG]
    if variant == "k":
        return _BASE + [_KEPT_LONG] + _K_BANDS
    raise ValueError(variant)


def period_tiles(variant):
    """P: the register-path tiles without multiplicities of one period -- the list the pair kernels walk (odd)."""
    return {"short": 13, "long": 11, "far": 11, "k": 13}[variant]


def periods_for(variant, min_tiles):
    return -(-int(min_tiles) // period_tiles(variant))


def _row(rng, L, kept):
    first = int(rng.integers(0, BAND))
    if L == 1:
        return [first]
    if kept:
        rest = rng.choice(np.arange(first + 1, KEEP_BELOW), size=L - 1, replace=False)
        return [first] + sorted(rest.tolist())
    last = int(rng.integers(KEEP_BELOW, NEAR_SPAN))
    mid = rng.choice(np.arange(first + 1, last), size=L - 2, replace=False)
    return [first] + sorted(mid.tolist()) + [last]


def _template(bands, rng):
    """One period's rows relative to its first transcript: (lengths, hits, k, the offsets in `hits` of the rows of a1 that a run of
    special start values may replace: one of 2 hits, two of 3)."""
    lens, hits, ks, spare = [], [], [], {2: [], 3: []}
    pos = 0
    for b, band in enumerate(bands):
        for spec in band["rows"]:
            L, count = spec[0], spec[1]
            k = spec[2] if len(spec) > 2 else 1
            for _ in range(count):
                r = _row(rng, L, band.get("kept", False))
                if b == 1 and k == 1 and L in spare and len(spare[L]) < 2:
                    spare[L].append(pos)
                lens.append(L); ks.append(k)
                hits.extend(BAND * b + h for h in r)
                pos += L
    return np.asarray(lens, np.int64), np.asarray(hits, np.int64), np.asarray(ks, np.uint32), spare


def mu_pattern(T):
    """Start values periodic in the transcript index (period 251): 1e-6 ... 1e6, entries of 1e-300, a run of zeros, a run of +inf, a
    run of subnormal values."""
    r = np.arange(MU_PERIOD)
    v = 10.0 ** (-6.0 + 12.0 * ((r * 37) % MU_PERIOD) / (MU_PERIOD - 1.0))
    v[[30, 31, 32, 100, 170, 171]] = 1e-300
    v[ZERO_RUN[0]:ZERO_RUN[0] + ZERO_RUN[1]] = 0.0
    v[INF_RUN[0]:INF_RUN[0] + INF_RUN[1]] = np.inf
    v[SUB_RUN[0]:SUB_RUN[0] + SUB_RUN[1]] = [5e-324, 1e-310, 3e-320]
    return v[np.arange(T) % MU_PERIOD]


def mu_live(mu0):
    """The pattern with its zeros and infinities replaced (an EM start value is positive and finite)."""
    mu = np.array(mu0, np.float64, copy=True)
    mu[mu0 == 0.0] = 0.75
    mu[np.isinf(mu0)] = 1e4
    return mu


def ladder(periods, variant, seed=0):
    """(row_ptr, col_idx, l, k or None, mu0) of `periods` periods of the variant's bands."""
    bands = period_bands(variant)
    B = len(bands)
    T = BAND * B * periods + NEAR_SPAN
    rng = np.random.default_rng(seed)
    tmpl = [_template(bands, rng) for _ in range(min(N_TEMPLATES, periods))]
    lens, cols, ks = [], [], []
    for p in range(periods):
        tl, th, tk, spare = tmpl[p % len(tmpl)]
        h = th + BAND * B * p
        # whole rows of zero, infinite and subnormal start values: where a run of the pattern begins inside band a1's first 64
        # transcripts, a row of a1 of the run's length becomes exactly the run (same length: the tiles stay as they are)
        lo = BAND * (B * p + 1)
        for (res, n), at in ((ZERO_RUN, spare[3][0]), (INF_RUN, spare[2][0]), (SUB_RUN, spare[3][1])):
            t = lo + (res - lo) % MU_PERIOD
            if t < lo + BAND:
                h[at:at + n] = np.arange(t, t + n)
        lens.append(tl); cols.append(h); ks.append(tk)
    if variant == "far":
        # every second band: 2 ... 5 rows of 3 ... 8 hits in the band's first 64 transcripts plus one or two hits a third of the
        # transcript range away (wrapping: below the window for the later bands, above it for the earlier, both for the middle)
        fl, fc = [], []
        for b in range(0, B * periods, 2):
            for j in range(2 + (b // 2) % 4):
                near = np.sort(rng.choice(BAND, size=3 + (b + j) % 6, replace=False)) + BAND * b
                x = BAND * b + 32 + j
                far = [(x + T // 3) % T, (x + 2 * (T // 3)) % T]
                far = far if j % 2 == 0 else far[(b // 2) % 2:][:1]
                row = np.sort(np.concatenate([near, np.asarray(far, np.int64)]))
                fl.append(row.size); fc.append(row)
        lens.append(np.asarray(fl, np.int64)); cols.append(np.concatenate(fc)); ks.append(np.ones(len(fl), np.uint32))
    lens = np.concatenate(lens)
    row_ptr = np.zeros(lens.size + 1, np.uint64)
    row_ptr[1:] = np.cumsum(lens)
    col_idx = np.concatenate(cols).astype(np.uint32)
    k = np.concatenate(ks)
    return row_ptr, col_idx, np.linspace(0.5, 2.0, T), (k if variant == "k" else None), mu_pattern(T)


# ---- the tile cut and the window rule, restated (mmgibbs.hip: problem_build_sell) ---------------------------------------------
def tile_table(row_ptr, col_idx, k, seg_key, row_id_base=0, max_seg=None):
    """The tiles of a STORED problem.  seg_key: a row's (near, band), i.e. its layout key >> 18 (an empty row's is ignored: it belongs
    to the run around it).  max_seg: the most runs of equal (near, band) the library cuts tiles by -- with more, the whole problem is
    one run (rows kept in the caller's order); None: no limit.
    Returns a dict of per-tile arrays: r0, nrows, nnz, maxlen, ng, call, cmax, far (the key's far bit), hask, knot1, kmax, odd (the tile
    starts on an odd row id); wbase and slid (the window moved in front of the tile) as ONE range over all tiles gives them, fast;
    and what the library derives before it lays the stream out (mmgibbs.hip: problem_build_sell; sell_kernels.h: k_tile_far):
      qual      the tile is on the register path: hits, no row above 255 hits, all hits inside the window of its smallest hit's band
      far_wbase, far_nn, far_nf   of a tile that has hits, does not qualify and has no row above 255 hits: the window base its rows
                were sorted for (the band field of its first non-empty row's key), the most hits a row has inside that window and the
                most it has outside -- far_nf = -1 where a row has a window hit behind a hit outside (not stored window-hits-first)
      far_tile  such a tile with 0 <= far_nf <= 255: a block for the window hits plus a far list of far_nf entries
      slow      a tile with hits that is neither: walked from the CSR
      blk_ng    the groups of the tile's block in the stream: ng for qual, ceil(far_nn / 4) for far_tile, else 0."""
    rp = np.asarray(row_ptr).astype(np.int64)
    col = np.asarray(col_idx)
    m = rp.size - 1
    L = np.diff(rp)
    seg_key = np.asarray(seg_key, np.uint64)
    ne = np.flatnonzero(L > 0)                                           # k_segment_starts: row 0, and a non-empty row whose key differs
    starts = ne[1:][seg_key[ne[1:]] != seg_key[ne[:-1]]]                 # from the last non-empty row's in front of it
    seg = sorted(set([0] + starts.tolist()))
    if max_seg is not None and len(seg) > max_seg:
        seg = [0]
    seg = seg + [m]
    r0 = []
    for s, e in zip(seg[:-1], seg[1:]):
        r = s
        while r < e:
            r0.append(r)
            r += 64 - ((int(row_id_base) + r) & 1)                      # a tile spans at most 32 Philox blocks
    r0 = np.asarray(r0, np.int64)
    nt = r0.size
    r1 = np.concatenate([r0[1:], [m]])
    nnz = rp[r1] - rp[r0]
    has = np.flatnonzero(nnz > 0)                                        # (reduceat over the tiles with hits: their first hits ascend strictly)
    call, cmax = np.zeros(nt, np.int64), np.zeros(nt, np.int64)
    if has.size:
        call[has] = np.minimum.reduceat(col, rp[r0[has]]).astype(np.int64)
        cmax[has] = np.maximum.reduceat(col, rp[r0[has]]).astype(np.int64)
    t = dict(r0=r0, nrows=r1 - r0, nnz=nnz, maxlen=np.maximum.reduceat(L, r0), call=call, cmax=cmax,
             odd=((int(row_id_base) + r0) & 1).astype(bool))
    first = np.minimum(np.searchsorted(ne, r0), max(ne.size - 1, 0))     # the tile's first non-empty row (a tile with hits has one)
    first = ne[first] if ne.size else np.zeros(nt, np.int64)
    t["far"] = (seg_key[first] >> np.uint64(45)).astype(bool) & (nnz > 0) if m else np.zeros(nt, bool)
    kk = np.ones(m, np.int64) if k is None else np.asarray(k).astype(np.int64)
    t["knot1"] = np.add.reduceat((kk != 1).astype(np.int64), r0)
    t["kmax"] = np.maximum.reduceat(kk, r0)
    t["hask"] = t["knot1"] > 0
    t["ng"] = (t["maxlen"] + 3) // 4
    wbase, slid, fast = np.zeros(nt, np.int64), np.zeros(nt, bool), np.zeros(nt, bool)
    have, cur = False, 0
    for i in range(nt):
        if t["far"][i]:                                                  # its own window: the home band's
            cur, have = int(seg_key[first[i]] & np.uint64((1 << 45) - 1)) * BAND, True
            wbase[i], slid[i] = cur, True
            continue
        # keep the window in force when the whole tile lies inside it; otherwise slide to the band start of its smallest id
        inside = have and t["call"][i] >= cur and t["cmax"][i] < cur + WIN
        if not inside:
            cur, have = int(t["call"][i]) & ~(BAND - 1), True
        wbase[i], slid[i] = cur, not inside
        fast[i] = t["maxlen"][i] <= 255 and t["nrows"][i] <= 64 and t["cmax"][i] < cur + WIN
    t.update(wbase=wbase, slid=slid, fast=fast)
    # the register path, and k_tile_far's answers for the tiles that miss it
    short = (nnz > 0) & (t["maxlen"] <= 255) & (t["nrows"] <= 64)
    t["qual"] = short & (cmax < (call & ~(BAND - 1)) + WIN)
    cand = short & ~t["qual"]
    far_wbase = np.where(cand, (seg_key[first] & np.uint64((1 << 45) - 1)).astype(np.int64) * BAND, 0) if m else np.zeros(nt, np.int64)
    far_nn, far_nf = np.zeros(nt, np.int64), np.full(nt, -1, np.int64)
    if cand.any():
        rid = np.repeat(np.arange(m, dtype=np.int64), L)
        tid = np.searchsorted(r0, rid, side="right") - 1
        sel = cand[tid]
        rid, tid, c = rid[sel], tid[sel], col[sel].astype(np.int64)
        pos = np.flatnonzero(sel) - rp[rid]                              # the hit's place in its row
        inw = ((c - far_wbase[tid]) & 0xffffffff) < WIN                  # (u32 wrap-around: a hit below the window is outside)
        n_in = np.bincount(rid, weights=inw, minlength=m).astype(np.int64)
        lead = np.bincount(rid, weights=inw & (pos < n_in[rid]), minlength=m).astype(np.int64)
        n_out = np.where(lead == n_in, L - n_in, 1 << 32)               # a window hit behind a far one: not stored window-hits-first
        ct = np.flatnonzero(cand)
        far_nn[ct] = np.maximum.reduceat(n_in, r0)[ct]
        nf = np.maximum.reduceat(n_out, r0)[ct]
        far_nf[ct] = np.where(nf <= 255, nf, -1)
    t["far_wbase"], t["far_nn"], t["far_nf"] = far_wbase, far_nn, far_nf
    t["far_tile"] = cand & (far_nf >= 0)
    t["slow"] = (nnz > 0) & ~t["qual"] & ~t["far_tile"]
    t["blk_ng"] = np.where(t["qual"], t["ng"], np.where(t["far_tile"], (far_nn + 3) // 4, 0))
    return t


def stored_tiles(orc, row_ptr, col_idx, k, row_id_base=0):
    """(stored problem as the oracle lays it out, its tile table): canonical_layout, then the restatement above."""
    rp, ci, kk, _ = orc.canonical_layout(row_ptr, col_idx, k)
    key, _ = orc.row_keys(rp, orc.sort_hits(rp, ci), kk)
    return (rp, ci, kk), tile_table(rp, ci, kk, key >> np.uint64(18), row_id_base)
