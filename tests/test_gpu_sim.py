"""mmg_sim_* on the device (mmseq_amd.Similarity, the mmsim CLI) against tests/sim_ref.py: the Gram matrices exactly on integer data
over the tile, k-step, chunk and block edges, z and the used features with ==, the Gram of real draws within the bound of a dot
product, stage 2 with == from the device's own Gram, an end-to-end case with the propagated bound, reruns, the memory formula, the
error codes, failed acquisitions, and the CLI's table."""
import ctypes as C
import gc
import subprocess

import numpy as np
import pytest

import sim_ref as R
from sim_fixtures import MMSIM, draws as _draws, write_table, write_trace

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DEV_KEYS = ("mean_D", "ss_D", "q_D", "mean_R", "ss_R", "q_R", "nn", "pair_status", "status")


def _sim(traces, offs=None, ranks=(), centre=None, mask=None, logged=False, want_z=False):
    """traces: (S, T, F) -> everything the handle returns"""
    from mmseq_amd import Similarity
    traces = np.asarray(traces, np.float64)
    S, T, F = traces.shape
    with Similarity(S, F, T, centre=centre, mask=mask, logged=logged) as h:
        for s in range(S):
            h.set_sample(s, traces[s], 0.0 if offs is None else offs[s])
        h.run(ranks)
        used, n = h.used()
        G, m = h.gram()
        out = dict(used=used, n=n, G=G, m=m, summary=h.summary(), bytes=h.device_bytes())
        if want_z:
            out["z"] = np.array([h.z(s) for s in range(S)])
    return out


def _same_summary(got, ref, what=None):
    for k in DEV_KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        assert np.array_equal(g, r, equal_nan=True), (what, k, np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r))))[:5])


# ------------------------------------------------------------------------------------------ stage 1 on integers: every sum exact
def _integers(seed, S, F, T):
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, (S, T, F)).astype(np.float64)
    c = rng.integers(-3, 4, F).astype(np.float64)
    return v, c


def _exact_gram(v, c, used=None):
    z = (v - c[None, None, :]).astype(np.int64)
    if used is not None:
        z = z[:, :, np.asarray(used) != 0]
    return np.einsum("rtf,stf->trs", z, z), z.sum(axis=2).T, z.shape[2]


def _check_exact(got, v, c, what):
    G, m, n = _exact_gram(v, c)
    assert got["n"] == n and got["used"].all(), what
    assert np.array_equal(got["m"], m.astype(np.float64)), (what, np.argwhere(got["m"] != m)[:5])
    assert np.array_equal(got["G"], G.astype(np.float64)), (what, np.argwhere(got["G"] != G)[:5])


@pytest.mark.parametrize("S", [2, 15, 16, 17, 63, 64, 65, 130])
def test_gram_is_exact_on_integers_at_the_tile_and_block_edges(gpu, S):
    """S + 1 rows: 16 and 64 are one past a tile and a block, 15 and 63 fill them, 130 is three blocks per side"""
    v, c = _integers(S, S, 67, 3)
    _check_exact(_sim(v, centre=c, logged=True), v, c, S)


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 63, 64, 65, 1000])
def test_gram_is_exact_on_integers_at_the_k_step_edges(gpu, F):
    v, c = _integers(100 + F, 5, F, 2)
    _check_exact(_sim(v, centre=c, logged=True), v, c, F)


@pytest.mark.parametrize("chunk", [1, 4, 7, 64])
@pytest.mark.parametrize("S", [5, 70])
def test_gram_is_exact_on_integers_at_the_chunk_edges(gpu, chunk, S):
    v, c = _integers(200 + chunk + S, S, 67, 3)
    F = 67
    NT = (S + 1 + 15) // 16
    with gpu.options(sim_chunk=chunk):
        got = _sim(v, centre=c, logged=True)
    _check_exact(got, v, c, (chunk, S))
    assert got["bytes"] == _bytes(S, F, 3, chunk, -(-F // chunk)), (chunk, S)
    assert NT == (1 if S == 5 else 5)


def test_gram_is_exact_on_integers_at_the_most_samples(gpu):
    v, c = _integers(256, 256, 8, 1)
    _check_exact(_sim(v, centre=c, logged=True), v, c, 256)


def test_invalid_and_masked_features_do_not_reach_the_gram_of_integers(gpu):
    v, c = _integers(7, 6, 90, 4)
    mask = np.ones(90, np.uint8)
    mask[[0, 17, 89]] = 0
    v[1, 2, 5] = np.nan; v[3, 0, 64] = np.inf; v[5, 3, 33] = -np.inf
    with gpu.options(sim_chunk=16):
        got = _sim(v, centre=c, mask=mask, logged=True, want_z=True)
    used = mask.copy()
    used[[5, 64, 33]] = 0
    assert np.array_equal(got["used"], used) and got["n"] == 84
    vv = np.where(np.isfinite(v), v, 0.0)
    G, m, n = _exact_gram(vv, c, used)
    assert n == 84 and np.array_equal(got["G"], G.astype(np.float64)) and np.array_equal(got["m"], m.astype(np.float64))
    assert (got["z"][:, :, used == 0] == 0.0).all()


# ------------------------------------------------------------------------------------------ z, used and the Gram of real draws
def _traces(rng, S, F, T, sig=None):
    return np.array([_draws(rng, F, T, sig=sig).T for _ in range(S)])


def _gram_within_the_bound(got, ref, what):
    z = ref["z"][:, :, ref["used"] != 0]
    n = ref["n"]
    az = np.abs(z).astype(np.longdouble)
    bG = (n + 1) * U * np.einsum("rtf,stf->trs", az, az)
    bm = (n + 1) * U * az.sum(axis=2).T
    eG = np.abs(got["G"].astype(np.longdouble) - ref["G"])
    em = np.abs(got["m"].astype(np.longdouble) - ref["m"])
    assert (eG <= bG).all(), (what, float((eG / bG).max()))
    assert (em <= bm).all(), (what, float((em / bm).max()))
    assert np.array_equal(got["G"], got["G"].transpose(0, 2, 1)), what
    return bG, bm


def test_z_and_used_are_the_references(gpu):
    rng = np.random.default_rng(3)
    S, F, T = 3, 200, 17
    v = _traces(rng, S, F, T)
    v[0, 3, 10] = 0.0; v[1, 16, 11] = -1.5; v[2, 0, 12] = np.nan; v[0, 9, 199] = np.inf; v[2, 7, 0] = -np.inf; v[1, 1, 64] = 0.0
    mask = np.ones(F, np.uint8)
    mask[[5, 11, 128]] = 0
    centre = rng.normal(-3.0, 1.0, F)
    offs = [0.0, 0.25, -0.125]
    ref = R.sim_ref(v, offs, [0, 8, 16], centre=centre, mask=mask)
    got = _sim(v, offs, [0, 8, 16], centre=centre, mask=mask, want_z=True)
    assert np.array_equal(got["used"], ref["used"]) and got["n"] == ref["n"] == F - 8
    assert np.array_equal(got["z"], ref["z"])
    assert not np.signbit(got["z"]).any() or (got["z"][np.signbit(got["z"])] != 0.0).all()   # no -0.0
    _gram_within_the_bound(got, ref, "z")                      # the Gram of the used columns alone
    _same_summary(got["summary"], R.summary_from_gram(got["G"], got["m"], got["n"], [0, 8, 16]))


@pytest.mark.parametrize("S,F,T", [(7, 1003, 5), (70, 129, 2)])
def test_gram_of_real_draws_is_within_the_bound_of_a_dot_product(gpu, S, F, T):
    """|G_dev - G_ref| <= (n + 1) 2^-53 sum_f |z_rf z_sf| with G_ref in longdouble: the bound of a dot product in any order, with or
    without fused multiply-add; the + 1 covers the reference's own rounding.  m likewise with sum |z|."""
    rng = np.random.default_rng(S)
    v = _traces(rng, S, F, T)
    offs = list(rng.normal(0.0, 0.2, S))
    ref = R.sim_ref(v, offs, [])
    got = _sim(v, offs, [])
    assert got["n"] == F
    _gram_within_the_bound(got, ref, (S, F, T))


# ------------------------------------------------------------------------------------------ stage 2 from the device's own Gram
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 1000, 4096])
def test_stage_two_is_the_references_from_the_devices_gram(gpu, T):
    rng = np.random.default_rng(T)
    v = _traces(rng, 3, 20, T, sig=3)
    ranks = [0, T - 1, T // 2, R.percentile_rank(2.5, T), T // 2, T, T + 5, R.percentile_rank(97.5, T)]
    got = _sim(v, [0.0, 0.1, -0.2], ranks, centre=np.log(v).mean(axis=(0, 1)))
    ref = R.summary_from_gram(got["G"], got["m"], got["n"], ranks)
    _same_summary(got["summary"], ref, T)
    s = got["summary"]
    assert s["status"] == 0 and (s["pair_status"] == 0).all()
    assert np.isnan(s["q_D"][:, 5:7]).all() and np.isfinite(s["q_D"][:, :5]).all() and np.isfinite(s["q_R"][:, :5]).all()
    assert np.array_equal(s["q_D"][:, 2], s["q_D"][:, 4])
    assert (s["nn"].sum(axis=1) == T).all() and (np.diag(s["nn"]) == 0).all()


def test_identical_samples_a_constant_sample_and_too_few_features(gpu):
    rng = np.random.default_rng(41)
    T, F = 65, 20
    v = np.log(_traces(rng, 4, F, T))
    v[1] = v[0]                                                # two identical samples
    v[3] = 2.0                                                 # a constant sample: its variance term is 80 - 40 * 40 / 20 = 0
    ranks = [0, 32, 64]
    got = _sim(v, None, ranks, logged=True)
    s = got["summary"]
    _same_summary(s, R.summary_from_gram(got["G"], got["m"], got["n"], ranks))
    pairs = R.pairs_of(4)
    p01 = pairs.index((0, 1))
    assert s["mean_D"][p01] == 0.0 and s["ss_D"][p01] == 0.0 and (s["q_D"][p01] == 0.0).all()
    assert s["nn"][0, 1] == T and s["nn"][1, 0] == T
    for p, (a, b) in enumerate(pairs):
        if b == 3:
            assert s["pair_status"][p] == 2 and np.isnan(s["mean_R"][p]) and np.isnan(s["ss_R"][p]) and np.isnan(s["q_R"][p]).all()
            assert np.isfinite(s["mean_D"][p]) and np.isfinite(s["q_D"][p]).all()
        else:
            assert s["pair_status"][p] == 0 and np.isfinite(s["mean_R"][p])
    for keep in (1, 0):                                        # n < 2
        mask = np.zeros(F, np.uint8)
        mask[:keep] = 1
        few = _sim(v, None, ranks, mask=mask, logged=True)
        s = few["summary"]
        assert few["n"] == keep and s["status"] == 1 and (s["nn"] == 0).all() and (s["pair_status"] == 0).all()
        for k in ("mean_D", "ss_D", "q_D", "mean_R", "ss_R", "q_R", "sd_D", "sd_R"):
            assert np.isnan(s[k]).all(), k
        _same_summary(s, R.summary_from_gram(few["G"], few["m"], few["n"], ranks))


# ------------------------------------------------------------------------------------------ end to end
def test_two_pairs_of_close_samples_end_to_end(gpu):
    """S = 4, F = 300, T = 64 and all 64 ranks, so the sorted D[t] and R[t] themselves come back.  The propagation, to first order
    and doubled for the neglected second-order terms, with u = 2^-53, bG and bm the stage-1 bounds above, and every operation of
    stage 2 adding a relative u:
      num = (G_rr + G_ss) - 2 G_rs:  E_num = bG_rr + bG_ss + 2 bG_rs + 4 u (G_rr + G_ss + 2 |G_rs|)
      D = sqrt(num / n):             E_D = E_num / (2 n D) + 4 u D
      cov = G_rs - m_r m_s / n:      E_cov = bG_rs + (|m_s| bm_r + |m_r| bm_s) / n + 4 u (|G_rs| + |m_r m_s| / n);  E_va, E_vb alike
      R = cov / sqrt(va vb):         E_R = E_cov / sqrt(va vb) + |R| (E_va / va + E_vb / vb) / 2 + 8 u |R|
    Sorting moves no value by more than the largest error, so sorted series are compared with the maximum over t; a mean adds
    (T + 1) u max |x|."""
    rng = np.random.default_rng(64)
    S, F, T = 4, 300, 64
    prof = [rng.normal(-3.0, 2.0, F), rng.normal(-3.0, 2.0, F)]
    v = np.array([np.exp(prof[s // 2][None, :] + 0.05 * rng.normal(0.0, 1.0, (T, F))) for s in range(S)])
    offs = [0.0, 0.1, -0.1, 0.05]
    lm = np.array([prof[s // 2] - offs[s] for s in range(S)]).T
    centre = R.centre_of(lm, offs, np.ones(F, bool))
    v = v * np.exp(-np.array(offs))[:, None, None]
    ranks = list(range(T))
    ref = R.sim_ref(v, offs, ranks, centre=centre)
    got = _sim(v, offs, ranks, centre=centre)
    bG, bm = _gram_within_the_bound(got, ref, "e2e")
    s = got["summary"]
    assert s["status"] == 0 and (s["pair_status"] == 0).all()
    want_nn = np.zeros((S, S), np.uint32)
    for a, b in ((0, 1), (1, 0), (2, 3), (3, 2)):
        want_nn[a, b] = T
    assert np.array_equal(s["nn"], want_nn) and np.array_equal(ref["nn"], want_nn)
    G, m, n = ref["G"], ref["m"], np.longdouble(ref["n"])
    for p, (a, b) in enumerate(R.pairs_of(S)):
        gaa, gbb, gab, ma, mb = G[:, a, a], G[:, b, b], G[:, a, b], m[:, a], m[:, b]
        D = np.sqrt(((gaa + gbb) - 2 * gab) / n)
        E_num = bG[:, a, a] + bG[:, b, b] + 2 * bG[:, a, b] + 4 * U * (gaa + gbb + 2 * np.abs(gab))
        E_D = 2 * float((E_num / (2 * n * D) + 4 * U * D).max())
        va, vb, cov = gaa - ma * ma / n, gbb - mb * mb / n, gab - ma * mb / n
        Rr = cov / np.sqrt(va * vb)
        E_cov = bG[:, a, b] + (np.abs(mb) * bm[:, a] + np.abs(ma) * bm[:, b]) / n + 4 * U * (np.abs(gab) + np.abs(ma * mb) / n)
        E_va = bG[:, a, a] + 2 * np.abs(ma) * bm[:, a] / n + 4 * U * (gaa + ma * ma / n)
        E_vb = bG[:, b, b] + 2 * np.abs(mb) * bm[:, b] / n + 4 * U * (gbb + mb * mb / n)
        E_R = 2 * float((E_cov / np.sqrt(va * vb) + np.abs(Rr) * (E_va / va + E_vb / vb) / 2 + 8 * U * np.abs(Rr)).max())
        eD = np.abs(s["q_D"][p].astype(np.longdouble) - np.sort(D))
        eR = np.abs(s["q_R"][p].astype(np.longdouble) - np.sort(Rr))
        print("pair", (a, b), "D error", float(eD.max()), "bound", E_D, "R error", float(eR.max()), "bound", E_R)
        assert (eD <= E_D).all() and (eR <= E_R).all(), (a, b)
        assert abs(float(s["mean_D"][p] - D.mean())) <= E_D + (T + 1) * U * float(D.max())
        assert abs(float(s["mean_R"][p] - Rr.mean())) <= E_R + (T + 1) * U * float(np.abs(Rr).max())
        close = (a, b) in ((0, 1), (2, 3))
        assert (s["mean_D"][p] < 0.2) == close and (s["mean_R"][p] > 0.9) == close


# ------------------------------------------------------------------------------------------ reruns, memory, errors
def _bytes(S, F, T, CH=None, chunks=None):
    NT = (S + 1 + 15) // 16
    U_ = NT * (NT + 1) // 2
    if CH is None:
        CH = min(F, max(4096, -(-F // 65535)))
        chunks = -(-F // CH)
    P = S * (S - 1) // 2
    return 8 * S * T * F + F * (S + 18) + 2048 * T * chunks * U_ + 8 * T * (S * S + S + 1) + 8 + 1057 * P + 4 * S * S + 256


def test_reruns_are_bit_identical_and_the_memory_is_the_formulas(gpu):
    from mmseq_amd import Similarity
    rng = np.random.default_rng(12)
    S, F, T = 5, 9000, 9
    v = _traces(rng, S, F, T, sig=4)
    ranks = [0, 4, 8]
    runs = []
    for _ in range(2):
        with Similarity(S, F, T) as h:
            for s in range(S):
                h.set_sample(s, v[s], 0.01 * s)
            h.set_sample(2, v[2], 0.02)                        # a sample set again before the run
            h.run(ranks)
            first = (h.gram(), h.summary())
            h.run(ranks)
            again = (h.gram(), h.summary())
            h.run([8])                                         # other ranks: the rest is what it was
            other = h.summary()
            assert h.device_bytes() == _bytes(S, F, T)
            runs.append(first)
        for a, b in ((first, again),):
            assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1])
            _same_summary(a[1], b[1])
        assert np.array_equal(other["q_D"][:, 0], first[1]["q_D"][:, 2]) and np.array_equal(other["mean_R"], first[1]["mean_R"])
    assert np.array_equal(runs[0][0][0], runs[1][0][0]) and np.array_equal(runs[0][0][1], runs[1][0][1])
    _same_summary(runs[0][1], runs[1][1])
    assert -(-F // 4096) == 3                                  # three chunks at the default length


def _live(lib):
    from mmseq_amd import _lib
    c = (C.c_int64 * 3)()
    _lib.check(lib.mmg_selftest_live(c))
    return list(c)


def test_the_errors_leave_the_library_usable(gpu):
    from mmseq_amd import Similarity, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(9)
    v = _traces(rng, 3, 10, 4)
    good = _sim(v, None, [0, 3])
    gc.collect()
    base = _live(lib)
    hnd = C.c_void_p()

    def create(S=3, F=10, T=4, centre=None, flags=0, out=C.byref(hnd), device=0):
        rc = lib.mmg_sim_create(device, S, F, T, centre, None, flags, out)
        return rc, lib.mmg_last_error().decode()

    bad_centre = np.zeros(10)
    bad_centre[7] = np.inf
    for kw, text in ((dict(S=1), "S = 1"), (dict(S=257), "S = 257"), (dict(F=0), "F = 0"), (dict(F=1 << 31), "F = 2147483648"), (dict(T=0), "T = 0"),
                     (dict(T=4097), "T = 4097"), (dict(flags=2), "flags = 2"), (dict(centre=bad_centre.ctypes.data_as(C.c_void_p)), "centre[7]"),
                     (dict(out=None), "NULL"), (dict(device=99), "device")):
        rc, msg = create(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    rc, msg = create(S=256, F=(1 << 31) - 1, T=4096)          # in order, but 16 PiB
    assert rc == 1 and str(8 * 256 * 4096 * ((1 << 31) - 1)) in msg and "free memory of" in msg, msg
    assert _live(lib) == base
    with Similarity(3, 10, 4) as h:
        for s, tr, off, code, text in ((3, v[0], 0.0, 1, "s = 3"), (0, v[0], float("nan"), 1, "off"), (0, v[0], float("inf"), 1, "off")):
            with pytest.raises(MMGError) as e:
                h.set_sample(s, tr, off)
            assert e.value.code == code and text in str(e.value)
        assert lib.mmg_sim_set_sample(h._h, 0, None, 0.0) == 1 and b"trace" in lib.mmg_last_error()
        h.set_sample(0, v[0])
        h.set_sample(2, v[2])
        with pytest.raises(MMGError) as e:
            h.run([0])
        assert e.value.code == 4 and "sample 1" in str(e.value)
        for call in (h.used, h.gram, h.summary, lambda: h.z(1)):
            with pytest.raises(MMGError) as e:
                call()
            assert e.value.code == 4
        h.set_sample(1, v[1])
        with pytest.raises(MMGError) as e:
            h.run(list(range(65)))
        assert e.value.code == 1 and "n_ranks = 65" in str(e.value)
        assert lib.mmg_sim_run(h._h, 2, None) == 1 and b"ranks" in lib.mmg_last_error()
        assert lib.mmg_sim_get_z(h._h, 0, 3, 2, None) == 1 and lib.mmg_sim_get_z(h._h, 5, 0, 1, None) == 1
        h.run([0, 3])
        _same_summary(h.summary(), good["summary"])
        assert lib.mmg_sim_get_gram(h._h, 4, 1, None, None) == 1
        with pytest.raises(MMGError) as e:
            h.set_sample(0, v[0])
        assert e.value.code == 4
    for fn, args in (("mmg_sim_set_sample", (None, 0, None, 0.0)), ("mmg_sim_run", (None, 0, None)), ("mmg_sim_get_used", (None, None, None)),
                     ("mmg_sim_get_z", (None, 0, 0, 0, None)), ("mmg_sim_get_gram", (None, 0, 0, None, None)), ("mmg_sim_get", (None,) * 10),
                     ("mmg_sim_device_bytes", (None, None))):
        assert getattr(lib, fn)(*args) == 1, fn
    lib.mmg_sim_destroy(None)
    gc.collect()
    assert _live(lib) == base
    _same_summary(_sim(v, None, [0, 3])["summary"], good["summary"])


def test_failed_acquisitions_give_back_everything(gpu):
    from mmseq_amd import Similarity, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(10)
    v = _traces(rng, 3, 40, 6)
    want = _sim(v, None, [0, 5])
    gc.collect()
    base = _live(lib)
    n = 0
    try:
        while True:
            _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, n))
            try:
                h = Similarity(3, 40, 6)
            except MMGError as e:
                assert e.code == 3 and str(e)
                assert _live(lib) == base, n
                n += 1
                continue
            break
    finally:
        lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
    assert n == 17                                             # the stream and the sixteen buffers of a handle
    for s in range(3):
        h.set_sample(s, v[s])
    h.run([0, 5])
    got = (h.gram(), h.summary())
    h.close()
    assert _live(lib) == base
    assert np.array_equal(got[0][0], want["G"]) and np.array_equal(got[0][1], want["m"])
    _same_summary(got[1], want["summary"])


# ------------------------------------------------------------------------------------------ the CLI
def _close_to_six_digits(got, want):
    """within 2 units of the sixth significant digit of the number the restatement prints"""
    if np.isnan(want):
        return np.isnan(got)
    if want == 0.0:
        return got == 0.0
    return abs(got - want) <= 2.0 * 10.0 ** (np.floor(np.log10(abs(want))) - 5)


def test_cli_table_and_matrix(gpu, tmp_path):
    rng = np.random.default_rng(77)
    S, F, T = 3, 120, 16
    ids = ["f%d" % i for i in range(F)]
    prof = rng.normal(1.0, 1.5, F)
    bases, log_mu, uh, traces = [], [], [], []
    for s in range(S):
        base = str(tmp_path / ("s%d" % s))
        lm = prof + rng.normal(0.0, 0.3, F) + 0.2 * s
        u = [int(x) for x in rng.integers(1, 6, F)]
        if s == 1:
            u[3] = 0                                           # below -uhmin in one sample
        write_table(base + ".mmseq", ids, ["NA" if (s == 2 and f == 5) else lm[f] for f in range(F)], u)
        tids = [i for i in ids if not (s == 0 and i == "f7")][::-1]     # sample 0 has no column for f7; the columns in another order
        draws = np.exp(np.array([lm[ids.index(i)] for i in tids])[:, None] + 0.1 * rng.normal(0.0, 1.0, (len(tids), T)))
        if s == 2:
            draws[tids.index("f9"), 4] = 0.0                   # an invalid draw
        read = write_trace(base + ".trace_gibbs.gz", tids, draws, rows=T)
        full = np.zeros((T, F))
        for k, i in enumerate(tids):
            full[:, ids.index(i)] = read[k]
        lm = lm.copy()
        if s == 2:
            lm[5] = np.nan
        bases.append(base); log_mu.append(lm); uh.append(u); traces.append(full)
    log_mu, uh = np.array(log_mu).T, np.array(uh).T
    traced = np.ones((F, S), bool)
    traced[7, 0] = False
    offs, n_norm = R.offsets(log_mu, uh)
    assert n_norm == F - 2 and all(o != 0.0 for o in offs)
    mask = R.feature_mask(log_mu, uh, traced)
    assert mask.sum() == F - 3
    centre = R.centre_of(log_mu, offs, mask)
    ranks = [R.percentile_rank(50, T)]
    ref = R.sim_ref(np.array(traces), offs, ranks, centre=centre, mask=mask)
    assert ref["n"] == F - 4
    want = R.table(bases, "transcript", T, ref["n"], F, offs, "mean", [50.0], ref).decode().splitlines()
    mpath = str(tmp_path / "dist.txt")
    r = subprocess.run([MMSIM, "-percentiles", "50", "-matrix", mpath] + bases, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    got = r.stdout.decode().splitlines()
    assert len(got) == len(want) == 5 + S + 1 + 3
    assert got[:5] == want[:5] and got[5 + S] == want[5 + S]
    for g, w in zip(got[5:5 + S], want[5:5 + S]):             # the sample lines: the offset to six digits
        assert g.rsplit(" ", 1)[0] == w.rsplit(" ", 1)[0] and _close_to_six_digits(float(g.rsplit(" ", 1)[1]), float(w.rsplit(" ", 1)[1]))
    for g, w in zip(got[5 + S + 1:], want[5 + S + 1:]):
        gc_, wc = g.split("\t"), w.split("\t")
        assert gc_[:2] == wc[:2] and gc_[-1] == wc[-1] == "0" and len(gc_) == len(wc) == 11
        for a, b in zip(gc_[2:-1], wc[2:-1]):
            assert _close_to_six_digits(float(a), float(b)), (g, w)
    M = [line.split("\t") for line in open(mpath).read().splitlines()]
    assert M[0] == [""] + bases and [row[0] for row in M[1:]] == bases
    A = np.array([[float(x) for x in row[1:]] for row in M[1:]])
    assert np.array_equal(A, A.T) and (np.diag(A) == 0.0).all() and (A[~np.eye(S, dtype=bool)] > 0).all()
    wantM = R.matrix(bases, ref).decode().splitlines()
    for g, w in zip(M[1:], [line.split("\t") for line in wantM[1:]]):
        for a, b in zip(g[1:], w[1:]):
            assert _close_to_six_digits(float(a), float(b))
