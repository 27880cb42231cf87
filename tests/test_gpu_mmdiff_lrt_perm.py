"""mmdiff -lrt FILE -lrtperm B on the device: DiffLrtPerm against the restatement (tests/mmdiff_lrt_perm_ref.py) with `==` on every
null statistic and status byte, the observed outputs with `==` against DiffLrt on the same arguments, the counts exactly and
perm_p / q_perm bitwise; slabs of every kind, lanes that leave at once, seeds and reruns, the call's error returns, the memory
formula and the CLI.

Which instantiation a case runs: k_lrt_perm<4> when both models have at most 4 columns (every -de design here, with a covariate
and with -fixalpha too); k_lrt_perm<0> (the triangle and theta in workspace slots) for k3: N = 12, three covariates, 4 and 5 columns."""
import numpy as np
import pytest

import mmdiff_lrt_perm_ref as LP
import mmdiff_lrt_ref as L
import mmdiff_ref as R
import wide_designs as W
from mmdiff_perm_ref import replica_data
from test_gpu_mmdiff import FAST, cli, synth, write_tables
from test_gpu_mmdiff_lrt import KEYS, cli_input

SEED = (0x5A17 << 32) | 42          # high bits set: the copy is xored into them
COVARIATE = np.array([[0.3], [1.1], [-0.4], [0.9], [0.0], [-1.2]])
PERM_KEYS = ("null_stat", "null_status", "perm_ge", "perm_n", "perm_p", "null_ge", "q_perm")


def _de(groups, F, seed, fixalpha=False, M=None):
    Md, P0, P1, C = R.de_design(groups)
    y, e, _, _ = synth(F, sum(groups), seed=seed, groups=list(groups))
    y[F // 2] = y[F // 2, 0]              # identical replicates: the boundary, in the data and in every copy
    return dict(y=y, e=e, M=Md if M is None else M, P0=P0, P1=P1, C=C, fixalpha=fixalpha)


def _k3(F):
    M, P0, P1, C = W.design("k3")
    y, e = W.data("k3", F, 5)
    return dict(y=y, e=e, M=M, P0=P0, P1=P1, C=C, fixalpha=False)


# name -> (the case, B)
CASES = {
    "de33": lambda: (_de((3, 3), 130, 11), 3),                      # two blocks of 64 and a third of 2 lanes
    "covariate": lambda: (_de((3, 3), 130, 12, M=COVARIATE), 3),
    "fixalpha": lambda: (_de((3, 3), 130, 13, fixalpha=True), 3),
    "f1_b1": lambda: (_de((3, 3), 1, 14), 1),
    "f1_b33": lambda: (_de((3, 3), 1, 15), 33),
    "f65_b1": lambda: (_de((3, 3), 65, 16), 1),                     # one lane past a block
    "n2": lambda: (_de((1, 1), 40, 17), 4),                         # one draw per shuffle; a saturated model 1
    "n7": lambda: (_de((3, 4), 40, 18), 4),
    "k3": lambda: (_k3(70), 5),                                     # PM = 0: the triangle and theta in the slab's workspace
}
REGISTERS = set(CASES) - {"k3"}


def run_device(c, B, seed=SEED, slab_copies=0, max_iters=0):
    from mmseq_amd.diff import DiffLrtPerm
    h = DiffLrtPerm(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], B, fixalpha=c["fixalpha"], max_iters=max_iters, seed=seed,
                    slab_copies=slab_copies)
    try:
        return h.results(), h.device_bytes()
    finally:
        h.close()


def run_plain(c):
    from mmseq_amd.diff import DiffLrt
    h = DiffLrt(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], fixalpha=c["fixalpha"])
    try:
        return h.results()
    finally:
        h.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def assert_same(got, want, keys, what=""):
    for k in keys:
        assert same_bits(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def k3_reference():
    c, B = CASES["k3"]()
    return c, B, LP.lrt_perm(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], B, c["fixalpha"], seed=SEED)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_restatement(gpu, name, k3_reference):
    if name == "k3":
        c, B, want = k3_reference
    else:
        c, B = CASES[name]()
        want = LP.lrt_perm(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], B, c["fixalpha"], seed=SEED)
    assert (max(want["n_cols"]) <= 4) == (name in REGISTERS)
    got, nbytes = run_device(c, B)
    F, N = c["y"].shape
    assert got["null_stat"].shape == got["null_status"].shape == (B, F)
    assert np.array_equal(got["null_stat"], want["null_stat"], equal_nan=True) and np.array_equal(got["null_status"], want["null_status"])
    assert_same(got, want, PERM_KEYS, name)
    # the observed test: DiffLrt on the same arguments, and the restatement
    plain = run_plain(c)
    assert got["df"] == plain["df"] and tuple(got["n_cols"]) == tuple(plain["n_cols"]) and tuple(got["n_classes"]) == tuple(plain["n_classes"])
    assert_same(got, plain, KEYS, name)
    assert_same(got, want, KEYS, name)
    assert nbytes == LP.perm_device_bytes(F, N, want["n_cols"], want["n_classes"], B)
    # the copies are fits like any other: finite, the boundary where the replicates are identical, and they are not the data's
    assert np.isfinite(got["null_stat"]).all() and np.all(got["perm_n"] == B)
    assert np.all(got["null_status"] & (L.ST_SINGULAR | L.ST_SINGULAR << 4) == 0)
    if name in ("de33", "f1_b1", "f1_b33", "f65_b1", "n2", "n7"):      # an intercept alone fits identical replicates: model 0 ends at 0
        assert np.all(got["null_status"][:, F // 2] & L.ST_BOUNDARY)
    if F > 1 and N > 2:
        assert np.any(got["null_stat"] != got["stat"][None, :])


@pytest.mark.gpu
def test_results_do_not_depend_on_the_slabs(gpu, k3_reference):
    """B = 5 copies in slabs of 1 (five launches), 2 (a partial last slab), 5 (one slab), the default, and more than B."""
    c, B, want = k3_reference
    F, N = c["y"].shape
    for Sc in (1, 2, 5, 0, 9):
        got, nbytes = run_device(c, B, slab_copies=Sc)
        assert_same(got, want, KEYS + PERM_KEYS, Sc)
        assert nbytes == LP.perm_device_bytes(F, N, want["n_cols"], want["n_classes"], B, asked=Sc)
    c, B = CASES["de33"]()                                         # and the register instantiation, device against device
    first, _ = run_device(c, B, slab_copies=1)
    for Sc in (2, 0):
        assert_same(run_device(c, B, slab_copies=Sc)[0], first, KEYS + PERM_KEYS, Sc)


@pytest.mark.gpu
def test_collinear_columns_and_unusable_weights_leave_at_once(gpu):
    c = _de((3, 3), 70, 21)
    rng = np.random.default_rng(3)
    M = np.round(rng.normal(0.0, 1.0, (6, 2)), 3)
    B = 4
    M2 = M.copy()
    M2[:, 1] = M2[:, 0]
    got, _ = run_device(dict(c, M=M2), B)
    assert np.isnan(got["null_stat"]).all() and np.all(got["null_status"] == (L.ST_SINGULAR | L.ST_SINGULAR << 4))
    assert np.isnan(got["stat"]).all() and np.all(got["perm_n"] == 0) and np.all(got["perm_ge"] == 0) and np.all(got["null_ge"] == 0)
    assert np.isnan(got["perm_p"]).all() and np.isnan(got["q_perm"]).all()
    # an e of 1e200 (finite, its square is not) travels with its sample through every shuffle: that feature is NaN alone
    good = dict(c, M=M)
    clean, _ = run_device(good, B)
    e = c["e"].copy()
    e[65, 2] = 1e200
    got, _ = run_device(dict(good, e=e), B)
    others = np.arange(70) != 65
    assert np.isnan(got["null_stat"][:, 65]).all() and np.all(got["null_status"][:, 65] == (L.ST_SINGULAR | L.ST_SINGULAR << 4))
    assert got["perm_n"][65] == 0 and got["perm_ge"][65] == 0 and np.isnan(got["perm_p"][65]) and np.isnan(got["q_perm"][65]) and got["null_ge"][65] == 0
    for k in ("stat", "null_stat", "null_status", "perm_ge", "perm_n", "perm_p"):
        assert same_bits(got[k][..., others], clean[k][..., others]), k
    assert np.isfinite(got["null_stat"][:, others]).all()
    want = LP.lrt_perm(c["y"], e, M, c["P0"], c["P1"], c["C"], B, seed=SEED)
    assert_same(got, want, KEYS + PERM_KEYS, "weights")


@pytest.mark.gpu
def test_seeds_reruns_and_the_copies_are_the_replicas_of_the_permutation_handle(gpu):
    c, B = _de((3, 3), 70, 31), 3
    a, _ = run_device(c, B)
    again, _ = run_device(c, B)
    assert_same(again, a, KEYS + PERM_KEYS, "rerun")
    other, _ = run_device(c, B, seed=SEED + 1)
    assert_same(other, a, KEYS, "seed")                            # the observed row does not see the seed
    assert not np.array_equal(other["null_stat"], a["null_stat"])
    # copy b is the plain test on the data replica b of DiffPerm holds (tests/mmdiff_perm_ref.replica_data, which
    # tests/test_gpu_mmdiff_perm.py holds that handle against), device against device
    for b in (1, B):
        yb, eb = replica_data(c["y"], c["e"], SEED, b)
        single = run_plain(dict(c, y=yb, e=eb))
        assert same_bits(a["null_stat"][b - 1], single["stat"]), b
        assert np.array_equal(a["null_status"][b - 1], (single["status"][0] | single["status"][1] << 4).astype(np.uint8)), b


@pytest.mark.gpu
def test_call_and_error_returns(gpu):
    import ctypes as C
    from mmseq_amd import _lib
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import DiffLrt, DiffLrtPerm, _ptr
    lib = _lib.load()
    c = _de((3, 3), 5, 41)
    args = (c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"])
    for B in (0, 65536):
        with pytest.raises(MMGError) as err:
            DiffLrtPerm(*args, B)
        assert err.value.code == 1 and "between 1 and 65535" in str(err.value)
    two = R.de_design((1, 1))
    with pytest.raises(MMGError) as err:
        DiffLrtPerm(np.ones((32769, 2)), np.ones((32769, 2)), *two, 65535)
    assert err.value.code == 1 and "at most 2147483647" in str(err.value)
    # NULL arguments
    y, e = np.ascontiguousarray(c["y"]), np.ascontiguousarray(c["e"])
    M, P0, P1 = (np.ascontiguousarray(c[k], np.float64) for k in ("M", "P0", "P1"))
    Cl = np.ascontiguousarray(c["C"], np.int32)
    full = [_ptr(y), _ptr(e), 1, _ptr(M), 1, _ptr(P0), 1, _ptr(P1), _ptr(Cl)]
    h = C.c_void_p()
    for i in (0, 1, 3, 5, 7, 8):
        a = list(full)
        a[i] = None
        assert lib.mmg_diff_lrt_perm_create(0, 5, 6, *a, 0, 0, 2, 1, 0, C.byref(h)) == 1 and not h.value
    assert lib.mmg_diff_lrt_perm_create(0, 5, 6, *full, 0, 0, 2, 1, 0, None) == 1
    assert lib.mmg_diff_lrt_perm_get(None, None, None, None, None, None) == 1
    assert lib.mmg_diff_lrt_perm_get_null(None, 0, 1, None, None) == 1
    assert lib.mmg_diff_lrt_perm_device_bytes(None, None) == 1
    assert not lib.mmg_diff_lrt_perm_observed(None)
    lib.mmg_diff_lrt_perm_destroy(None)
    # a handle: any out pointer may be NULL, a range past B is refused, a range inside it is those rows
    p = DiffLrtPerm(*args, 4, seed=SEED)
    try:
        r = p.results()
        assert lib.mmg_diff_lrt_perm_get(p._perm, None, None, None, None, None) == 0
        assert lib.mmg_diff_lrt_perm_get_null(p._perm, 0, 4, None, None) == 0
        for b0, nb in ((0, 5), (4, 1), (3, 2), (0xFFFFFFFF, 2)):
            assert lib.mmg_diff_lrt_perm_get_null(p._perm, b0, nb, None, None) == 1
        assert lib.mmg_diff_lrt_perm_get_null(p._perm, 4, 0, None, None) == 0
        stat, status = np.full((2, 5), -1.0), np.zeros((2, 5), np.uint8)
        assert lib.mmg_diff_lrt_perm_get_null(p._perm, 1, 2, _ptr(stat), _ptr(status)) == 0
        assert same_bits(stat, r["null_stat"][1:3]) and np.array_equal(status, r["null_status"][1:3])
        assert lib.mmg_diff_lrt_perm_device_bytes(p._perm, None) == 1
        assert p.device_bytes() == LP.perm_device_bytes(5, 6, r["n_cols"], r["n_classes"], 4)
        assert DiffLrt.device_bytes(p) == LP.lrt_device_bytes(5, 6, r["n_cols"], r["n_classes"])      # the observed test's own
    finally:
        p.close()


# ----------------------------------------------------------------------------- the CLI
@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    y, e, uh, _ = synth(60, 6, seed=51, groups=[3, 3])
    y[7] = y[7, 0]
    return write_tables(tmp_path_factory.mktemp("lrt_perm_tables"), y, e, uh)


def want_files(files, B, seed):
    feats, y, e = cli_input(files)
    M, P0, P1, C = R.de_design((3, 3))
    r = LP.lrt_perm(y, e, M, P0, P1, C, B, seed=seed)
    return L.lrt_file(feats, r, M, P0, P1, False), LP.lrt_perm_file(feats, r, M, P0, P1, False), r


def null_line(r, B):
    st = r["null_status"]
    bits = [int(((st >> k) & 1).sum() + ((st >> (4 + k)) & 1).sum()) for k in range(3)]
    return ("Null of the likelihood-ratio test: %d fits on %d shuffled copies; status bit 1 (cap) on %d, bit 2 (singular) on %d, "
            "bit 4 (boundary) on %d\n" % (2 * st.size, B, bits[0], bits[1], bits[2]))


@pytest.mark.gpu
def test_cli_appends_four_columns_and_leaves_stdout_alone(gpu, tmp_path, tables):
    plain_file, want, r = want_files(tables, 4, 1234)
    plain, _ = cli(FAST + ["-de", "3", "3"] + tables)
    out = tmp_path / "perm.lrt"
    stdout, err = cli(FAST + ["-lrt", str(out), "-lrtperm", "4", "-de", "3", "3"] + tables)
    assert stdout == plain and out.read_text() == want
    assert null_line(r, 4) in err and "Wrote the likelihood-ratio tests of 60 features" in err
    assert r["null_status"][:, 7].all()                             # (the identical replicates: the boundary bit is counted)


@pytest.mark.gpu
def test_cli_lrtonly_and_the_seed(gpu, tmp_path, tables):
    plain_file, want, r = want_files(tables, 4, 77)
    out, without = tmp_path / "perm.lrt", tmp_path / "plain.lrt"
    stdout, err = cli(["-seed", "77", "-lrt", str(out), "-lrtperm", "4", "-lrtonly", "-de", "3", "3"] + tables)
    assert stdout == "" and "BURNIN" not in err and out.read_text() == want and null_line(r, 4) in err
    stdout, err = cli(["-lrt", str(without), "-lrtonly", "-de", "3", "3"] + tables)
    assert stdout == "" and without.read_text() == plain_file and "Null of the" not in err
    # the first columns: the file of the run without the flag, line by line
    for a, b in zip(out.read_text().split("\n"), plain_file.split("\n")):
        assert a == b == "" or (a.startswith(b + "\t") and a[len(b):].count("\t") == 4)
