"""The call-order and index errors of the handles of several replicas: `DiffPoly`, `DiffChains` and `DiffPerm` share one state machine
on the host (DiffReplicas in mmseq_amd/csrc/diff.hip), so one walk through it serves the three.  The codes are those each family's
own entries returned before they were shared: MMG_ERR_ARG = 1, MMG_ERR_STATE = 4."""
import ctypes as C

import numpy as np
import pytest

import mmdiff_ref as R
from test_gpu_mmdiff import synth

ARG, STATE = 1, 4
FAMILIES = ["poly", "chains", "perm"]


def make(family, y, e, design):
    """A handle of two replicas on F = 10, N = 6 and the -de 3 3 design; chains with a total sampling length of 64."""
    from mmseq_amd.diff import DiffChains, DiffPerm, DiffPoly
    M, P0, P1, classes = design
    if family == "poly":
        return DiffPoly(y, e, M, P0, classes[:, 0], [P1, P1], [classes[:, 1], classes[:, 1]])
    if family == "chains":
        return DiffChains(y, e, *design, 2, 64)
    return DiffPerm(y, e, *design, 1)


def live(lib):
    from mmseq_amd._lib import check
    c = (C.c_int64 * 3)()
    check(lib.mmg_selftest_live(c))
    return tuple(c)


def code(call, *args):
    from mmseq_amd._lib import MMGError
    with pytest.raises(MMGError) as ex:
        call(*args)
    return ex.value.code, str(ex.value)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_call_order_and_index_errors(gpu, family):
    from mmseq_amd._lib import load
    y, e, _, _ = synth(10, 6, seed=5)
    design = R.de_design([3, 3])
    lib = load()
    base = live(lib)
    h = make(family, y, e, design)
    n = getattr(h, {"poly": "J", "chains": "C", "perm": "R"}[family])
    assert n == 2 and live(lib) != base
    # nothing runs before the burn-in
    assert code(h.tune_batch)[0] == STATE
    assert code(h.sample, 64)[0] == STATE
    assert code(h.results, 0)[0] == STATE
    # the burn-in: a multiple of 1024, once
    assert code(h.burnin, 1000)[0] == ARG
    h.burnin(1024)
    assert code(h.burnin, 1024)[0] == STATE
    assert code(h.sample, 0)[0] == ARG
    # a replica that is not there, before and after sampling (the entry itself: DiffPoly.results indexes its L1 before it calls)
    get_results = getattr(lib, "mmg_diff_%s_get_results" % family)
    assert get_results(h._h, n, None, None, None, None, None) == ARG
    assert code(h.info, n)[0] == ARG
    h.sample(64)
    assert get_results(h._h, n, None, None, None, None, None) == ARG
    assert h.results(n - 1)["gamma_mean"].shape == (10,)
    # no tuning once sampling has started
    assert code(h.tune_batch)[0] == STATE
    if family == "chains":
        rc, msg = code(h.sample, 16)
        assert rc == ARG and "total sampling length" in msg
    else:
        h.sample(16)
    h.close()
    assert live(lib) == base
