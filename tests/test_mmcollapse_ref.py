"""CPU checks of mmcollapse's yardsticks and host-side argument checks: the oracle's keyed simulated trace (the draw of DESIGN.md
section 9, difference 1) against the library's host draw, and mmg_collapse_summarize's argument checks, which run before any
device is touched."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as B


def test_keyed_simu_trace_at_the_mmseq_key_is_the_mmseq_draw():
    from mmseq_amd import _lib
    lib = _lib.load()
    for seed, sid, shape, scale in ((13837, 0, 0.1, 1.0), (31, 77, 0.1, 3.5e-7), (9, 901, 2.5, 0.5)):
        want = B.simu_gamma_trace(seed, sid, shape, scale, 1024)
        got = B.simu_gamma_trace_keyed(seed, 0, B.TAG_SIMU, sid, shape, scale, 1024)
        assert got.tobytes() == want.tobytes()
        host = np.empty(1024)
        _lib.check(lib.mmg_host_gamma_trace(seed, sid, shape, scale, 1024, host.ctypes.data_as(C.c_void_p)))
        assert host.tobytes() == want.tobytes()


def test_keyed_simu_trace_depends_on_chain_and_tag():
    base = B.simu_gamma_trace_keyed(13837, 0, B.TAG_COLLAPSE_SIMU, 5, 0.1, 1.0, 1024)
    others = [B.simu_gamma_trace_keyed(13837, 1, B.TAG_COLLAPSE_SIMU, 5, 0.1, 1.0, 1024),
              B.simu_gamma_trace_keyed(13837, 2, B.TAG_COLLAPSE_SIMU, 5, 0.1, 1.0, 1024),
              B.simu_gamma_trace_keyed(13837, 0, B.TAG_SIMU, 5, 0.1, 1.0, 1024),
              B.simu_gamma_trace_keyed(13837, 0, B.TAG_COLLAPSE_SIMU, 6, 0.1, 1.0, 1024)]
    for o in others:
        assert np.count_nonzero(o == base) == 0
    assert np.all(base > 0) and np.all(np.isfinite(base))
    # the scale multiplies one unit draw
    s = B.simu_gamma_trace_keyed(13837, 0, B.TAG_COLLAPSE_SIMU, 5, 0.1, 4.0, 1024)
    assert s.tobytes() == (base * 4.0).tobytes()


def _summarize_raw(trace_len=16, n_cols=2, n_virtual=1, ptr=(0, 1, 3), members=(0, 1, 2), stream=0):
    from mmseq_amd import _lib
    lib = _lib.load()
    tr = np.ones((trace_len, n_cols))
    vid = np.arange(n_virtual, dtype=np.uint64)
    vsc = np.ones(n_virtual)
    ptr = np.asarray(ptr, np.uint64)
    mem = np.asarray(members, np.uint32)
    g = len(ptr) - 1
    lm, var, tau = (np.empty(max(g, 1)) for _ in range(3))
    rc = np.empty(max(g, 1), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    _lib.check(lib.mmg_collapse_summarize(0, trace_len, n_cols, p(tr), n_virtual, p(vid), p(vsc), 0.1, 13837, stream, g, p(ptr),
                                          p(mem), p(lm), p(var), p(tau), p(rc)))


@pytest.mark.parametrize("kw", [dict(ptr=(0, 2, 1), members=(0, 1)),                  # series_ptr decreasing
                                dict(ptr=(1, 2, 3), members=(0, 1, 2)),               # series_ptr[0] != 0
                                dict(ptr=(0, 1, 3), members=(0, 1, 3)),               # member >= n_cols + n_virtual
                                dict(n_virtual=0, ptr=(0, 1, 2), members=(0, 2)),     # a virtual member without virtual traces
                                dict(stream=1 << 24),                                 # stream beyond 24 bits
                                dict(trace_len=0)],
                         ids=["ptr-decreasing", "ptr0", "member-range", "member-no-virtual", "stream", "trace-len-0"])
def test_summarize_argument_checks_happen_before_device_use(kw):
    from mmseq_amd._lib import MMGError
    with pytest.raises(MMGError) as e:
        _summarize_raw(**kw)
    assert e.value.code == 1
