"""CPU checks of the drop-in boundary: libmmgibbs.so loads, exports every symbol include/mmgibbs.h
declares, refuses to compute without a device (no fallback), and the host instantiation of its
inline math/RNG equals the oracle bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "mmgibbs.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mmg_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from mmseq_amd import _lib
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), "libmmgibbs.so does not export %s" % name
    assert sorted(_lib.SYMBOLS) == declared, "python binding table out of sync with include/mmgibbs.h"
    assert lib.mmg_abi_version() == 8


def test_selftest_options_and_the_series_launch_record():
    """the option table of the binding is the header's, MMG_OPT_SERIES_GROUPS is its last entry, and mmg_selftest_series_launch answers
    for its four kernels on the host alone: zeros while no workspace instantiation was launched (no device here), MMG_ERR_ARG otherwise"""
    from mmseq_amd import _lib, gibbs
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "mmgibbs.h")).read()
    ids = {name: int(v) for name, v in re.findall(r"\bMMG_(OPT_[A-Z0-9_]+?)_? = (\d+)", txt)}
    count = ids.pop("OPT_COUNT")
    assert count == 26 and sorted(ids.values()) == list(range(count))
    assert {k: v for k, v in vars(_lib).items() if k.startswith("OPT_")} == ids
    assert _lib.OPT_SERIES_GROUPS == 25 and gibbs.OPT["series_groups"] == 25 and sorted(gibbs.OPT.values()) == sorted(set(gibbs.OPT.values()))
    assert lib.mmg_selftest_option(_lib.OPT_SERIES_GROUPS, 2) == 0 and lib.mmg_selftest_option(_lib.OPT_SERIES_GROUPS, -1) == 0
    assert lib.mmg_selftest_option(count, 1) == 1
    g, c = C.c_uint32(7), C.c_uint32(7)
    if gibbs.device_count() == 0:
        for kernel in range(4):
            assert lib.mmg_selftest_series_launch(kernel, C.byref(g), C.byref(c)) == 0 and (g.value, c.value) == (0, 0)
            assert gibbs.selftest_series_launch(kernel) == (0, 0)
        assert gibbs.selftest_series_launch("contrast") == (0, 0)
    for kernel in (-1, 4):
        assert lib.mmg_selftest_series_launch(kernel, C.byref(g), C.byref(c)) == 1 and b"kernel" in lib.mmg_last_error()
    assert lib.mmg_selftest_series_launch(0, None, C.byref(c)) == 1 and lib.mmg_selftest_series_launch(0, C.byref(g), None) == 1


def test_struct_layouts_match_header():
    from mmseq_amd import _lib
    assert C.sizeof(_lib.ProblemDesc) == 72
    assert C.sizeof(_lib.SynthDesc) == 72
    assert C.sizeof(_lib.Config) == 48
    assert C.sizeof(_lib.Timing) == 32
    assert C.sizeof(_lib.ProblemInfo) == 112
    assert C.sizeof(_lib.KeyedIO) == 208
    assert C.sizeof(_lib.BigkPoints) == 160


def test_no_cpu_fallback_without_device():
    from mmseq_amd import gibbs
    from mmseq_amd._lib import MMGError
    if gibbs.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(MMGError) as e:
        gibbs.Problem.from_csr(np.array([0, 1], np.uint64), np.array([0], np.uint32), np.ones(1))
    assert e.value.code == 2 and "no CPU fallback" in str(e.value)
    with pytest.raises(MMGError):
        gibbs.Problem.synthetic(100, 10, 4)
    with pytest.raises(MMGError):
        gibbs.selftest_math(np.ones(4), 0)


def test_argument_validation_happens_before_device_use():
    from mmseq_amd import _lib, gibbs
    from mmseq_amd._lib import MMGError
    with pytest.raises(MMGError) as e:
        gibbs.Problem.from_csr(np.array([0, 2], np.uint64), np.array([0, 7], np.uint32), np.ones(3))
    assert e.value.code == 1          # col index out of range
    with pytest.raises(MMGError) as e:
        gibbs.Problem.from_csr(np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([0.0]))
    assert e.value.code == 1          # l must be > 0 (src/mmseq.cpp:604)
    with pytest.raises(MMGError) as e:
        gibbs.Problem.from_csr(np.array([1, 1], np.uint64), np.array([0], np.uint32), np.ones(1))
    assert e.value.code == 1
    # mmg_selftest_keyed: a part with a count needs every one of its arrays, also on a device that does not exist
    lib = _lib.load()
    x = np.ones(3)
    for device in (-1, 0, 99):
        assert lib.mmg_selftest_keyed(device, None) == 1
        for io in (_lib.KeyedIO(n_math=3, x=x.ctypes.data), _lib.KeyedIO(n_streams=1), _lib.KeyedIO(n_words=-1)):
            assert lib.mmg_selftest_keyed(device, C.byref(io)) == 1, device
    assert lib.mmg_selftest_keyed(-1, C.byref(_lib.KeyedIO())) == 0          # nothing asked, nothing done
    # mmg_selftest_bigk_points: the same rule, and every element inside the domain on which the kernel takes that path
    for device in (-1, 0, 99):
        assert lib.mmg_selftest_bigk_points(device, None) == 1
        for io in (_lib.BigkPoints(n_inv=3, inv_p=x.ctypes.data), _lib.BigkPoints(n_btrs=1), _lib.BigkPoints(n_inv=-1)):
            assert lib.mmg_selftest_bigk_points(device, C.byref(io)) == 1, device
        for n, p, u, slack in ((0, .1, .5, 1), (5, 0., .5, 1), (5, .6, .5, 1), (100, .1, .5, 1), (5, .1, 0., 1), (5, .1, 1., 1), (5, .1, .5, 0),
                               (5, float("nan"), .5, 1), (5, .1, float("nan"), 1)):
            with pytest.raises(MMGError) as e:
                gibbs.selftest_bigk_inversion(n, p, u, slack=slack, device=device)
            assert e.value.code == 1 and "selftest_bigk_points" in str(e.value), (n, p, u, slack)
        for n, p, u, v in ((20, .5, .5, .5), (100, .05, .5, .5), (100, .6, .5, .5), (100, .3, 0., .5), (100, .3, .5, 1.), (100, .3, .5, float("nan"))):
            with pytest.raises(MMGError) as e:
                gibbs.selftest_bigk_btrs(n, p, u, v, device=device)
            assert e.value.code == 1 and "BTRS element 0" in str(e.value), (n, p, u, v)
    assert lib.mmg_selftest_bigk_points(-1, C.byref(_lib.BigkPoints())) == 0


def test_host_instantiation_of_library_math_equals_oracle(orc):
    from mmseq_amd import gibbs
    rng = np.random.default_rng(11)
    x = np.concatenate([np.exp(rng.uniform(-700, 700, 100000)), rng.uniform(-745, 709, 100000),
                        [5e-324, 1e-310, 0.0, 1.0, np.inf]])
    r = gibbs.selftest_math(x, -1)
    assert np.array_equal(r["log"], orc.log_v(x), equal_nan=True)
    assert np.array_equal(r["exp"], orc.exp_v(x), equal_nan=True)
    got = gibbs.selftest_philox([1, 2, 3, 4], [5, 6], -1)
    assert np.array_equal(got[:4], orc.philox([1, 2, 3, 4], [5, 6])) and np.array_equal(got[4:], orc.philox2x32([1, 2], 5))
    for shape in (0.1, 1.0, 9.5):
        ref = np.empty(20000)
        orc.lib().orc_keyed_gamma_v(21, shape, 1.5, 20000, ref)
        assert np.array_equal(gibbs.selftest_gamma(21, shape, 1.5, 20000, -1), ref)
    for nn, p in ((1, 0.4), (25, 0.3), (5000, 0.6)):
        ref = np.empty(20000, np.uint32)
        orc.lib().orc_keyed_binomial_v(8, nn, p, 20000, ref)
        assert np.array_equal(gibbs.selftest_binomial(8, nn, p, 20000, -1), ref)
