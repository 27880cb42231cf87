"""Ownership of the library's device memory, streams and events: every create entry, repeated, gives back what it acquired, and every
acquisition of device memory, a stream or an event that fails (MMG_OPT_FAIL_ALLOC: the v-th one after the option is set fails without
reaching the runtime) leaves an error, no handle and nothing acquired behind -- after which the call still gives what it gave before.
What the library holds is counted exactly by its owners (mmg_selftest_live); device free memory is checked as well."""
import ctypes as C

import numpy as np
import pytest

from mmseq_amd import _lib

MiB = 1 << 20
REPS = 50
# Device free memory after REPS create/destroy cycles of every entry moved by 0 bytes (MI355X).  The runtime sub-allocates small buffers from
# 2 MiB blocks, so free memory can only show leaks of that order; the live counts of the owners are the exact check.
TOL = 2 * MiB
ERR_HIP = 3   # MMG_ERR_HIP


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def env(gpu):
    lib = _lib.load()
    # the HIP runtime this process already has (the one libmmgibbs.so is bound to; a second copy cannot share the device)
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line))
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_mem():
        assert hip.hipDeviceSynchronize() == 0
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    def live():
        c = np.zeros(3, np.int64)
        _lib.check(lib.mmg_selftest_live(_p(c)))
        return tuple(int(x) for x in c)   # device buffers, streams, events

    yield lib, free_mem, live
    lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)


def _problem_inputs(seed, kmult, layout):
    rng = np.random.default_rng(seed)
    m, n = 3000, 400
    rows = []
    for _ in range(m):
        c = int(rng.integers(0, n))
        rows.append(np.unique((c + rng.integers(-20, 21, int(rng.integers(1, 6)))) % n).astype(np.uint32))
    rp = np.zeros(m + 1, np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.uint32)
    k = None
    if kmult:   # multiplicities: rows that expand (2, 3), stay on the multiplicity path (50) or take the conditional-binomial chain (5000)
        k = rng.choice(np.array([1, 1, 1, 2, 3, 50, 5000], np.uint32), m).astype(np.uint32)
    l = rng.uniform(0.5, 2.0, n)
    arrays = dict(rp=rp, col=col, k=k, l=l)
    d = _lib.ProblemDesc(m=m, n=n, row_ptr=_p(rp), col_idx=_p(col), k=_p(k) if k is not None else None, l=_p(l), row_id_base=0,
                         layout=layout, tx_order=None)
    return d, arrays


def _download(lib, p):
    info = _lib.ProblemInfo()
    _lib.check(lib.mmg_problem_info_get(p, C.byref(info)))
    rp = np.zeros(info.m + 1, np.uint64)
    col = np.zeros(max(info.nnz, 1), np.uint32)
    k = np.zeros(max(info.m, 1), np.uint32)
    _lib.check(lib.mmg_problem_download(p, _p(rp), _p(col), _p(k)))
    return (info.m, info.nnz, info.n_tiles, info.device_bytes, info.sample_kernel, info.tx_renumbered), rp, col, k


def _same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a, b)
    return a == b


class Entry:
    """create(out) -> rc; result(handle) -> what the handle gives; destroy(handle)."""

    def __init__(self, name, create, destroy, result):
        self.name, self.create, self.destroy, self.result = name, create, destroy, result


@pytest.fixture(scope="module")
def entries(env):
    lib = env[0]
    keep = []   # host arrays the descriptors point at

    def problem(d, arrays, derive=None):
        keep.append((d, arrays))

        def create(out):
            if derive is not None:
                lib.mmg_selftest_option(_lib.OPT_DERIVE_ORDER, derive)
            try:
                return lib.mmg_problem_create(C.byref(d), 0, C.byref(out))
            finally:
                lib.mmg_selftest_option(_lib.OPT_DERIVE_ORDER, -1)
        return create

    canon_d, canon_a = _problem_inputs(1, True, _lib.LAYOUT_CANONICAL)
    keep_d, keep_a = _problem_inputs(2, False, _lib.LAYOUT_KEEP_ROWS)
    synth = _lib.SynthDesc(seed=7, rows=20000, row0=0, n=2000, avg_hits=3.0, uniform=0, sorted=1, mapped_reads=0, far_fraction=0.02,
                           gene_size=0, far_family=0)
    keep.append(synth)

    # long-lived parents of the handles that need one
    parent = C.c_void_p()
    _lib.check(problem(canon_d, canon_a)(parent))
    sparent = C.c_void_p()
    _lib.check(lib.mmg_problem_create_synthetic(C.byref(synth), 0, C.byref(sparent)))
    info = _lib.ProblemInfo()
    _lib.check(lib.mmg_problem_info_get(parent, C.byref(info)))
    n = info.n
    mu0 = np.zeros(n)
    _lib.check(lib.mmg_problem_start_values(parent, _p(mu0), None))
    cfg = _lib.Config(alpha=0.1, beta=0.1, seed=11, n_chains=2, chain_base=0, gibbs_iter=8, trace_len=8, keep_trace=1, timing=0)
    chain = C.c_void_p()
    _lib.check(lib.mmg_sampler_create(parent, C.byref(cfg), _p(mu0), C.byref(chain)))
    _lib.check(lib.mmg_sampler_run(chain, 8))
    _lib.check(lib.mmg_sampler_sync(chain))
    sdesc = _lib.SummaryDesc(chain=0, n_virtual=0, n_identical=0, n_genes=0, n_percentiles=0)
    keep.extend([mu0, cfg, sdesc])

    def problem_result(p):
        return _download(lib, p)

    def sampler_create(out):
        return lib.mmg_sampler_create(parent, C.byref(cfg), _p(mu0), C.byref(out))

    def sampler_result(s):
        _lib.check(lib.mmg_sampler_run(s, 4))
        mu = np.zeros(n)
        _lib.check(lib.mmg_sampler_get_mu(s, 1, _p(mu)))
        tr = np.zeros(8 * n)
        _lib.check(lib.mmg_sampler_get_trace(s, 0, _p(tr)))
        return mu, tr

    def summary_result(q):
        lm, var, tau = np.zeros(n), np.zeros(n), np.zeros(n)
        rc = np.zeros(n, np.int32)
        _lib.check(lib.mmg_summary_get(q, 0, _p(lm), _p(var), _p(tau), _p(rc), None))
        return lm, var, tau, rc

    def em_create(out):
        ll = C.c_double()
        rc = lib.mmg_em_create(parent, _p(mu0), C.byref(out), C.byref(ll))
        return rc

    def em_result(e):
        ll = C.c_double()
        _lib.check(lib.mmg_em_step(e, C.byref(ll)))
        mu = np.zeros(n)
        _lib.check(lib.mmg_em_get_mu(e, _p(mu)))
        return ll.value, mu

    rng = np.random.default_rng(5)
    S, Cn, N = 3, 40, 32
    obs = np.ones((Cn, S), np.uint8)
    traces = [rng.gamma(2.0, 1.0, (N, Cn)) for _ in range(S)]
    keep.extend([obs, traces])

    def collapse_create(out):
        return lib.mmg_collapse_create(0, S, Cn, N, _p(obs), C.byref(out))

    def collapse_result(h):
        for s in range(S):
            _lib.check(lib.mmg_collapse_set_sample(h, s, _p(traces[s])))
        _lib.check(lib.mmg_collapse_correlate(h))
        rm = np.zeros(Cn)
        _lib.check(lib.mmg_collapse_row_max(h, _p(rm)))
        return rm

    F, Nd = 64, 6
    y = rng.normal(2, 1, (F, Nd))
    e = rng.uniform(0.05, 0.5, (F, Nd))
    M = np.ones((Nd, 1))
    P0 = np.ones((Nd, 1))
    P1 = np.array([[0.5], [0.5], [0.5], [-0.5], [-0.5], [-0.5]])
    cls = np.array([[0, 0]] * 3 + [[0, 1]] * 3, np.int32)
    keep.extend([y, e, M, P0, P1, cls])

    def diff_create(out):
        return lib.mmg_diff_create(0, F, Nd, _p(y), _p(e), 1, _p(M), 1, _p(P0), 1, _p(P1), _p(cls), 1.4, 2.0, 0.5, 0, 99, C.byref(out))

    def diff_result(h):
        _lib.check(lib.mmg_diff_burnin(h, 1024))
        _lib.check(lib.mmg_diff_sample(h, 512))
        gamma, logitp = np.zeros(F), np.zeros(F)
        _lib.check(lib.mmg_diff_get_results(h, _p(gamma), _p(logitp), None, None, None))
        return gamma, logitp

    sh_lo, sh_hi = 1000, 2400
    out = [
        Entry("canonical_multiplicities", problem(canon_d, canon_a), lib.mmg_problem_destroy, problem_result),
        Entry("canonical_derived_order", problem(*_problem_inputs(3, False, _lib.LAYOUT_CANONICAL), derive=1), lib.mmg_problem_destroy, problem_result),
        Entry("keep_rows", problem(keep_d, keep_a), lib.mmg_problem_destroy, problem_result),
        Entry("shard", lambda o: lib.mmg_problem_shard(parent, sh_lo, sh_hi, 0, C.byref(o)), lib.mmg_problem_destroy, problem_result),
        Entry("synthetic", lambda o: lib.mmg_problem_create_synthetic(C.byref(synth), 0, C.byref(o)), lib.mmg_problem_destroy, problem_result),
        Entry("sampler_trace", sampler_create, lib.mmg_sampler_destroy, sampler_result),
        Entry("summary", lambda o: lib.mmg_summary_create(chain, C.byref(sdesc), C.byref(o)), lib.mmg_summary_destroy, summary_result),
        Entry("em", em_create, lib.mmg_em_destroy, em_result),
        Entry("collapse", collapse_create, lib.mmg_collapse_destroy, collapse_result),
        Entry("diff", diff_create, lib.mmg_diff_destroy, diff_result),
    ]
    yield out, (lib, sparent)
    lib.mmg_sampler_destroy(chain)
    lib.mmg_problem_destroy(parent)
    lib.mmg_problem_destroy(sparent)


def _names():
    return ["canonical_multiplicities", "canonical_derived_order", "keep_rows", "shard", "synthetic", "sampler_trace", "summary", "em",
            "collapse", "diff"]


def _entry(entries, name):
    return next(e for e in entries[0] if e.name == name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names())
def test_create_destroy_gives_back_what_it_acquired(env, entries, name):
    lib, free_mem, live = env
    ent = _entry(entries, name)
    h = C.c_void_p()
    _lib.check(ent.create(h))   # warm-up: code objects, runtime pools, a problem's lazily built caches
    ent.destroy(h)
    base, base_live = free_mem(), live()
    for _ in range(REPS):
        h = C.c_void_p()
        _lib.check(ent.create(h))
        assert live() != base_live
        ent.destroy(h)
        assert live() == base_live
    drift = base - free_mem()
    print("%s: %d bytes after %d create/destroy" % (name, drift, REPS))
    assert drift <= TOL


@pytest.mark.gpu
def test_shard_bounds_timed_gives_back_what_it_acquired(env, entries):
    lib, free_mem, live = env
    _, sparent = entries[1]
    info = _lib.ProblemInfo()
    _lib.check(lib.mmg_problem_info_get(sparent, C.byref(info)))
    mu = np.full(info.n, 1.0 / info.n)
    bounds = np.zeros(3, np.uint64)
    _lib.check(lib.mmg_problem_shard_bounds_timed(sparent, _p(mu), 2, _p(bounds)))
    base, base_live = free_mem(), live()
    for _ in range(REPS):
        _lib.check(lib.mmg_problem_shard_bounds_timed(sparent, _p(mu), 2, _p(bounds)))
        assert live() == base_live
    drift = base - free_mem()
    print("shard_bounds_timed: %d bytes after %d calls" % (drift, REPS))
    assert drift <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names())
def test_every_failed_acquisition_is_released(env, entries, name):
    lib, free_mem, live = env
    ent = _entry(entries, name)
    h = C.c_void_p()
    _lib.check(ent.create(h))
    before = ent.result(h)
    ent.destroy(h)
    base, base_live = free_mem(), live()
    v = 0
    try:
        while True:
            _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
            h = C.c_void_p()
            rc = ent.create(h)
            if rc == 0:
                break
            msg = lib.mmg_last_error().decode()
            assert rc == ERR_HIP, (v, rc, msg)
            assert msg, v
            assert not h.value, v
            assert live() == base_live, (v, msg)
            assert base - free_mem() <= TOL, v
            v += 1
            assert v < 10000
    finally:
        lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
    assert v > 0   # the entry acquires something
    ent.destroy(h)
    assert live() == base_live
    h = C.c_void_p()
    _lib.check(ent.create(h))
    after = ent.result(h)
    ent.destroy(h)
    assert _same(before, after)
    assert live() == base_live
    assert base - free_mem() <= TOL
    print("%s: %d acquisitions can fail" % (name, v))


@pytest.mark.gpu
def test_shard_bounds_timed_failed_acquisitions(env, entries):
    lib, free_mem, live = env
    _, sparent = entries[1]
    info = _lib.ProblemInfo()
    _lib.check(lib.mmg_problem_info_get(sparent, C.byref(info)))
    mu = np.full(info.n, 1.0 / info.n)
    bounds = np.zeros(3, np.uint64)
    _lib.check(lib.mmg_problem_shard_bounds_timed(sparent, _p(mu), 2, _p(bounds)))
    base, base_live = free_mem(), live()
    v = 0
    try:
        while True:
            _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
            rc = lib.mmg_problem_shard_bounds_timed(sparent, _p(mu), 2, _p(bounds))
            if rc == 0:
                break
            assert rc == ERR_HIP and lib.mmg_last_error().decode(), v
            assert live() == base_live, v
            assert base - free_mem() <= TOL, v
            v += 1
            assert v < 10000
    finally:
        lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
    assert v > 0
    _lib.check(lib.mmg_problem_shard_bounds_timed(sparent, _p(mu), 2, _p(bounds)))
    assert live() == base_live
    assert bounds[0] == 0 and bounds[2] == info.m and bounds[0] <= bounds[1] <= bounds[2]


def _pool(lib, s):
    pool, free, pending = C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.mmg_selftest_sampler_events(s, C.byref(pool), C.byref(free), C.byref(pending)))
    return pool.value, free.value, pending.value


@pytest.mark.gpu
@pytest.mark.parametrize("fail_at", [0, 1, 2])
def test_timed_sampler_event_pool_failure(env, entries, fail_at):
    """A timed sample() takes its events from a pool and creates one whenever the free list is empty -- as it is after every
    sample() + update() here, with nothing harvested in between.  So in every cycle the fail_at-th event creation of sample() fails:
    sample() reports it, every pool index it already held is back on the free list (pool == free + pending), and the chain runs on."""
    lib, _, live = env
    ent = _entry(entries, "canonical_multiplicities")
    p = C.c_void_p()
    _lib.check(ent.create(p))
    try:
        info = _lib.ProblemInfo()
        _lib.check(lib.mmg_problem_info_get(p, C.byref(info)))
        mu0 = np.zeros(info.n)
        _lib.check(lib.mmg_problem_start_values(p, _p(mu0), None))
        cfg = _lib.Config(alpha=0.1, beta=0.1, seed=3, n_chains=2, chain_base=0, gibbs_iter=16, trace_len=16, keep_trace=0, timing=1)
        base_live = live()
        s = C.c_void_p()
        _lib.check(lib.mmg_sampler_create(p, C.byref(cfg), _p(mu0), C.byref(s)))
        created = live()
        try:
            failed = 0
            for cycle in range(4):
                assert _pool(lib, s)[1] == 0, cycle   # (the free list is empty: the next ev_get creates)
                _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, fail_at))
                rc = lib.mmg_sampler_sample(s)
                _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1))
                pool, free, pending = _pool(lib, s)
                assert pool == free + pending, (cycle, pool, free, pending)
                assert live()[2] == created[2] + pool
                if rc != 0:   # (fail_at = 2 fails only a sample() with a side-stream launch: the third event)
                    assert rc == ERR_HIP and lib.mmg_last_error().decode()
                    failed += 1
                    _lib.check(lib.mmg_sampler_sample(s))
                _lib.check(lib.mmg_sampler_update(s))
                pool, free, pending = _pool(lib, s)
                assert pool == free + pending, (cycle, pool, free, pending)
            assert failed == 4 or (fail_at == 2 and failed == 0)
            print("fail_at %d: %d failed sample() calls, pool %d" % (fail_at, failed, _pool(lib, s)[0]))
            _lib.check(lib.mmg_sampler_run(s, 12))
            _lib.check(lib.mmg_sampler_sync(s))
            t = _lib.Timing()
            _lib.check(lib.mmg_sampler_get_timing(s, C.byref(t)))
            assert t.sample_launches == 16 and t.update_launches == 16
            pool, free, pending = _pool(lib, s)
            assert pending == 0 and free == pool
            it = C.c_int()
            _lib.check(lib.mmg_sampler_iteration(s, C.byref(it)))
            assert it.value == 16
        finally:
            lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
            lib.mmg_sampler_destroy(s)
        assert live() == base_live
    finally:
        lib.mmg_problem_destroy(p)


@pytest.mark.gpu
def test_chain_indices_beyond_the_gamma_streams_24_bits_are_refused(env, gpu):
    """mmg_sampler_create: chain_base >= 0 and chain_base + n_chains <= 2^24 (MMG_MAX_CHAINS).  The key of K2's Gamma stream holds 24 bits of
    the chain index, the row stream's all 32: chain 2^24 would redraw mu from chain 0's uniforms while drawing rows of its own
    (tests/test_key_space.py::test_gamma_stream_sees_24_bits_of_the_chain).  The refusal comes before anything is acquired."""
    from mmseq_amd._lib import MMGError
    lib, free_mem, live = env
    prob = gpu.Problem.synthetic(2000, 100, 4, seed=3)
    mu0, _ = prob.start_values()
    base_live = live()
    for base, chains in ((-1, 1), (-2 ** 31, 1), (1 << 24, 1), ((1 << 24) - 2, 3), ((1 << 24) - 1, 2), (2 ** 31 - 1, 2)):
        with pytest.raises(MMGError) as e:
            gpu.Sampler(prob, mu0, n_chains=chains, chain_base=base, gibbs_iter=4, trace_len=4)
        assert e.value.code == 1 and "16777216" in str(e.value) and "24 bits" in str(e.value), (base, chains)
        assert live() == base_live
    for base, chains in (((1 << 24) - 3, 3), ((1 << 24) - 1, 1), (0, 3)):
        s = gpu.Sampler(prob, mu0, n_chains=chains, chain_base=base, gibbs_iter=4, trace_len=4)
        s.run(4)
        assert np.isfinite(s.mu(chains - 1)).all()
        s.close()
    assert live() == base_live
    prob.close()
