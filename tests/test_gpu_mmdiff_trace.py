"""mmdiff's traces on the device against the restatement (tests/mmdiff_trace_ref.py): the rows the ABI hands out, `==` for `==`; the
tuning rows and the pseudopriors; results and memory with and without tracing; a sink that stops the run; and the CLI's trace
directory byte for byte.  Features are independent chains keyed by their index, so one restatement of 130 features serves every
smaller feature count as its first F columns."""
import functools
import os
import subprocess

import numpy as np
import pytest

import mmdiff_ref as R
import mmdiff_trace_ref as TR
from test_gpu_mmdiff import MMDIFF, write_tables

FMAX, N = 130, 4


def data(seed=31):
    rng = np.random.default_rng(seed)
    y = rng.normal(2, 1, (FMAX, 1)) + rng.normal(0, 0.3, (FMAX, N))
    y[:26, :2] += 1.5
    e = rng.uniform(0.05, 0.5, (FMAX, N))
    return y, e


def design(name):
    """(M, P0, P1, C, fixalpha): -de 2 2; one covariate with a nil P0 (a constant column); -de 2 2 with -fixalpha."""
    if name == "covariate":
        M = np.array([[0.3], [1.1], [-0.4], [0.9]])
        C = np.array([[0, 0], [0, 0], [0, 1], [0, 1]])
        return M, np.ones((N, 1)), np.where(C[:, 1:] == 0, 0.5, -0.5), C, False
    return R.de_design([2, 2]) + (name == "fixalpha",)


@functools.lru_cache(maxsize=None)
def ref_thinned(name):
    """Burn-in 1100 recorded every 7th, 600 sampling iterations every 5th, no tuning: neither interval divides the 512 iterations of
    a launch, and rows lie on both sides of the launch edges at 512 and 1024."""
    y, e = data()
    M, P0, P1, C, fixalpha = design(name)
    return TR.run_traced(y, e, M, P0, P1, C, 1100, 600, tune=False, every_burnin=7, every_sample=5, fixalpha=fixalpha, seed=77)


@functools.lru_cache(maxsize=None)
def ref_every():
    """Every iteration a row: burn-in 1024 (two full launches, both buffers), three tuning batches, 130 sampling iterations."""
    y, e = data()
    M, P0, P1, C, _ = design("de22")
    return TR.run_traced(y, e, M, P0, P1, C, 1024, 130, batches=3, every_burnin=1, every_sample=1, seed=78)


def make(name, F, seed):
    from mmseq_amd.diff import Diff
    y, e = data()
    M, P0, P1, C, fixalpha = design(name)
    return Diff(y[:F], e[:F], M, P0, P1, C, fixalpha=fixalpha, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["de22", "covariate", "fixalpha"])
@pytest.mark.parametrize("F", [1, 64, 65, 130])
def test_thinned_rows_equal_the_restatement(gpu, name, F):
    b, pseudo = ref_thinned(name)
    d = make(name, F, 77)
    assert d.trace_names() == b.names()
    calls = []
    kept = ([], [])

    def sink(phase, first, rows):
        calls.append((phase, first, rows.shape[0]))
        kept[phase].append(rows.copy())
        return 0

    d.open_traces(7, 5, sink)
    d.burnin(1100)
    got_pseudo = d.pseudo()
    d.sample(600)
    burn, samp = np.concatenate(kept[0]), np.concatenate(kept[1])
    # 1100 = 512 + 512 + 76 iterations: rows 0..73 | 74..146 | 147..157; 600 = 512 + 88: rows 0..102 | 103..119
    assert calls == [(0, 0, 74), (0, 74, 73), (0, 147, 11), (1, 0, 103), (1, 103, 17)]
    assert burn.shape == (158, len(b.names()) - 1, F) and samp.shape == (120, len(b.names()), F)
    assert np.array_equal(burn, b.stacked(0)[:, :, :F])
    assert np.array_equal(samp, b.stacked(1)[:, :, :F])
    assert np.array_equal(got_pseudo, pseudo[:, :F])
    d.close()


@pytest.mark.gpu
def test_every_iteration_and_tuning_rows_equal_the_restatement(gpu):
    b, pseudo = ref_every()
    for F in (1, 64, 65, 130):
        d = make("de22", F, 78)
        d.open_traces(1, 1)
        d.burnin(1024)
        assert np.array_equal(d.pseudo(), pseudo[:, :F])
        tune_rows = []
        for batch in range(3):
            if batch > 0:
                tune_rows.append(d.tune_state())
            d.tune_batch()
        d.sample(130)
        burn, samp = d.traces()
        assert burn.shape == (1024, 13, F) and samp.shape == (130, 14, F)
        assert np.array_equal(burn, b.stacked(0)[:, :, :F])
        assert np.array_equal(samp, b.stacked(1)[:, :, :F])
        assert set(np.unique(samp[:, -1])) <= {0.0, 1.0}
        assert len(b.tune_rows) == 2
        for (lo, lp), (wlo, wlp) in zip(tune_rows, b.tune_rows):
            assert np.array_equal(lo, wlo[:F]) and np.array_equal(lp, wlp[:F])
        if F >= 65:      # a frozen feature keeps its row: some features are tuned before batch 2 here
            assert b.tuned[:F].any() and not b.tuned[:F].all()
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_rows", [1, 5])
def test_launches_shortened_to_a_small_buffer_record_the_same_rows(gpu, max_rows):
    """What a default-size run does (64 MiB hold fewer rows than a full launch has), here with the buffer cut to max_rows rows by the
    self-test option: more and shorter launches, the same rows and the same chain."""
    from mmseq_amd import _lib
    b, _ = ref_thinned("de22")
    lib = _lib.load()
    F = 130
    plain = make("de22", F, 77)
    plain.burnin(1100)
    plain.sample(600)
    want = plain.results()
    base = plain.device_bytes()
    plain.close()
    _lib.check(lib.mmg_selftest_option(_lib.OPT_DIFF_TRACE_ROWS, max_rows))
    try:
        d = make("de22", F, 77)
        calls, kept = [], ([], [])

        def sink(phase, first, rows):
            calls.append((phase, first, rows.shape[0]))
            kept[phase].append(rows.copy())
            return 0

        d.open_traces(7, 5, sink)
    finally:
        lib.mmg_selftest_option(_lib.OPT_DIFF_TRACE_ROWS, -1)
    assert d.device_bytes() == base + 2 * max_rows * 14 * F * 8 + 2 * 496
    d.burnin(1100)
    d.sample(600)
    assert all(n <= max_rows for _, _, n in calls) and len(calls) >= (158 + 120) // max_rows
    for phase, total in ((0, 158), (1, 120)):
        mine = [(f, n) for ph, f, n in calls if ph == phase]
        assert [f for f, _ in mine] == [sum(n for _, n in mine[:i]) for i in range(len(mine))] and sum(n for _, n in mine) == total
    assert np.array_equal(np.concatenate(kept[0]), b.stacked(0)) and np.array_equal(np.concatenate(kept[1]), b.stacked(1))
    got = d.results()
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [65, 130])
def test_results_and_memory_with_and_without_tracing(gpu, F):
    plain = make("covariate", F, 9)
    base = plain.device_bytes()
    plain.burnin(1024)
    plain.tune_batch()
    plain.sample(600)
    want = plain.results()
    assert plain.device_bytes() == base                       # nothing is allocated later
    traced = make("covariate", F, 9)
    assert traced.device_bytes() == base
    P = len(traced.trace_names())
    traced.open_traces(7, 5)
    rows = min(-(-512 // 5), max(1, (64 << 20) // (P * F * 8)))
    assert rows == 103 and traced.device_bytes() == base + 2 * rows * P * F * 8 + 2 * 496
    traced.burnin(1024)
    traced.tune_batch()
    traced.sample(600)
    got = traced.results()
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert traced.traces()[1].shape == (120, P, F)
    plain.close()
    traced.close()


@pytest.mark.gpu
def test_trace_open_arguments_and_a_sink_that_stops_the_run(gpu):
    from mmseq_amd._lib import MMGError
    d = make("de22", 65, 3)
    for eb, es in ((0, 1), (1, 0)):
        with pytest.raises(MMGError) as ex:
            d.open_traces(eb, es)
        assert ex.value.code == 1 and "at least 1" in str(ex.value)
    calls = []

    def sink(phase, first, rows):
        calls.append((phase, first, rows.shape[0]))
        return 7 if len(calls) == 2 else 0

    d.open_traces(8, 8, sink)
    with pytest.raises(MMGError) as ex:
        d.burnin(2048)
    assert ex.value.code == 5 and "the trace sink returned 7" in str(ex.value)
    assert calls == [(0, 0, 64), (0, 64, 64)]
    with pytest.raises(MMGError) as ex:
        d.burnin(1024)
    assert ex.value.code == 4
    d.close()                                                  # an error path: the handle goes cleanly
    # an exception in the caller's sink stops the run and is raised from the entry that was running; traces() needs kept rows
    d = make("de22", 65, 3)

    def broken(phase, first, rows):
        raise ValueError("sink broke at row %d" % first)

    d.open_traces(8, 8, broken)
    with pytest.raises(ValueError, match="sink broke at row 0"):
        d.burnin(1024)
    with pytest.raises(RuntimeError, match="without a sink"):
        d.traces()
    d.close()
    late = make("de22", 1, 3)
    late.burnin(1024)
    with pytest.raises(MMGError) as ex:
        late.open_traces(1, 1)
    assert ex.value.code == 1 and "after the burn-in" in str(ex.value)
    late.close()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def cli_inputs(tmp_path):
    rng = np.random.default_rng(400)
    y = rng.normal(2, 1, (FMAX, 1)) + rng.normal(0, 0.3, (FMAX, N))
    e = rng.uniform(0.4, 0.6, (FMAX, N))
    uh = rng.integers(1, 5, (FMAX, N))
    return write_tables(tmp_path, y, e, uh)


def restated_files(files, burnin, iters, tune):
    tabs = [R.read_table(f) for f in files]
    y = np.stack([t[1] for t in tabs], 1)
    e = np.stack([t[2] for t in tabs], 1)
    uh = np.stack([t[3] for t in tabs], 1)
    y, factors = R.normalise(y, uh, max(0.2, float(N - N * N // 160) / float(N)))
    assert factors is not None                                 # 130 features: the CLI normalises
    M, P0, P1, C = R.de_design([2, 2])
    b, pseudo = TR.run_traced(y, e, M, P0, P1, C, burnin, iters, tune=tune, seed=1234)
    return b, TR.files_of(b, pseudo)


@pytest.mark.gpu
@pytest.mark.parametrize("args,tune", [(["-burnin", "1024", "-iter", "1024", "-notune"], False), (["-burnin", "3072", "-iter", "2048"], True)])
def test_cli_trace_directory_is_byte_identical_to_the_restatement(gpu, tmp_path, args, tune):
    """The device side of either case takes seconds.  The tuned case's restatement is the slow part: 130 features tune for some tens of
    batches (the last few features take long), each 128 numpy iterations of about 10 ms."""
    files = cli_inputs(tmp_path)
    d = tmp_path / "traces"
    run = lambda a: subprocess.run([MMDIFF] + a + ["-de", "2", "2"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    plain = run(args)
    traced = run(args + ["-traces", str(d)])
    assert plain.returncode == 0 and traced.returncode == 0, traced.stderr.decode()[-2000:]
    assert traced.stdout == plain.stdout and len(plain.stdout) > 0
    b, want = restated_files(files, int(args[1]), int(args[3]), tune)
    assert set(os.listdir(d)) == set(want)
    for name in sorted(want):
        got = (d / name).read_bytes()
        assert got == want[name].encode(), name
    assert want["alpha0-burnin"].count("\n") == 1024 and want["gamma"].count("\n") == 1024
    if tune:
        assert b.batches >= 2 and want["logitp"].count("\n") == b.batches - 1 and want["meanLO"].count("\n") == b.batches - 1 + 1024
        assert ("sampling after %d tuning batches" % b.batches).encode() in traced.stderr
    else:
        assert want["logitp"] == "" and want["meanLO"] == "\n" * 1024
