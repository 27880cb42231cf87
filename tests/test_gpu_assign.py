"""mmg_assign_* on the device (mmseq_amd.Assign, mmseq -assign) against tests/assign_ref.py: bit identity at the kernel's edges, the
sampler's trace taken on the device, reruns and the memory formula, the error codes, the CLI's files, and a statistical check that the
probabilities are those of what the sampler draws."""
import gzip
import os

import numpy as np
import pytest

from oracle import host_oracle as H
from test_cli import dataset, run
import assign_ref as R

pytestmark = pytest.mark.gpu

HITS_PER_WAVE = 256           # assign_kernels.h: ASG_HITS_PER_WAVE
SCRATCH_BYTES = 64 << 20      # ASG_SCRATCH_BYTES


def _trace(rng, n_tx, S):
    return np.exp(rng.normal(0.0, 3.0, (n_tx, S)))


def _csr(rng, lengths, n_tx):
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    ci = np.concatenate([rng.choice(n_tx, l, replace=False) for l in lengths] + [np.empty(0, np.int64)]).astype(np.uint32)
    return rp, ci


def _formula(n_rows, hits, n_tx=0, T=0, count=0, cap=0):
    """mmg_assign_device_bytes as include/mmgibbs.h states it (T = 0: before the first run)"""
    b = 8 * (n_rows + 1) + 12 * max(hits, 1)
    if T:
        pad = (count + 63) // 64 * 64
        W = min(-(-hits // HITS_PER_WAVE), SCRATCH_BYTES // (8 * pad))
        if cap:
            W = min(W, cap)
        b += 8 * n_tx * T + 8 * max(W, 1) * pad
    return b


@pytest.fixture
def option(gpu):
    from mmseq_amd import _lib
    lib = _lib.load()
    yield lambda v: lib.mmg_selftest_option(_lib.OPT_ASSIGN_WAVES, v)
    lib.mmg_selftest_option(_lib.OPT_ASSIGN_WAVES, -1)


# rows of 1, 2, 8, 9 hits (registers / scratch slice), 63, 64, 65 and 5 000; empty rows first, last and in the middle
EDGE_LENGTHS = [0, 1, 2, 8, 9, 0, 63, 64, 65, 5000, 3, 0]


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130, 1024])
def test_bit_identity_at_the_edges(gpu, S):
    from mmseq_amd import Assign
    rng = np.random.default_rng(10 + S)
    n_tx = 5003
    rp, ci = _csr(rng, EDGE_LENGTHS, n_tx)
    tr = _trace(rng, n_tx, S)
    with Assign(rp, ci, n_tx) as a:
        assert a.device_bytes() == _formula(len(EDGE_LENGTHS), ci.size)
        a.run_trace(tr)
        got = a.probabilities()
        assert a.device_bytes() == _formula(len(EDGE_LENGTHS), ci.size, n_tx, S, S)
        a.run_trace(tr)                                     # the same handle again: the same bits
        assert np.array_equal(a.probabilities(), got)
    want = R.assign_ref(rp, ci, tr)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("n_tx", [1, 70000])
def test_transcript_counts(gpu, n_tx):
    from mmseq_amd import Assign
    rng = np.random.default_rng(n_tx)
    S = 65
    if n_tx == 1:
        rp, ci = np.array([0, 1, 1, 3, 12], np.uint64), np.zeros(12, np.uint32)     # the one column, also repeated inside a row
    else:
        rp, ci = _csr(rng, [3, 1, 9, 0, 70, 8], n_tx)
        ci[0], ci[-1] = n_tx - 1, 0
    tr = _trace(rng, n_tx, S)
    with Assign(rp, ci, n_tx) as a:
        a.run_trace(tr)
        assert np.array_equal(a.probabilities(), R.assign_ref(rp, ci, tr))


@pytest.mark.parametrize("n_rows", [1, HITS_PER_WAVE - 1, HITS_PER_WAVE, HITS_PER_WAVE + 1])
def test_row_counts_around_one_wave(gpu, n_rows):
    """rows of one and two hits: a wave owns the rows that start in its 256 hit offsets"""
    from mmseq_amd import Assign
    rng = np.random.default_rng(n_rows)
    n_tx, S = 40, 70
    for lengths in (np.ones(n_rows, np.int64), rng.integers(1, 3, n_rows)):
        rp, ci = _csr(rng, lengths, n_tx)
        tr = _trace(rng, n_tx, S)
        with Assign(rp, ci, n_tx) as a:
            a.run_trace(tr)
            assert np.array_equal(a.probabilities(), R.assign_ref(rp, ci, tr))


def test_scratch_chunks_and_sample_sub_range(gpu, option):
    """MMG_OPT_ASSIGN_WAVES = 2 on 9 waves' worth of hits: five launches that share two scratch slices; rows on both paths; the
    samples [3, 73) of 130"""
    from mmseq_amd import Assign
    rng = np.random.default_rng(5)
    n_tx, S = 500, 130
    lengths = rng.integers(0, 14, 260)
    lengths[100] = 400
    rp, ci = _csr(rng, lengths, n_tx)
    assert 8 * HITS_PER_WAVE < ci.size <= 9 * HITS_PER_WAVE
    tr = _trace(rng, n_tx, S)
    with Assign(rp, ci, n_tx) as a:
        a.run_trace(tr, first=3, count=70)
        whole = a.probabilities()
        assert a.device_bytes() == _formula(lengths.size, ci.size, n_tx, S, 70)
        assert option(2) == 0
        a.run_trace(tr, first=3, count=70)
        assert a.device_bytes() == _formula(lengths.size, ci.size, n_tx, S, 70, cap=2)
        chunked = a.probabilities()
    want = R.assign_ref(rp, ci, tr, first=3, count=70)
    assert np.array_equal(whole, want) and np.array_equal(chunked, want)


def test_degenerate_samples(gpu):
    """a sample where every mu of the row is 0 and one where the sum is inf, on a row of 2 hits and on one of 9"""
    from mmseq_amd import Assign
    rng = np.random.default_rng(6)
    n_tx, S = 12, 66
    rp, ci = np.array([0, 2, 11, 12], np.uint64), np.arange(12, dtype=np.uint32)
    tr = _trace(rng, n_tx, S)
    tr[:, 5] = 0.0
    tr[:, 64] = 1e308
    tr[3, 9] = np.inf
    with Assign(rp, ci, n_tx) as a:
        a.run_trace(tr)
        got = a.probabilities()
    assert np.array_equal(got, R.assign_ref(rp, ci, tr)) and got[11] == 1.0
    with Assign(rp, ci, n_tx) as a:
        a.run_trace(np.zeros((n_tx, 3)))
        got = a.probabilities()
    assert np.array_equal(got, R.assign_ref(rp, ci, np.zeros((n_tx, 3))))
    assert abs(got[0] - 0.5) < 1e-15 and abs(got[2] - 1.0 / 9.0) < 1e-15


def test_sampler_trace_on_device_equals_host_trace(gpu, orc):
    """2 000 synthetic rows, 256 iterations, two chains, transcripts renumbered on the device: run() on the sampler's trace equals
    run_trace() on Sampler.trace(), and both the restated specification"""
    from mmseq_amd import Assign
    from mmseq_amd._lib import MMGError
    T = 300
    q, _ = orc.synth_problem(R=2000, T=T, avg_hits=4, seed=99, sort=False)
    order = np.random.default_rng(7).permutation(T).astype(np.uint64)
    prob = gpu.Problem.from_csr(q.row_ptr, q.col_idx, q.l, tx_order=order)
    mu0, _ = prob.start_values()
    smp = gpu.Sampler(prob, mu0, seed=7, n_chains=2, gibbs_iter=256, trace_len=256)
    with Assign(q.row_ptr, q.col_idx, T) as a:
        with pytest.raises(MMGError) as e:
            a.run(smp)                                      # nothing kept yet
        assert e.value.code == 4
        smp.run(256)
        for chain, first, count in ((0, 0, None), (1, 0, None), (1, 5, 200)):
            a.run(smp, chain=chain, first=first, count=count)
            on_device = a.probabilities()
            tr = smp.trace(chain)
            a.run_trace(tr, first=first, count=count)
            assert np.array_equal(on_device, a.probabilities())
            assert np.array_equal(on_device, R.assign_ref(q.row_ptr, q.col_idx, tr, first=first, count=count))
        k = np.random.default_rng(8).integers(1, 9, 2000)
        assert np.array_equal(a.expected_hits(k), R.expected_hits(q.row_ptr, q.col_idx, a.probabilities(), T, k))
    smp.close()
    prob.close()


def test_errors_return_their_codes(gpu):
    from mmseq_amd import Assign
    from mmseq_amd._lib import MMGError
    rp, ci = np.array([0, 2, 3], np.uint64), np.array([0, 1, 2], np.uint32)
    with pytest.raises(MMGError) as e:
        Assign(rp, ci, 2)                                   # column 2 with n_tx = 2
    assert e.value.code == 1
    with pytest.raises(MMGError) as e:
        Assign(np.array([0, 3, 2, 3], np.uint64), ci, 3)    # row_ptr decreases
    assert e.value.code == 1
    with Assign(rp, ci, 3) as a:
        with pytest.raises(MMGError) as e:
            a.probabilities()                               # before a run
        assert e.value.code == 4
        tr = np.ones((3, 10))
        for first, count in ((5, 6), (0, 11), (-1, 3), (0, 0)):
            with pytest.raises(MMGError) as e:
                a.run_trace(tr, first=first, count=count)
            assert e.value.code == 1
        a.run_trace(tr, first=5, count=5)
        assert np.array_equal(a.probabilities(), [0.5, 0.5, 1.0])
        q = gpu.Problem.from_csr(np.array([0, 1], np.uint64), np.array([0], np.uint32), np.ones(5))
        smp = gpu.Sampler(q, np.ones(5), gibbs_iter=4, trace_len=4)
        smp.run(4)
        with pytest.raises(MMGError) as e:
            a.run(smp)                                      # 5 transcripts against 3
        assert e.value.code == 1
        smp.close()
        q.close()


def test_cli_writes_the_assignments(gpu, tmp_path):
    """mmseq -assign: .assign is .M with a third column, the posterior probability over chain 0's 1 024 samples; .counts / .gene.counts
    the host sums.  The trace file prints six digits, so the probabilities are restated from the oracle's chain for the same file and
    seed -- the chain the device runs bit for bit (tests/test_cli.py compares its printed samples with the same trace file).  Without
    the flag every other file and stdout are the same bytes."""
    h = dataset(n_reads=1500)
    for d in ("with", "without"):
        (tmp_path / d).mkdir()
        (tmp_path / d / "in.hits").write_bytes(H.write_hits_text(h))
    flag = run(["-gibbs_iter", "1024", "-seed", "5", "-assign", "in.hits", "out"], timeout=300, cwd=str(tmp_path / "with"))
    plain = run(["-gibbs_iter", "1024", "-seed", "5", "in.hits", "out"], timeout=300, cwd=str(tmp_path / "without"))
    assert flag.returncode == 0 and plain.returncode == 0, flag.stderr.decode() + plain.stderr.decode()
    listed = b"  out.assign\n  out.counts\n  out.gene.counts\n\n"
    assert flag.stdout.count(listed) == 1 and flag.stdout.replace(listed, b"") == plain.stdout
    names_with, names_without = sorted(os.listdir(tmp_path / "with")), sorted(os.listdir(tmp_path / "without"))
    assert sorted(set(names_with) - set(names_without)) == ["out.assign", "out.counts", "out.gene.counts"]
    for name in names_without:
        opener = gzip.open if name.endswith(".gz") else open
        assert opener(tmp_path / "with" / name, "rb").read() == opener(tmp_path / "without" / name, "rb").read(), name

    e = H.expected_run(h, seed=5, gibbs_iter=1024)
    g = e["ingest"]
    with gzip.open(tmp_path / "with" / "out.trace_gibbs.gz", "rt") as f:
        lines = f.read().split("\n")
    assert [ln.split(" ")[:-1] for ln in lines[1:-1]] == [[H.fmt6(v) for v in e["trace"][:, s]] for s in range(1024)]
    rows, k = e["rows"], np.asarray(e["k"])
    rp = np.cumsum([0] + [len(r) for r in rows])
    ci = np.array([c for r in rows for c in r])
    n = len(g["index_sid"])
    P = R.assign_ref(rp, ci, e["trace"])
    alines = (tmp_path / "with" / "out.assign").read_text().split("\n")
    mlines = (tmp_path / "with" / "out.M").read_text().split("\n")
    assert alines[-1] == "" and [ln.rsplit("\t", 1)[0] for ln in alines[:-1]] == mlines[1:-1]
    assert [ln.rsplit("\t", 1)[1] for ln in alines[:-1]] == ["%.9g" % v for v in P]
    E = R.expected_hits(rp, ci, P, n, k)
    of = lambda name: float(E[g["sid_index"][name]]) if name in g["sid_index"] else 0.0
    want = ["feature_id\texpected_hits"] + ["%s\t%.9g" % (name, of(name)) for name in h.names]
    assert (tmp_path / "with" / "out.counts").read_text().split("\n") == want + [""]
    want = ["feature_id\texpected_hits"]
    for gid, ts in h.genes.items():
        s = 0.0
        for name in ts:
            s += of(name)
        want.append("%s\t%.9g" % (gid, s))
    assert (tmp_path / "with" / "out.gene.counts").read_text().split("\n") == want + [""]


def test_it_estimates_what_the_sampler_draws(gpu):
    rp, ci, k, l, n_tx = R.stat_problem()
    prob = gpu.Problem.from_csr(rp, ci, l, k=k)
    mu0, _ = prob.start_values()
    smp = gpu.Sampler(prob, mu0, seed=4321, gibbs_iter=1024, trace_len=1024)
    counts = []
    for _ in range(1024):
        smp.run(1)
        counts.append(smp.counts(0))
    worst, n_exact, E = R.stat_rule(rp, ci, k, smp.trace(0), counts)
    print("largest |mean d| / (sd / sqrt(n)) = %.3f, transcripts with d = 0 throughout: %d" % (worst, n_exact))
    assert n_exact >= 12
    # the device's expected hits are the mean over the samples of those conditional expectations
    from mmseq_amd import Assign
    with Assign(rp, ci, n_tx) as a:
        a.run(smp)
        assert np.allclose(a.expected_hits(k), E.mean(axis=1), rtol=1e-12, atol=0.0)
        assert abs(a.expected_hits(k).sum() - float(k.sum())) <= 1e-9 * float(k.sum())
    smp.close()
    prob.close()
