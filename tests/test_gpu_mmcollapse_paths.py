"""mmcollapse's device paths that tests/test_gpu_mmcollapse.py leaves open, each against an independent yardstick (the numpy
restatement tests/mmcollapse_ref.py, the C oracle's keyed draws and Sokal): the output stage with simulated traces, V and the row
maxima at tile edges and degenerate columns, long merge chains over more than one workgroup of columns, exact ties, runs in chunks
and the state errors of the C entries."""
import ctypes as C
import os
import subprocess
import gzip

import numpy as np
import pytest

import mmcollapse_ref as R
from oracle import binding as B
from oracle import host_oracle as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")


def _collapse():
    from mmseq_amd.collapse import Collapse
    return Collapse


def _close(got, want):
    """entries off by more than 1e-12 relative and 1e-13 absolute, NaN equal to NaN and infinities to themselves"""
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
        ok = (got == want) | (d <= 1e-12 * np.abs(want)) | (d <= 1e-13) | (np.isnan(got) & np.isnan(want))
    return int((~ok).sum())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------ the output stage
@pytest.mark.parametrize("N", [1024, 1000, 16384, 16])
def test_summarize_matches_numpy_and_the_oracle(N):
    from mmseq_amd.collapse import summarize
    rng = np.random.default_rng(N)
    n, nv = 7, 5
    trace = rng.gamma(2.0, 1.0, (N, n)) * np.exp(rng.uniform(np.log(1e-6), np.log(1e2), n))
    vid = np.array([3, 17, 0, 12345678901, 42], np.uint64)
    vscale = np.array([1e-6, 3.7e-3, 1.0, 55.0, 1e2])
    # singletons real and virtual, virtual members only, mixed sets, members out of column order
    groups = [[0], [n + 2], [3, 1], [n + 0, 2], [n + 3, n + 1], [6, n + 4, 4, 5], [n + 1], [5, n + 2, 0]]
    for stream in (0, 2, 5):
        lm, var, tau, rc = summarize(trace, groups, virtual_id=vid, virtual_scale=vscale, stream=stream)
        V = [B.simu_gamma_trace_keyed(13837, stream, B.TAG_COLLAPSE_SIMU, int(vid[v]), 0.1, vscale[v], N) for v in range(nv)]
        full = [trace[:, c] for c in range(n)] + V
        for g, ms in enumerate(groups):
            t = np.zeros(N)
            for m in ms:
                t = t + full[m]                                  # the members in the order given, as k_group_sums
            y = np.log(t)
            np.testing.assert_allclose(lm[g], y.mean(), rtol=1e-12, err_msg="stream %d series %d" % (stream, g))
            orc_rc, orc_var, orc_tau, _ = B.sokal(y)
            assert rc[g] == orc_rc, (stream, g)
            if orc_rc == 0:
                np.testing.assert_allclose([var[g], tau[g]], [orc_var, orc_tau], rtol=1e-9, err_msg="stream %d series %d" % (stream, g))
        assert (rc == 201).all() if N == 1000 else (rc == 0).all()


# ------------------------------------------------------------------------------------------ end to end with simulated traces
# the transcripts without reads in a sample (sample 0 keeps every one: the list of features comes from the first sample)
DROPPED = {0: (), 1: ("P01_0", "P04_2", "P07_1", "S003", "S010"), 2: ("P02_3", "P05_1", "P08_0", "S007")}


def _families_with_gaps(seed, drop, n_fam=12, n_single=30):
    """tests/test_gpu_mmcollapse.py's paralogue families and singletons, where the transcripts in drop get no reads (members of
    families of three or four only, so what remains of a family still has no unique hits)"""
    rng = np.random.default_rng(seed)
    names, fams = [], []
    for f in range(n_fam):
        k = 2 + f % 3
        fams.append(["P%02d_%d" % (f, i) for i in range(k)])
        names += fams[-1]
    singles = ["S%03d" % i for i in range(n_single)]
    names += singles
    efflen = {n: 1000.0 + 10 * i for i, n in enumerate(names)}
    truelen = {n: int(efflen[n]) + 180 for n in names}
    genes = {"G%03d" % i: [n] for i, n in enumerate(names)}
    reads = []
    r = 0
    for f in fams:
        live = [t for t in f if t not in drop]
        assert len(live) >= 2
        for _ in range(int(rng.integers(150, 400))):
            k = int(rng.integers(2, len(live) + 1))
            ts = sorted(rng.choice(len(live), k, replace=False))
            reads.append(("r%07d" % r, [live[t] for t in ts])); r += 1
    for i, s in enumerate(singles):
        if s in drop:
            continue
        for _ in range(int(rng.integers(20, 200))):
            hit = [s]
            if rng.random() < 0.3 and singles[(i + 1) % n_single] not in drop:
                hit.append(singles[(i + 1) % n_single])
            reads.append(("r%07d" % r, sorted(hit))); r += 1
    return H.HitsData(names, efflen, truelen, genes, [], reads)


def _trace_ids(path):
    with gzip.open(path, "rt") as f:
        return f.readline().split()


def _same(txt, val, rel=2e-5):
    if isinstance(val, (int, np.integer)):
        return txt == str(int(val))
    if np.isnan(val):
        return txt == "nan"
    return abs(float(txt) - val) <= rel * abs(val) + 1e-12


def test_end_to_end_with_simulated_traces(tmp_path):
    bases = []
    for s in range(3):
        p = tmp_path / ("s%d.hits" % s)
        p.write_bytes(H.write_hits_text(_families_with_gaps(200 + s, DROPPED[s])))
        base = str(tmp_path / ("s%d" % s))
        r = subprocess.run([os.path.join(BIN_DIR, "mmseq"), str(p), base], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        bases.append(base)
    r = subprocess.run([os.path.join(BIN_DIR, "mmcollapse")] + bases, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    merges, names, want = R.run(bases)
    # the fixture does what it is for: the dropped transcripts have no trace, and a final set holds one of them
    for s, base in enumerate(bases):
        ids = set(_trace_ids(base + ".trace_gibbs.gz"))
        assert not ids & set(DROPPED[s]) and len(ids) > 40
    sets = [set(n.split("*")) for n in names if "*" in n]
    simulated_in_a_set = [t for s in (1, 2) for t in DROPPED[s] if any(t in x for x in sets)]
    assert simulated_in_a_set, names
    for base in bases:
        com, rows = want[base]
        lines = open(base + ".collapsed.mmseq").read().rstrip("\n").split("\n")
        assert lines[:len(com)] == com
        got = [ln.split("\t") for ln in lines[len(com) + 1:]]
        assert [g[0] for g in got] == [w[0] for w in rows]
        for g, w in zip(got, rows):
            assert g[6] == str(w[5]), (g, w)
            for txt, val in ((g[1], w[1]), (g[2], w[2]), (g[3], w[3]), (g[5], w[4])):
                assert _same(txt, val), (base, g, w)


# ------------------------------------------------------------------------------------------ V and the row maxima across shapes
def _shaped(C, S, N, seed):
    """random traces with shared factors, and among the columns: a constant one (zero variance), one observed nowhere, one observed
    in one sample only, and two scaled to 1e-170 (x * x underflows to zero)"""
    rng = np.random.default_rng(seed)
    tr = []
    for s in range(S):
        z = rng.gamma(2.0, 1.0, (N, C))
        f = rng.gamma(2.0, 1.0, (N, 4))
        z[:, : C // 2] += f[:, rng.integers(0, 4, C // 2)]
        z *= np.exp(rng.uniform(np.log(1e-30), np.log(1e3), C))
        tr.append(z)
    obs = rng.random((C, S)) > 0.2
    special = rng.permutation(C)[:5]
    if C > 2:
        for z in tr:
            z[:, special[0]] = 3.25
    if C > 3:
        obs[special[1], :] = False
        obs[special[2], :] = False
        obs[special[2], 0] = True
    if C > 5:
        for z in tr:
            z[:, special[3:5]] *= 1e-170 / np.abs(z[:, special[3:5]]).max(axis=0)
    return tr, obs


@pytest.mark.parametrize("C,S,N", [(2, 1, 16), (3, 2, 1024), (63, 5, 2048), (64, 1, 1024), (65, 2, 16), (129, 5, 1024),
                                   (1025, 2, 2048), (129, 1, 2048), (64, 5, 16)])
def test_v_and_row_max_across_shapes(C, S, N):
    tr, obs = _shaped(C, S, N, seed=C * 31 + S * 7 + N)
    h = _collapse()(tr, obs)
    V = h.rows()
    want = R.mean_corr(R.centre(tr), obs)
    assert _close(V, want) == 0
    assert np.array_equal(V, V.T, equal_nan=True)
    assert _close(h.row_max(), R.row_max(want)) == 0
    if C > 5:
        assert np.isnan(want).any() and np.isnan(V).any()          # the degenerate columns are there
    h.close()


# ------------------------------------------------------------------------------------------ long merge chains
def _chains(C=2100, S=2, n_groups=200, n_tri=12, seed=21):
    """groups of 2-6 columns sharing a near-constant total with strongly uneven shares: the loop merges each group whole, a merged
    candidate again and again, over 600 merges; groups and the background are spread over all 2100 columns.  And triangles a < b,
    j: a = u + z, b = -u - z, j = z (plus noise), so (a, b) is merged first (V near -1) while column j's minimum, -0.7, sits in row
    b; the merged a + b is independent of j, so that minimum must be rescanned, not kept from the dead row."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(C)
    groups, j = [], 0
    for _ in range(n_groups):
        k = int(rng.integers(2, 7))
        groups.append(perm[j:j + k]); j += k
    tris = []
    for _ in range(n_tri):
        a, b = sorted(perm[j:j + 2])
        tris.append((a, b, perm[j + 2])); j += 3
    tr = []
    for s in range(S):
        X = rng.gamma(3.0, 1.0, (1024, C))
        for g in groups:
            w = rng.dirichlet(np.ones(len(g)) * 0.3, 1024)
            X[:, g] = 5.0 * w * (1.0 + 0.01 * rng.normal(size=(1024, 1)))
        for a, b, jj in tris:
            u, z = rng.normal(size=(2, 1024))
            X[:, a] = 10.0 + u + z + 0.05 * rng.normal(size=1024)
            X[:, b] = 10.0 - u - z + 0.05 * rng.normal(size=1024)
            X[:, jj] = 10.0 + z + 0.05 * rng.normal(size=1024)
        tr.append(X)
    return tr, np.ones((C, S), bool), tris


def test_long_merge_chains_beyond_one_workgroup():
    tr, obs, tris = _chains()
    thr = -0.15                       # the loop stops at -0.100: far from any decision
    ref = R.Greedy(tr, obs)
    for a, b, j in tris:              # column j's minimum sits in row b, below thr
        assert R.vmin(ref.V[:, [j]])[1] == b and ref.V[b, j] < -0.6
    h = _collapse()(tr, obs)
    got_p, got_v = [], []
    want = []
    for m in (150, 300, None):        # checkpoints: the whole of V, dead rows and columns included
        w = ref.run(thr, tie_tol=1e-9, max_merges=None if m is None else m - len(want))
        p, v, stopped = h.run(thr, max_merges=(1 << 20) if m is None else m - len(got_p))
        want += w
        got_p += [tuple(map(int, x)) for x in p]
        got_v += list(v)
        assert got_p == [(a, b) for a, b, _ in want]
        assert stopped == (m is None)
        assert _close(h.rows(), ref.V) == 0, "V after %d merges" % len(want)
    assert len(want) >= 500
    np.testing.assert_allclose(got_v, [v for _, _, v in want], rtol=1e-12)
    into = np.bincount([a for a, _ in got_p])
    assert into.max() >= 4                                        # one candidate merged again and again
    assert max(a for a, _ in got_p) >= 1024                       # picks in columns past the first 1024
    h.close()


# ------------------------------------------------------------------------------------------ exact ties
def _ties(S=2, n_bg=70, n_pairs=8, seed=8):
    """strongly anti-correlated pairs (p, q), p < q, each of a different strength, in an independent background, and copies of q
    scaled by 2^k after every original column: a copy d has V(p, d) = V(p, q) bit for bit (the scale cancels exactly, and d is the
    higher index of its pair as q is, so even the order of the divisions is the same), on the device and in the restatement's fixed
    order alike.  So each pair's pick ties between columns p, q and the copies, and in column p between rows q and the copies."""
    rng = np.random.default_rng(seed)
    tr = [rng.gamma(3.0, 1.0, (1024, n_bg + 2 * n_pairs)) for _ in range(S)]
    pairs = []
    for i in range(n_pairs):
        p, q = n_bg + 2 * i, n_bg + 2 * i + 1
        pairs.append((p, q))
        for X in tr:
            w = rng.beta(0.5, 0.5, 1024)
            T = 5.0 * (1.0 + (0.005 + 0.01 * i) * rng.normal(size=1024))
            X[:, p] = T * w
            X[:, q] = T * (1 - w)
    dup = []
    for i, (p, q) in enumerate(pairs):
        dup.append((q, [3, -2, 5][i % 3]))
        if i % 2 == 0:
            dup.append((q, [-4, 6][i % 4 // 2]))
    copies = {q: [tr[0].shape[1] + i for i, (c, _) in enumerate(dup) if c == q] for _, q in pairs}
    tr = [np.concatenate([X] + [np.ldexp(X[:, [c]], k) for c, k in dup], axis=1) for X in tr]
    return tr, np.ones((tr[0].shape[1], S), bool), pairs, copies


def test_exact_ties_follow_the_column_major_rule():
    tr, obs, pairs, copies = _ties()
    ref = R.Greedy(tr, obs, fixed_order=True)
    h = _collapse()(tr, obs)
    V = h.rows()
    for p, q in pairs:                # the ties are real: bit-equal entries on the device as in the restatement
        for d in copies[q]:
            assert V[p, d] == V[p, q] and V[d, p] == V[q, p] and ref.V[p, d] == ref.V[p, q] and ref.V[d, p] == ref.V[q, p]
    thr = -0.5
    want = []
    while True:                       # one pick at a time: the device's (row, col) against R.vmin's
        m = R.vmin(ref.V)
        w = ref.run(thr, tie_tol=1e-9, max_merges=1)
        p, v, stopped = h.run(thr, max_merges=1)
        if not w:
            assert len(p) == 0 and stopped
            break
        assert [tuple(map(int, x)) for x in p] == [(a, b) for a, b, _ in w], "pick %d" % len(want)
        assert (min(m[1], m[2]), max(m[1], m[2])) == tuple(map(int, p[0]))
        np.testing.assert_allclose(v, [w[0][2]], rtol=1e-12)
        want += w
    assert len(want) == len(pairs)
    assert ref.exact_ties >= len(pairs)                           # every pick was decided by the tie rule
    assert [(a, b) for a, b, _ in want] == sorted(pairs, key=lambda pq: pq[0])
    h.close()


# ------------------------------------------------------------------------------------------ continuation and state
def _planted(C=240, S=3, seed=11):
    rng = np.random.default_rng(seed)
    groups, j = [], 0
    perm = rng.permutation(C)
    while j < C // 2:
        k = int(rng.integers(2, 5))
        groups.append(list(perm[j:j + k])); j += k
    tr = []
    for s in range(S):
        X = rng.gamma(3.0, 1.0, (1024, C))
        for g in groups:
            w = rng.dirichlet(np.ones(len(g)) * 2.0, 1024)
            X[:, g] = 5.0 * w * (1.0 + 0.02 * rng.normal(size=(1024, 1)))
        tr.append(X)
    obs = np.ones((C, S), bool)
    obs[rng.integers(0, C, 10), rng.integers(0, S, 10)] = False
    return tr, obs


def test_runs_in_chunks_equal_one_run():
    tr, obs = _planted()
    Collapse = _collapse()
    h = Collapse(tr, obs)
    thr = h.threshold(0.975)
    p_all, v_all, stopped = h.run(thr)
    assert stopped and len(p_all) >= 20
    rows_all = h.rows()
    p, v, s = h.run(thr)                                          # after the stop: nothing more
    assert len(p) == 0 and len(v) == 0 and s
    h.close()
    for chunks in ([1] * (len(p_all) + 1), [7, 1 << 20]):
        h = Collapse(tr, obs)
        ps, vs = [], []
        for k in chunks:
            p, v, stopped = h.run(thr, max_merges=k)
            ps.append(p); vs.append(v)
            if stopped:
                break
        assert stopped
        assert np.concatenate(ps).tobytes() == p_all.tobytes()
        assert np.concatenate(vs).tobytes() == v_all.tobytes()
        assert h.rows().tobytes() == rows_all.tobytes()
        h.close()


def test_fewer_than_two_candidates_collapse_nothing():
    Collapse = _collapse()
    h = Collapse([np.zeros((1024, 0)), np.zeros((1024, 0))], np.zeros((0, 2), bool))
    assert h.rows().shape == (0, 0) and h.row_max().shape == (0,)
    p, v, stopped = h.run(0.0)
    assert len(p) == 0 and stopped
    h.close()
    rng = np.random.default_rng(1)
    h = Collapse([rng.gamma(2.0, 1.0, (1024, 1)) for _ in range(2)], np.ones((1, 2), bool))
    assert h.row_max().tolist() == [-1.0]
    thr = h.threshold(0.975)
    assert thr == 1.0
    p, v, stopped = h.run(thr)
    assert len(p) == 0 and stopped
    h.close()


def test_state_errors_of_the_c_entries():
    from mmseq_amd import _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    S, Cn, N = 2, 5, 32
    obs = np.ones((Cn, S), np.uint8)
    tr = np.random.default_rng(2).gamma(2.0, 1.0, (N, Cn))
    h = C.c_void_p()
    _lib.check(lib.mmg_collapse_create(0, S, Cn, N, _ptr(obs), C.byref(h)))
    try:
        pairs = np.empty(8, np.uint32)
        vals = np.empty(4)
        n = C.c_uint32(0)
        st = C.c_int32(0)
        rows = np.empty((Cn + 1, Cn))
        _lib.check(lib.mmg_collapse_set_sample(h, 0, _ptr(tr)))
        with pytest.raises(MMGError) as e:                        # correlate before every sample is set
            _lib.check(lib.mmg_collapse_correlate(h))
        assert e.value.code == 4
        with pytest.raises(MMGError) as e:                        # run before correlate
            _lib.check(lib.mmg_collapse_run(h, 0.0, 4, _ptr(pairs), _ptr(vals), C.byref(n), C.byref(st)))
        assert e.value.code == 4
        with pytest.raises(MMGError) as e:                        # rows before correlate
            _lib.check(lib.mmg_collapse_get_rows(h, 0, 1, _ptr(rows)))
        assert e.value.code == 4
        with pytest.raises(MMGError) as e:                        # sample out of range
            _lib.check(lib.mmg_collapse_set_sample(h, S, _ptr(tr)))
        assert e.value.code == 1
        _lib.check(lib.mmg_collapse_set_sample(h, 1, _ptr(tr)))
        _lib.check(lib.mmg_collapse_correlate(h))
        with pytest.raises(MMGError) as e:                        # set_sample after correlate
            _lib.check(lib.mmg_collapse_set_sample(h, 0, _ptr(tr)))
        assert e.value.code == 4
        for first, count in ((0, Cn + 1), (Cn, 1), (3, 3)):       # rows out of range
            with pytest.raises(MMGError) as e:
                _lib.check(lib.mmg_collapse_get_rows(h, first, count, _ptr(rows)))
            assert e.value.code == 1
        _lib.check(lib.mmg_collapse_get_rows(h, 1, Cn - 1, _ptr(rows)))
        _lib.check(lib.mmg_collapse_run(h, -2.0, 4, _ptr(pairs), _ptr(vals), C.byref(n), C.byref(st)))
        assert n.value == 0 and st.value == 1
    finally:
        lib.mmg_collapse_destroy(h)
    for bad in (0, 8, 24):
        with pytest.raises(MMGError) as e:
            _lib.check(lib.mmg_collapse_create(0, S, Cn, bad, _ptr(obs), C.byref(h)))
        assert e.value.code == 1
