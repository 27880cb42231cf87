"""mmcollapse on the device (src/mmcollapse.cpp): V and the row maxima through the C ABI against the numpy restatement
(tests/mmcollapse_ref.py), the greedy loop on planted and random fixtures, determinism, the CLI end to end after our own mmseq,
and a scale run at C = 20 000, S = 8 with the device memory it holds."""
import hashlib
import math
import os
import subprocess
import time

import numpy as np
import pytest

import mmcollapse_ref as R
from oracle import host_oracle as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
N = 1024


def _collapse():
    from mmseq_amd.collapse import Collapse
    return Collapse


def _wide_traces(C, S, seed):
    """S samples of C columns, column scales log-uniform over 1e-40 .. 1e3, some columns sharing a factor"""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(math.log(1e-40), math.log(1e3), C))
    out = []
    for s in range(S):
        z = rng.gamma(2.0, 1.0, (N, C))
        f = rng.gamma(2.0, 1.0, (N, 8))
        z[:, : C // 2] += f[:, rng.integers(0, 8, C // 2)]
        out.append(z * scale)
    obs = rng.random((C, S)) > 0.15
    obs[0, :] = False                       # a candidate observed nowhere: NaN row
    return out, obs


def _close(got, want):
    bad = ~((np.abs(got - want) <= 1e-12 * np.abs(want)) | (np.abs(got - want) <= 1e-13) | (np.isnan(got) & np.isnan(want)))
    return int(bad.sum())


@pytest.mark.parametrize("C", [1000, 5003])
def test_v_and_row_max_match_numpy(C):
    tr, obs = _wide_traces(C, 3, seed=C)
    h = _collapse()(tr, obs)
    V = h.rows()
    want = R.mean_corr(R.centre(tr), obs)
    assert _close(V, want) == 0
    np.testing.assert_array_equal(V, V.T)
    rm = h.row_max()
    assert _close(rm, R.row_max(want)) == 0
    assert h.threshold(0.975) == pytest.approx(R.threshold(R.row_max(want), 0.975), rel=1e-12, abs=1e-13)
    h.close()


def _planted(C=240, S=3, seed=11):
    """groups of 2-4 columns whose traces share a near-constant total (anti-correlated), in a background of independent columns"""
    rng = np.random.default_rng(seed)
    groups, j = [], 0
    perm = rng.permutation(C)
    while j < C // 2:
        k = int(rng.integers(2, 5))
        groups.append(list(perm[j:j + k])); j += k
    tr = []
    for s in range(S):
        X = rng.gamma(3.0, 1.0, (N, C))
        for g in groups:
            w = rng.dirichlet(np.ones(len(g)) * 2.0, N)
            X[:, g] = 5.0 * w * (1.0 + 0.02 * rng.normal(size=(N, 1)))
        tr.append(X)
    obs = np.ones((C, S), bool)
    obs[rng.integers(0, C, 10), rng.integers(0, S, 10)] = False
    return tr, obs


def test_greedy_loop_planted_exact():
    tr, obs = _planted()
    C = obs.shape[0]
    names = ["t%04d" % i for i in range(C)]
    ref = R.Greedy(tr, obs, names)
    thr = R.threshold(R.row_max(ref.V), 0.975)
    want = ref.run(thr, tie_tol=1e-9)
    assert len(want) >= 20
    h = _collapse()(tr, obs)
    assert h.threshold(0.975) == pytest.approx(thr, rel=1e-12)
    pairs, vals, stopped = h.run(thr)
    assert stopped
    assert [tuple(map(int, p)) for p in pairs] == [(a, b) for a, b, _ in want]
    np.testing.assert_allclose(vals, [v for _, _, v in want], rtol=1e-12)
    got = list(names)
    for a, b in pairs:
        t = sorted([got[a], got[b]])
        got[a] = t[0] + "*" + t[1]
        got[b] = "NA"
    assert got == ref.names
    h.close()


def test_greedy_loop_random_replays():
    rng = np.random.default_rng(3)
    C, S = 400, 3
    tr = [rng.gamma(1.0, 1.0, (N, C)) for _ in range(S)]
    obs = rng.random((C, S)) > 0.1
    h = _collapse()(tr, obs)
    thr = h.threshold(0.2)
    pairs, vals, stopped = h.run(thr)
    assert stopped and len(pairs) > 0
    ref = R.Greedy(tr, obs)
    stop, last = ref.replay(thr, pairs, tol=1e-9)
    assert stop or (last is not None and abs(last - thr) <= 1e-9)
    h.close()


def test_deterministic():
    tr, obs = _wide_traces(1000, 3, seed=77)
    out = []
    for _ in range(2):
        h = _collapse()(tr, obs)
        V = h.rows()
        thr = h.threshold(0.9)
        p, v, _ = h.run(thr, max_merges=300)
        out.append((V, p, v, h.rows()))
        h.close()
    for a, b in zip(out[0], out[1]):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ end to end
def _families(seed, n_fam=12, n_single=30, n_reads=6000):
    """paralogue families of 2-4 transcripts whose reads hit at least two members (no unique hits), and singletons with reads of
    their own; every transcript gets hits"""
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
        share = rng.dirichlet(np.ones(len(f)))
        for _ in range(int(rng.integers(150, 400))):
            k = int(rng.integers(2, len(f) + 1))
            ts = sorted(rng.choice(len(f), k, replace=False, p=share if k == 1 else None))
            reads.append(("r%07d" % r, [f[t] for t in ts])); r += 1
    for i, s in enumerate(singles):
        for _ in range(int(rng.integers(20, 200))):
            hit = [s]
            if rng.random() < 0.3:
                hit.append(singles[(i + 1) % n_single])
            reads.append(("r%07d" % r, sorted(hit))); r += 1
    return H.HitsData(names, efflen, truelen, genes, [], reads)


def _digest(paths):
    return {p: (os.stat(p).st_mtime_ns, hashlib.sha256(open(p, "rb").read()).hexdigest()) for p in paths}


def _same(txt, val, rel=2e-5):
    if isinstance(val, str):
        return txt == val
    if isinstance(val, (int, np.integer)):
        return txt == str(int(val))
    if math.isnan(val):
        return txt == "nan"
    return abs(float(txt) - val) <= rel * abs(val) + 1e-12


def test_end_to_end_three_samples(tmp_path):
    bases = []
    for s in range(3):
        h = _families(100 + s)
        p = tmp_path / ("s%d.hits" % s)
        p.write_bytes(H.write_hits_text(h))
        base = str(tmp_path / ("s%d" % s))
        r = subprocess.run([os.path.join(BIN_DIR, "mmseq"), str(p), base], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        bases.append(base)
    inputs = sorted(str(x) for x in tmp_path.iterdir())
    before = _digest(inputs)
    r = subprocess.run([os.path.join(BIN_DIR, "mmcollapse")] + bases, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       env=dict(os.environ, MMSEQ_TIMING="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert _digest(inputs) == before
    merges, names, want = R.run(bases)
    assert len(merges) > 0 and any("*" in n for n in names)
    for base in bases:
        com, rows = want[base]
        lines = open(base + ".collapsed.mmseq").read().rstrip("\n").split("\n")
        assert lines[:len(com)] == com
        assert lines[len(com)] == "feature_id\tlog_mu\tsd\tmcse\teffective_length\tiact\tunique_hits"
        got = [ln.split("\t") for ln in lines[len(com) + 1:]]
        assert [g[0] for g in got] == [w[0] for w in rows]
        for g, w in zip(got, rows):
            assert g[4] == "NA"
            assert g[6] == str(w[5]), (g, w)
            for txt, val in ((g[1], w[1]), (g[2], w[2]), (g[3], w[3]), (g[5], w[4])):
                assert _same(txt, val), (g, w)


def test_scale_20000_by_8():
    C, S = 20000, 8
    rng = np.random.default_rng(5)
    obs = rng.random((C, S)) > 0.05
    from mmseq_amd.collapse import Collapse
    t0 = time.time()
    tr = [rng.gamma(1.0, 1.0, (N, C)) for _ in range(S)]
    h = Collapse(tr, obs)
    del tr
    t1 = time.time()
    thr = h.threshold(0.2)
    pairs, vals, stopped = h.run(thr, max_merges=500)
    t2 = time.time()
    slack = 64 << 20
    assert h.device_bytes() < C * C * 8 + S * N * C * 8 + slack
    assert len(pairs) > 0 and np.all(vals < thr)
    assert t2 - t0 < 300
    h.close()
