"""What mmdiff's traces cost, at tools/mmdiff_probe.py's workload (F features x N samples, default 8192 + 16 384 iterations, every =
8 and 16 as the CLI sets them): the burn-in and sampling times of the library without tracing, with a sink that drops the rows (the
traced kernel, the copies out and the hand-over), and the CLI end to end with and without -traces with the bytes it wrote.  One JSON
line per measurement.
usage: mmdiff_trace_probe.py [F N [repeats]]"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import mmdiff_ref as R  # noqa: E402
from mmseq_amd.diff import Diff  # noqa: E402

BURNIN, ITERS = 8192, 16384
COLS = ("feature_id", "log_mu", "sd", "mcse", "iact", "effective_length", "true_length", "unique_hits")


def workload(F, N):
    rng = np.random.default_rng(5)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, N))
    y[: F // 5, : N // 2] += 1.5
    e = rng.uniform(0.05, 0.5, (F, N))
    return y, e


def library(F, N, traced, rep):
    y, e = workload(F, N)
    M, P0, P1, C = R.de_design([N // 2, N - N // 2])
    d = Diff(y, e, M, P0, P1, C)
    base = d.device_bytes()
    rows = [0, 0]

    def drop(phase, first, r):
        rows[phase] += r.shape[0]
        return 0

    if traced:
        d.open_traces(BURNIN // 1024, ITERS // 1024, drop)
    t0 = time.time()
    d.burnin(BURNIN)
    t1 = time.time()
    d.sample(ITERS)          # (no tuning: the tuning batches are the same launches either way)
    t2 = time.time()
    print(json.dumps(dict(what="library", F=F, N=N, traced=traced, rep=rep, burnin_s=round(t1 - t0, 4), sample_s=round(t2 - t1, 4),
                          rows=rows, trace_device_bytes=d.device_bytes() - base)), flush=True)
    d.close()


def cli(F, N, rep):
    y, e = workload(F, N)
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for s in range(N):
            path = os.path.join(tmp, "s%d.mmseq" % s)
            with open(path, "w") as f:
                f.write("# Mapped fragments: 1000\n" + "\t".join(COLS) + "\n")
                f.write("".join("f%d\t%r\t%r\t0.01\t1.5\t1000\t1200\t2\n" % (i, float(y[i, s]), float(e[i, s])) for i in range(F)))
            files.append(path)
        mmdiff = os.path.join(ROOT, "mmseq_amd", "csrc", "mmdiff")
        outs = {}
        for traced in (False, True):
            args = (["-traces", os.path.join(tmp, "tr")] if traced else []) + ["-notune", "-de", str(N // 2), str(N - N // 2)] + files
            t0 = time.time()
            r = subprocess.run([mmdiff] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            dt = time.time() - t0
            assert r.returncode == 0, r.stderr.decode()[-1000:]
            outs[traced] = r.stdout
            wrote = [ln for ln in r.stderr.decode().split("\n") if ln.startswith("Wrote ")]
            print(json.dumps(dict(what="cli -notune", F=F, N=N, traced=traced, rep=rep, wall_s=round(dt, 3),
                                  trace_bytes=int(wrote[0].split()[1]) if wrote else 0)), flush=True)
        assert outs[False] == outs[True]


a = [int(v) for v in sys.argv[1:]]
F, N, reps = (a + [20000, 6, 3][len(a):])[:3]
for rep in range(reps):
    for traced in (False, True):
        library(F, N, traced, rep)
for rep in range(reps):
    cli(F, N, rep)
