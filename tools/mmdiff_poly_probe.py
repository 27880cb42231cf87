"""Stage timings of the polytomous mmdiff handle (mmg_diff_poly_*: J alternatives in every launch) against the same J comparisons run
one after another on single-comparison handles (mmg_diff_*), in one session: F features, 6 samples in groups 2, 2, 2 of generated
estimates (a fifth of the features shifted by 1.5 in the first group), the alternatives A != B = C, A = B != C, all differ, A = C != B,
default iteration counts.  One warm-up of each path (1024 + 1024 iterations, 8 tuning batches), then `repeats` timed runs of each,
interleaved.  Prints one JSON line per handle as it finishes, one per repeat and a summary line.
usage: mmdiff_poly_probe.py [F [repeats [burnin iters]]]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from mmseq_amd.diff import Diff, DiffPoly  # noqa: E402

N = 6
CLASSES1 = [np.array(c) for c in ([0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 0, 0])]
P1ROWS = [np.array([[0.5], [-0.5]]), np.eye(2), np.eye(3), np.array([[0.5], [-0.5]])]


def stages(h, burnin, iters, max_batches=8192):
    t0 = time.time()
    h.burnin(burnin)
    t1 = time.time()
    nb = h.tune(max_batches)
    t2 = time.time()
    h.sample(iters)
    t3 = time.time()
    return dict(burnin_s=round(t1 - t0, 3), tune_s=round(t2 - t1, 3), sample_s=round(t3 - t2, 3), total_s=round(t3 - t0, 3), batches=nb)


def one_run(y, e, burnin, iters, max_batches=8192):
    M, P0, C0 = np.zeros((N, 1)), np.ones((N, 1)), np.zeros(N, np.int64)
    P1s = [P1ROWS[j][CLASSES1[j]] for j in range(4)]
    h = DiffPoly(y, e, M, P0, C0, P1s, CLASSES1)
    out = stages(h, burnin, iters, max_batches)
    out["device_bytes"] = h.device_bytes()
    h.close()
    print(json.dumps(dict(path="one_run", **out)), flush=True)
    return out


def separate(y, e, burnin, iters, max_batches=8192):
    M, P0, C0 = np.zeros((N, 1)), np.ones((N, 1)), np.zeros(N, np.int64)
    out = []
    for j in range(4):
        d = Diff(y, e, M, P0, P1ROWS[j][CLASSES1[j]], np.stack([C0, CLASSES1[j]], 1))
        r = stages(d, burnin, iters, max_batches)
        r["device_bytes"] = d.device_bytes()
        d.close()
        print(json.dumps(dict(path="separate", alternative=j + 1, **r)), flush=True)
        out.append(r)
    return out


def main():
    a = [int(v) for v in sys.argv[1:]]
    F = a[0] if a else 20000
    repeats = a[1] if len(a) > 1 else 3
    burnin, iters = (a[2], a[3]) if len(a) > 3 else (8192, 16384)
    rng = np.random.default_rng(5)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, N))
    y[: F // 5, :2] += 1.5
    e = rng.uniform(0.05, 0.5, (F, N))
    print(json.dumps(dict(warmup=True)), flush=True)
    one_run(y, e, 1024, 1024, 8)       # warm-up: code objects loaded, allocator primed, clocks up
    separate(y, e, 1024, 1024, 8)
    print(json.dumps(dict(warmup=False)), flush=True)
    ratios_sum, ratios_max = [], []
    for rep in range(repeats):
        one = one_run(y, e, burnin, iters)
        sep = separate(y, e, burnin, iters)
        total = sum(r["total_s"] for r in sep)
        slowest = max(r["total_s"] for r in sep)
        ratios_sum.append(one["total_s"] / total)
        ratios_max.append(one["total_s"] / slowest)
        print(json.dumps(dict(F=F, N=N, J=4, repeat=rep, burnin=burnin, iters=iters, one_run=one, separate=sep,
                              separate_sum_s=round(total, 3), separate_slowest_s=round(slowest, 3),
                              one_run_over_sum=round(ratios_sum[-1], 3), one_run_over_slowest=round(ratios_max[-1], 3))), flush=True)
    print(json.dumps(dict(summary=True, F=F, repeats=repeats, one_run_over_sum=[round(min(ratios_sum), 3), round(max(ratios_sum), 3)],
                          one_run_over_slowest=[round(min(ratios_max), 3), round(max(ratios_max), 3)])), flush=True)


main()
