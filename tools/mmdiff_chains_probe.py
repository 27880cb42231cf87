"""Stage timings of mmdiff's chains handle (mmg_diff_chains_*: C chains in every launch) against the single run (mmg_diff_*) and against
the same C chains one after another on seed-shifted single handles, in one session: F features, 6 samples in groups 3, 3 of generated
estimates (a fifth of the features shifted by 1.5 in the first group), default iteration counts.  One warm-up of each path (1024 + 1024
iterations, 8 tuning batches), then one timed run of the single handle, of the chains handle at C = 1, 4 and 8, and of the 8 separate
chains (the first 4 of them are what C = 4 is set against).  Prints one JSON line per handle as it finishes and a summary line with
the ratios and, at the largest C, the median over the null features of log_bf_sd / (sqrt(C) log_bf_mcse).
usage: mmdiff_chains_probe.py [F [burnin iters]]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from mmseq_amd.diff import Diff, DiffChains  # noqa: E402

N = 6
CS = (1, 4, 8)
SEED = 1234


def design():
    C = np.stack([np.zeros(N, np.int64), np.repeat([0, 1], N // 2)], 1)
    return np.zeros((N, 1)), np.ones((N, 1)), np.where(C[:, 1:] == 0, 0.5, -0.5), C


def stages(h, burnin, iters, max_batches=8192, pool=False):
    t0 = time.time()
    h.burnin(burnin)
    t1 = time.time()
    nb = h.tune(max_batches)
    t2 = time.time()
    h.sample(iters)
    t3 = time.time()
    if pool:
        h.pool()
    t4 = time.time()
    return dict(burnin_s=round(t1 - t0, 3), tune_s=round(t2 - t1, 3), sample_s=round(t3 - t2, 3), pool_s=round(t4 - t3, 3),
                total_s=round(t4 - t0, 3), batches=nb)


def single(y, e, burnin, iters, chain=0, max_batches=8192):
    d = Diff(y, e, *design(), seed=SEED ^ (chain << 32))
    out = stages(d, burnin, iters, max_batches)
    out["device_bytes"] = d.device_bytes()
    d.close()
    print(json.dumps(dict(path="single", chain=chain, **out)), flush=True)
    return out


def chains(y, e, C, burnin, iters, max_batches=8192, n_null_from=None):
    h = DiffChains(y, e, *design(), C, iters, seed=SEED)
    out = stages(h, burnin, iters, max_batches, pool=True)
    out["device_bytes"] = h.device_bytes()
    if n_null_from is not None and C > 1:
        p = h.pooled()
        with np.errstate(all="ignore"):
            ratio = p["log_bf_sd"][n_null_from:] / (np.sqrt(float(C)) * p["log_bf_mcse"][n_null_from:])
        ok = np.isfinite(ratio)
        out["null_features_with_a_ratio"] = int(ok.sum())
        out["median_sd_over_sqrtC_mcse"] = round(float(np.median(ratio[ok])), 3) if ok.any() else None
        out["features_not_mixed_in_every_chain"] = int((p["chains_mixed"] < C).sum())
    h.close()
    print(json.dumps(dict(path="chains", C=C, **out)), flush=True)
    return out


def main():
    a = [int(v) for v in sys.argv[1:]]
    F = a[0] if a else 20000
    burnin, iters = (a[1], a[2]) if len(a) > 2 else (8192, 16384)
    rng = np.random.default_rng(5)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, N))
    y[: F // 5, : N // 2] += 1.5
    e = rng.uniform(0.05, 0.5, (F, N))
    print(json.dumps(dict(warmup=True)), flush=True)
    single(y, e, 1024, 1024, 0, 8)         # warm-up: code objects loaded, allocator primed, clocks up
    chains(y, e, 2, 1024, 1024, 8)
    print(json.dumps(dict(warmup=False)), flush=True)
    one = single(y, e, burnin, iters)
    runs = {C: chains(y, e, C, burnin, iters, n_null_from=F // 5) for C in CS}
    sep = [one] + [single(y, e, burnin, iters, c) for c in range(1, max(CS))]
    summary = dict(summary=True, F=F, N=N, burnin=burnin, iters=iters, single_s=one["total_s"])
    for C in CS:
        tot, slow = sum(r["total_s"] for r in sep[:C]), max(r["total_s"] for r in sep[:C])
        summary["C%d" % C] = dict(total_s=runs[C]["total_s"], over_single=round(runs[C]["total_s"] / one["total_s"], 3),
                                  separate_sum_s=round(tot, 3), over_separate_sum=round(runs[C]["total_s"] / tot, 3),
                                  separate_slowest_s=round(slow, 3), over_separate_slowest=round(runs[C]["total_s"] / slow, 3))
    print(json.dumps(summary), flush=True)


main()
