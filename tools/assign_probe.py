#!/usr/bin/env python
"""Times mmg_assign_run_sampler next to the chain of the same run and writes profiles/assign_probe.md.

Two shapes: `collapsed` -- 2 M hit sets with 83 M hits over 200 k transcripts -- and `reads` -- the benchmark's 50 M reads x 200 k transcripts, 1.0 G hits.  Per shape: the
chain's time for `--iters` iterations with every `--iters / 1024`-th sample kept, the pass's time (the device transpose of the trace
included), and the achieved bytes/s counted as 2 * 8 * S bytes per hit over the pass's time.

`collapsed` STANDS IN for a `synth_hits -zipf` file of that size: the rows are drawn here in numpy (Pareto row lengths cut at 5 000
hits, columns inside a window around a random centre, Zipf multiplicities cut at 10^6), not read from a file that tool wrote, so
the row-length tail and the locality of the columns are this generator's.

    python tools/assign_probe.py [--shape collapsed|reads|both] [--iters 1024] [--scale 1.0]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd import Assign, Problem, Sampler  # noqa: E402

S = 1024


def collapsed_rows(rows, n_tx, hits, seed=1):
    """Row lengths 1 + a Pareto tail scaled to `hits` in all (longest rows: thousands of hits), columns inside a window around a
    random centre so that the sampler's layout sees locality."""
    rng = np.random.default_rng(seed)
    raw = rng.pareto(1.3, rows) + 0.2
    L = np.minimum(1 + (raw * (hits - rows) / raw.sum()).astype(np.int64), 5000)
    rp = np.concatenate([[0], np.cumsum(L)]).astype(np.uint64)
    centre = np.repeat(rng.integers(0, n_tx, rows), L)
    spread = np.repeat(np.maximum(L, 8), L)
    ci = ((centre + (rng.random(centre.size) * 2 * spread).astype(np.int64) - spread) % n_tx).astype(np.uint32)
    k = np.minimum(rng.zipf(1.6, rows), 10 ** 6).astype(np.uint32)
    return rp, ci, k


def probe(name, prob, rp, ci, n_tx, iters):
    mu0, _ = prob.start_values()
    smp = Sampler(prob, mu0, gibbs_iter=iters, trace_len=S)
    smp.run(iters // 8)
    smp.sync()
    t0 = time.perf_counter()
    smp.run(iters - iters // 8)
    smp.sync()
    chain_s = (time.perf_counter() - t0) * iters / (iters - iters // 8)
    with Assign(rp, ci, n_tx) as a:
        a.run(smp)                                          # allocations, first touch
        t0 = time.perf_counter()
        a.run(smp)
        pass_s = time.perf_counter() - t0
        dev = a.device_bytes()
        total = float(a.probabilities().sum())
    smp.close()
    hits = int(ci.size)
    rows_with_hits = int((np.diff(rp.astype(np.int64)) > 0).sum())
    assert abs(total - rows_with_hits) <= 1e-6 * rows_with_hits
    return dict(name=name, rows=int(rp.size - 1), hits=hits, n_tx=n_tx, iters=iters, chain_s=chain_s, pass_s=pass_s,
                gbs=2 * 8 * S * hits / pass_s / 1e9, dev_gb=dev / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=("collapsed", "reads", "both"))
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks both shapes (rows and hits)")
    args = ap.parse_args()
    out = []
    n_tx = 200000
    if args.shape in ("collapsed", "both"):
        rp, ci, k = collapsed_rows(int(2e6 * args.scale), n_tx, int(83e6 * args.scale))
        prob = Problem.from_csr(rp, ci, np.full(n_tx, 1e-3), k=k)
        out.append(probe("collapsed", prob, rp, ci, n_tx, args.iters))
        prob.close()
    if args.shape in ("reads", "both"):
        prob = Problem.synthetic(int(50e6 * args.scale), n_tx, 20)
        rp, ci = prob.download()[:2]
        out.append(probe("reads", prob, rp, ci, n_tx, args.iters))
        prob.close()
    lines = ["# mmg_assign_run_sampler next to the chain of the same run (tools/assign_probe.py)", "",
             "| shape | rows | hits | chain, %d iterations | pass over 1024 samples | 2 x 8 x S bytes per hit / pass | device memory of the handle |" % args.iters,
             "|---|---|---|---|---|---|---|"]
    for r in out:
        lines.append("| %s | %d | %d | %.3f s | %.3f s | %.0f GB/s | %.2f GB |"
                     % (r["name"], r["rows"], r["hits"], r["chain_s"], r["pass_s"], r["gbs"], r["dev_gb"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "assign_probe.md"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
