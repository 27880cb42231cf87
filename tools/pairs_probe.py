#!/usr/bin/env python
"""Times the pairs pass (mmg_pairs_create) next to the chain and mmg_summary_finish of the same run and writes profiles/pairs_probe.md.

The 200 000-transcript generated problem, 1 024 kept samples, 1 000 000 pairs drawn within windows of the transcript order (a
transcript against one of the `--window` that follow it: what shares reads is mostly a neighbour).  One run, timed on the host: the
clock around the call also holds what is not a kernel (the checks and the compaction of the members on the host, the allocations,
the copies), so the kernels' own times come from a second run under the profiler, whose trace a third call appends:

    python tools/pairs_probe.py [--rows 2000000] [--window 8]
    rocprofv3 --kernel-trace -d DIR -- python tools/pairs_probe.py --no-write
    python tools/pairs_probe.py --kernel-db DIR/.../*_results.db
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd import Pairs, Problem, Sampler  # noqa: E402
from mmseq_amd import gibbs  # noqa: E402

S = 1024
N_PAIRS = 1_000_000
MD = os.path.join(ROOT, "profiles", "pairs_probe.md")
KERNELS = ("k_pair_", "k_contrast_gather", "k_series_summary")
HEAD = "## Kernel times"


def kernel_section(db_path):
    """the kernels of the pass in a rocprofv3 trace of this probe (rocpd: the view `kernels`, durations in ns)"""
    import sqlite3
    rows = sqlite3.connect(db_path).cursor().execute(
        "select name, count(*), sum(duration), sum(grid_x / workgroup_x) from kernels group by name order by sum(duration) desc").fetchall()
    lines = [HEAD + " (one run of this probe under `rocprofv3 --kernel-trace`)", "",
             "`k_pair_members` and `k_pair_stats` run four waves per workgroup, a member or a pair each.", "",
             "| kernel | launches | total ms | workgroups | us per workgroup |", "|---|---|---|---|---|"]
    for name, calls, ns, wgs in rows:
        if any(k in name for k in KERNELS):
            lines.append("| `%s` | %d | %.3f | %d | %.3f |" % (name[:100], calls, ns / 1e6, wgs, ns / 1e3 / max(wgs, 1)))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--no-write", action="store_true", help="run the pass and print, but leave profiles/pairs_probe.md (a run under the profiler)")
    ap.add_argument("--kernel-db", default="", help="no run: append the kernel times of this rocprofv3 trace (.db) of the probe to the file")
    args = ap.parse_args()
    if args.kernel_db:
        text = open(MD).read().split(HEAD)[0].rstrip("\n") + "\n\n" + kernel_section(args.kernel_db)
        with open(MD, "w") as f:
            f.write(text)
        print(text)
        return
    n = 200_000
    rng = np.random.default_rng(1)
    a = rng.integers(0, n - args.window, N_PAIRS)
    pairs = np.stack([a, a + rng.integers(1, args.window + 1, N_PAIRS)], axis=1)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]      # in (a, b) order, as the CLI generates them: a slab's members are neighbours
    prob = Problem.synthetic(args.rows, n, 20)
    mu0, _ = prob.start_values()
    smp = Sampler(prob, mu0, gibbs_iter=S, trace_len=S)
    q = gibbs.Summary(smp, staged=True)
    t0 = time.perf_counter()
    smp.run(S)
    smp.sync()
    chain_s = time.perf_counter() - t0
    q.advance(S)
    t0 = time.perf_counter()
    q.finish()
    finish_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    with Pairs.from_sampler(smp, pairs) as h:
        pass_s = time.perf_counter() - t0
        dev = h.device_bytes()
        s = h.summary()
    q.close()
    smp.close()
    prob.close()
    distinct = np.unique(pairs).size
    lines = ["# The pairs pass next to the chain and mmg_summary_finish of the same run (tools/pairs_probe.py)", "",
             "%d transcripts, %d reads, %d kept samples, %d pairs within windows of %d of the transcript order (%d distinct members)."
             % (n, args.rows, S, N_PAIRS, args.window, distinct),
             "One run on one MI355X, timed on the host: allocations, the gather, the copies of the results and the host's compaction of",
             "the members included.  These are the figures of that one run, not a mean and not a bound.", "",
             "| stage | time | per unit |", "|---|---|---|",
             "| the chain, %d iterations | %.3f s | %.3f ms per iteration |" % (S, chain_s, chain_s / S * 1e3),
             "| mmg_summary_finish (%d log series + %d proportion series) | %.3f s | %.2f us per series |" % (n, n, finish_s, finish_s / (2 * n) * 1e6),
             "| mmg_pairs_create (%d pairs) | %.3f s | %.2f us per pair |" % (N_PAIRS, pass_s, pass_s / N_PAIRS * 1e6), "",
             "Device memory of the pass at its peak: %.1f MB.  Share of pairs with cor < -0.5: %.4f; median |cor|: %.4f."
             % (dev / 1e6, float(np.mean(s["cor"] < -0.5)), float(np.nanmedian(np.abs(s["cor"])))), "",
             "The 58 M-read collapsed file through the CLI: not measured."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.no_write:
        return
    os.makedirs(os.path.dirname(MD), exist_ok=True)
    with open(MD, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
