#!/usr/bin/env python
"""Times mmdiff's likelihood-ratio pass (mmg_diff_lrt_create) next to the chain of the same data and writes profiles/mmdiff_lrt_probe.md.

Three shapes: 20 000 x 6 and 200 000 x 6 with the design of `-de 3 3` (the register instantiation), 20 000 x 24 with `-de 12 12` and
three covariates (the workspace instantiation).  Per shape the pass runs `--runs` times (default 3) and the table states the median
and the spread (min - max) of the whole call, timed on the host: the transposition of y and e, the allocations, the copies, the
kernel, the p- and q-values.  The chain (burn-in 8192, tuning until every feature is tuned or 8192 batches, 16384 sampling
iterations: the CLI's defaults) runs `--chain-runs` times (default 1: it takes up to a minute per run).  No time is fixed in advance.
The kernel's own device time comes from a second run under the profiler, whose trace a third call appends:

    python tools/mmdiff_lrt_probe.py
    rocprofv3 --kernel-trace -d DIR -- python tools/mmdiff_lrt_probe.py --no-write --chain-runs 0
    python tools/mmdiff_lrt_probe.py --kernel-db DIR/.../*_results.db
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd.diff import Diff, DiffLrt  # noqa: E402

MD = os.path.join(ROOT, "profiles", "mmdiff_lrt_probe.md")
HEAD = "## Kernel times"
BURNIN, ITERS = 8192, 16384


def de_design(groups, M):
    N = sum(groups)
    first = np.arange(N) < groups[0]
    return M, np.ones((N, 1)), np.where(first, 0.5, -0.5)[:, None], np.stack([np.zeros(N, np.int64), (~first).astype(np.int64)], 1)


def data(F, N, first, seed):
    rng = np.random.default_rng(seed)
    y = rng.normal(2.0, 1.0, (F, 1)) + rng.normal(0.0, 0.3, (F, N))
    y[:F // 5, :first] += 1.5
    return y, rng.uniform(0.05, 0.5, (F, N))


SHAPES = (
    ("20 000 x 6, -de 3 3", 20000, (3, 3), 0),
    ("200 000 x 6, -de 3 3", 200000, (3, 3), 0),
    ("20 000 x 24, -de 12 12, three covariates", 20000, (12, 12), 3),
)


def stat(ts, unit=1e3):
    ts = sorted(ts)
    return "%.1f (%.1f - %.1f)" % (ts[len(ts) // 2] * unit, ts[0] * unit, ts[-1] * unit) if ts else "not run"


def kernel_section(db_path):
    """the launches of k_lrt in a rocprofv3 trace of this probe (rocpd: the view `kernels`, durations in ns), per instantiation and grid"""
    import sqlite3
    rows = sqlite3.connect(db_path).cursor().execute(
        "select name, grid_x / workgroup_x, duration from kernels where name like '%k_lrt%' order by start").fetchall()
    groups = {}
    for name, wgs, ns in rows:
        groups.setdefault((name, wgs), []).append(ns / 1e9)
    lines = [HEAD + " (one run of this probe under `rocprofv3 --kernel-trace`: device time of each launch)", "",
             "| kernel | workgroups of 64 features | launches | median ms (min - max) |", "|---|---|---|---|"]
    for (name, wgs), ts in groups.items():
        lines.append("| `%s` | %d | %d | %s |" % (name[:60], wgs, len(ts), stat(ts)))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chain-runs", type=int, default=1)
    ap.add_argument("--no-write", action="store_true", help="run and print, but leave profiles/mmdiff_lrt_probe.md (a run under the profiler)")
    ap.add_argument("--kernel-db", default="", help="no run: append the kernel times of this rocprofv3 trace (.db) of the probe to the file")
    args = ap.parse_args()
    if args.kernel_db:
        text = open(MD).read().split(HEAD)[0].rstrip("\n") + "\n\n" + kernel_section(args.kernel_db)
        with open(MD, "w") as f:
            f.write(text)
        print(text)
        return
    lines = ["# mmdiff -lrt next to the chain of the same data (tools/mmdiff_lrt_probe.py)", "",
             "One MI355X.  The pass: the whole mmg_diff_lrt_create call on the host's clock, %d runs, median (min - max).  The chain: burn-in %d,"
             % (args.runs, BURNIN),
             "tuning, %d sampling iterations on the host's clock, %d run(s).  These are the figures of these runs, not bounds." % (ITERS, args.chain_runs), "",
             "| shape | p, classes | the pass, ms | iterations (median, max) | status 1 / 2 / 4 | the chain, s | tuning batches |", "|---|---|---|---|---|---|---|"]
    for label, F, groups, K in SHAPES:
        N = sum(groups)
        M = np.round(np.random.default_rng(K).normal(0.0, 1.0, (N, K)), 3) if K else np.zeros((N, 1))
        M, P0, P1, C = de_design(groups, M)
        y, e = data(F, N, groups[0], F + N)
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            h = DiffLrt(y, e, M, P0, P1, C)
            ts.append(time.perf_counter() - t0)
            r = h.results()
            h.close()
        st = r["status"]
        chain, batches = [], 0
        for _ in range(args.chain_runs):
            t0 = time.perf_counter()
            d = Diff(y, e, M, P0, P1, C)
            d.burnin(BURNIN)
            batches = d.tune()
            d.sample(ITERS)
            d.results()
            chain.append(time.perf_counter() - t0)
            d.close()
        lines.append("| %s | %s, %s | %s | %d, %d | %d / %d / %d | %s | %s |"
                     % (label, r["n_cols"], r["n_classes"], stat(ts), int(np.median(r["iters"])), int(r["iters"].max()), int(((st & 1) != 0).sum()),
                        int(((st & 2) != 0).sum()), int(((st & 4) != 0).sum()), stat(chain, 1.0), batches if chain else "not run"))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.no_write:
        return
    os.makedirs(os.path.dirname(MD), exist_ok=True)
    with open(MD, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
