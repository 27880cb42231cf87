#!/usr/bin/env python
"""Times the isoform-usage pass (mmg_isoform_create, what mmseq -isoforms runs) next to mmg_summary_finish of the same run and
writes profiles/isoforms_probe.md.

The 200 000-transcript generated problem, 1 024 kept samples, 12 127 isoforms without hits spread evenly among the transcripts, all
of them in 70 709 genes of three consecutive members; two thresholds and the five percentile ranks of the CLI.  The whole call is
timed from Python by the host's clock (it ends in a stream synchronise and the copy of the results), three times, medians reported
with the three values beside them; a warm-up call comes first.  The kernels' own times come from a second run under the profiler,
whose trace a third call appends:

    python tools/isoforms_probe.py [--rows 2000000]
    rocprofv3 --kernel-trace -d DIR -- python tools/isoforms_probe.py --no-write
    python tools/isoforms_probe.py --kernel-db DIR/.../*_results.db
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from mmseq_amd import Isoforms, Problem, Sampler  # noqa: E402
from mmseq_amd import gibbs  # noqa: E402

S = 1024
N, NV, GENE = 200_000, 12_127, 3
MD = os.path.join(ROOT, "profiles", "isoforms_probe.md")
KERNELS = ("k_iso_", "k_contrast_gather", "k_series_summary", "k_transpose", "k_group_sums", "k_proportions", "k_virtual_traces")
HEAD = "## Kernel times"
REPEATS = 3


def kernel_section(db_path):
    """the kernels of the two passes in a rocprofv3 trace of this probe (rocpd: the view `kernels`, durations in ns)"""
    import sqlite3
    rows = sqlite3.connect(db_path).cursor().execute(
        "select name, count(*), sum(duration), sum(grid_x / workgroup_x) from kernels group by name order by sum(duration) desc").fetchall()
    lines = [HEAD + " (a run of this probe under `rocprofv3 --kernel-trace`: the warm-up and the %d repeats together)" % REPEATS, "",
             "| kernel | launches | total ms | ms per launch | workgroups | us per workgroup |", "|---|---|---|---|---|---|"]
    for name, calls, ns, wgs in rows:
        if any(k in name for k in KERNELS):
            lines.append("| `%s` | %d | %.3f | %.3f | %d | %.3f |" % (name[:100], calls, ns / 1e6, ns / 1e6 / calls, wgs, ns / 1e3 / max(wgs, 1)))
    return "\n".join(lines) + "\n"


def workload():
    """the members of the genes: transcripts 0 .. N - 1 with the NV isoforms without hits (N + v) spread evenly among them, in threes"""
    at = np.linspace(0, N, NV, endpoint=False).astype(np.int64) + np.arange(NV)     # where the simulated ones sit in the merged list
    members = np.empty(N + NV, np.int64)
    is_virtual = np.zeros(N + NV, bool)
    is_virtual[at] = True
    members[is_virtual] = N + np.arange(NV)
    members[~is_virtual] = np.arange(N)
    assert (N + NV) % GENE == 0
    return members.reshape(-1, GENE).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--no-write", action="store_true", help="run the passes and print, but leave profiles/isoforms_probe.md (a run under the profiler)")
    ap.add_argument("--kernel-db", default="", help="no run: append the kernel times of this rocprofv3 trace (.db) of the probe to the file")
    args = ap.parse_args()
    if args.kernel_db:
        text = open(MD).read().split(HEAD)[0].rstrip("\n") + "\n\n" + kernel_section(args.kernel_db)
        with open(MD, "w") as f:
            f.write(text)
        print(text)
        return
    prob = Problem.synthetic(args.rows, N, 20)
    mu0, _ = prob.start_values()
    smp = Sampler(prob, mu0, gibbs_iter=S, trace_len=S)
    smp.run(S)
    smp.sync()
    genes = workload()
    vid = (N + np.arange(NV)).astype(np.uint64)
    vscale = np.full(NV, 0.5)
    pidx = [int(round(p / 100.0 * (S - 1))) for p in (5, 25, 50, 75, 95)]
    th = [0.1, 0.5]
    finish_s, pass_s, get_s = [], [], []
    for rep in range(REPEATS + 1):                               # (the first is the warm-up: code objects, first allocations)
        q = gibbs.Summary(smp, virtual_id=vid, virtual_scale=vscale, genes=genes, percentile_index=pidx, staged=True)
        q.advance(S)
        t0 = time.perf_counter()
        q.finish()
        t1 = time.perf_counter()
        with Isoforms.from_sampler(smp, q, genes, th, pidx) as h:
            t2 = time.perf_counter()
            grp = h.groups()
            t3 = time.perf_counter()
            dev = h.device_bytes()
        q.close()
        if rep:
            finish_s.append(t1 - t0); pass_s.append(t2 - t1); get_s.append(t3 - t2)
    smp.close()
    prob.close()
    assert (grp["status"] == 0).all()
    fmt = lambda v: "%.4f (%s)" % (statistics.median(v), ", ".join("%.4f" % x for x in v))
    lines = ["# The isoform-usage pass next to mmg_summary_finish of the same run (tools/isoforms_probe.py)", "",
             "%d transcripts and %d isoforms without hits in %d genes of %d, %d kept samples, thresholds %s, %d ranks; host clock around each call,"
             % (N, NV, len(genes), GENE, S, th, len(pidx)),
             "median of %d repeats after a warm-up call (the three values in brackets), seconds." % REPEATS, "",
             "| call | seconds |", "|---|---|",
             "| `mmg_summary_finish` (%d log series + %d proportion series) | %s |" % (N + NV + len(genes), N + NV, fmt(finish_s)),
             "| `Isoforms.from_sampler` = `mmg_isoform_create` (checks, slab cut, gather, both kernels, copies) | %s |" % fmt(pass_s),
             "| `Isoforms.groups()` (host only: two getters and the derived columns) | %s |" % fmt(get_s), "",
             "Device memory the handle keeps: %.1f MB.  Mean entropy over the genes %.3f, mean top share %.3f." % (dev / 1e6, grp["mean_H"].mean(),
                                                                                                             grp["mean_P"].mean())]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.no_write:
        return
    os.makedirs(os.path.dirname(MD), exist_ok=True)
    with open(MD, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
