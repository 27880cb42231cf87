#!/usr/bin/env python
"""Times the contrast pass (mmg_contrast_create) next to mmg_summary_finish of the same run and writes profiles/contrast_probe.md.

The 200 000-transcript generated problem, 1 024 kept samples.  Contrasts: 100 000 of one transcript against one (allele pairs:
consecutive transcripts) plus, per gene of `--gene-size` consecutive transcripts, {first isoform} / {all isoforms}.  The yardstick is
the existing summary: k_contrast_summary does the work of k_series_summary<., true> minus the logarithm, so its time per series
should not exceed that kernel's.  Both passes are run twice; the table gives both repeats, the per-series times and the spread.
The host's clock around the two calls also holds what is not a kernel (the checks and the compaction of the lists on the host, the
allocations, the copies), so the kernels' own times come from a second run under the profiler, whose trace a third call appends:

    python tools/contrast_probe.py [--rows 2000000] [--gene-size 4]
    rocprofv3 --kernel-trace -d DIR -- python tools/contrast_probe.py --no-write
    python tools/contrast_probe.py --kernel-db DIR/.../*_results.db
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd import Contrast, Problem, Sampler  # noqa: E402
from mmseq_amd import gibbs  # noqa: E402

S = 1024
MD = os.path.join(ROOT, "profiles", "contrast_probe.md")
KERNELS = ("k_series_summary", "k_contrast_", "k_transpose", "k_group_sums", "k_proportions", "k_virtual_traces")
HEAD = "## Kernel times"


def kernel_section(db_path):
    """the kernels of the two passes in a rocprofv3 trace of this probe (rocpd: the view `kernels`, durations in ns)"""
    import sqlite3
    rows = sqlite3.connect(db_path).cursor().execute(
        "select name, count(*), sum(duration), sum(grid_x / workgroup_x) from kernels group by name order by sum(duration) desc").fetchall()
    lines = [HEAD + " (a run of this probe under `rocprofv3 --kernel-trace`, both repeats together)", "",
             "The summary kernels run one workgroup per series, so their time per workgroup is their time per series.", "",
             "| kernel | launches | total ms | workgroups | us per workgroup |", "|---|---|---|---|---|"]
    per = {}
    for name, calls, ns, wgs in rows:
        if any(k in name for k in KERNELS):
            lines.append("| `%s` | %d | %.3f | %d | %.3f |" % (name[:100], calls, ns / 1e6, wgs, ns / 1e3 / max(wgs, 1)))
            per[name.split("(")[0].split("::")[-1]] = ns / 1e3 / max(wgs, 1)
    new, old = per.get("k_contrast_summary<1024>"), per.get("k_series_summary<1024, true>")
    if new is not None and old is not None:
        lines += ["", "The yardstick: `k_contrast_summary` %.3f us per series, `k_series_summary<1024, true>` %.3f us (%s)."
                  % (new, old, "not above it" if new <= old else "ABOVE it: the reason has to be found and written here")]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--gene-size", type=int, default=4)
    ap.add_argument("--no-write", action="store_true", help="run the passes and print, but leave profiles/contrast_probe.md (a run under the profiler)")
    ap.add_argument("--kernel-db", default="", help="no run: append the kernel times of this rocprofv3 trace (.db) of the probe to the file")
    args = ap.parse_args()
    if args.kernel_db:
        text = open(MD).read().split(HEAD)[0].rstrip("\n") + "\n\n" + kernel_section(args.kernel_db)
        with open(MD, "w") as f:
            f.write(text)
        print(text)
        return
    n = 200_000
    prob = Problem.synthetic(args.rows, n, 20)
    mu0, _ = prob.start_values()
    smp = Sampler(prob, mu0, gibbs_iter=S, trace_len=S)
    smp.run(S)
    smp.sync()
    genes = [list(range(t, min(n, t + args.gene_size))) for t in range(0, n, args.gene_size)]
    contrasts = [([2 * i], [2 * i + 1]) for i in range(n // 2)] + [([g[0]], g) for g in genes]
    pidx = [int(round(p / 100.0 * (S - 1))) for p in (5, 25, 50, 75, 95)]
    finish_s, pass_s = [], []
    n_series = n + len(genes)                                # the series mmg_summary_finish summarises in log mode
    for _ in range(2):
        q = gibbs.Summary(smp, genes=genes, percentile_index=pidx, staged=True)
        q.advance(S)
        t0 = time.perf_counter()
        q.finish()                                           # transposes + k_series_summary over transcripts and genes + the proportions
        finish_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        with Contrast.from_sampler(smp, q, contrasts, pidx) as h:
            pass_s.append(time.perf_counter() - t0)
            dev = h.device_bytes()
        q.close()
    smp.close()
    prob.close()
    # mmg_summary_finish also summarises the n proportion series (the probit mode of the same kernel): 2 n + genes series in all
    per_finish = [t / (2 * n + len(genes)) * 1e6 for t in finish_s]
    per_pass = [t / len(contrasts) * 1e6 for t in pass_s]
    lines = ["# The contrast pass next to mmg_summary_finish of the same run (tools/contrast_probe.py)", "",
             "%d transcripts, %d kept samples, %d contrasts (%d pairs, %d first-isoform shares of genes of %d); both passes timed on the host,"
             % (n, S, len(contrasts), n // 2, len(genes), args.gene_size),
             "allocations, gathers / transposes and the copy of the results included.", "",
             "| repeat | mmg_summary_finish (%d log series + %d proportion series) | per series | mmg_contrast_create (%d series) | per series |"
             % (n_series, n, len(contrasts)), "|---|---|---|---|---|"]
    for i in range(2):
        lines.append("| %d | %.3f s | %.2f us | %.3f s | %.2f us |" % (i + 1, finish_s[i], per_finish[i], pass_s[i], per_pass[i]))
    spread = max(abs(per_finish[0] - per_finish[1]), abs(per_pass[0] - per_pass[1]))
    lines += ["", "Run-to-run spread of the per-series times: %.2f us.  Device memory the contrast handle keeps: %.1f MB." % (spread, dev / 1e6)]
    if min(per_pass) > max(per_finish) + spread:
        lines += ["", "By the host's clock the contrast pass takes longer per series than the summary, by more than that spread. The clock also covers "
                  "the host's checks and compaction of the lists, the allocations and the copies; the kernels' own times are below."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.no_write:
        return
    os.makedirs(os.path.dirname(MD), exist_ok=True)
    with open(MD, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
