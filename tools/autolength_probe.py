#!/usr/bin/env python
"""Times what mmseq -gibbs_auto adds and writes profiles/autolength_probe.md.  No time was fixed in advance; three runs, medians.

1. mmg_sampler_extend at 200 000 transcripts x 1 024 samples, 1 and 4 chains (host clock around the call, which waits for the
   sampler's stream, allocates its scratch, runs its kernels and waits again).  Expectation from the code: two streaming passes over
   8 C n S bytes, around a millisecond per chain beside the allocation.
2. The per-stage diagnostics: mmg_convergence_create on the transcripts alone plus the read-out of the three columns, 4 chains.
3. With --hits FILE (a `synth_hits -zipf 1000000 2000000 200000 10 FILE` file: 58 M reads in 2 M hit sets): the CLI end to end,
   `-gibbs_iter 1024 -gibbs_auto 16384` beside a plain `-gibbs_iter 16384` of --parent-bin (the parent commit's mmseq; this build's
   when not given), alternating, with the stage timings (MMSEQ_TIMING=1) of each side's median run.

    python tools/autolength_probe.py [--rows 2000000] [--hits FILE [--parent-bin PATH/mmseq]] [--note FILE ...]

--note FILE: text appended as it is (the comparison of the device assembly with the parent commit, the two bench.py lines)."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd import Problem, Sampler  # noqa: E402
from mmseq_amd import gibbs  # noqa: E402

S, N, REPEATS = 1024, 200_000, 3
MD = os.path.join(ROOT, "profiles", "autolength_probe.md")
MMSEQ = os.path.join(ROOT, "mmseq_amd", "csrc", "mmseq")


def med(v):
    return "%.4f (%s)" % (statistics.median(v), ", ".join("%.4f" % x for x in v))


def library_part(rows):
    prob = Problem.synthetic(rows, N, 20)
    mu0, _ = prob.start_values()
    out = {}
    for chains in (1, 4):
        ext, chain = [], []
        for rep in range(REPEATS + 1):                           # (the first is the warm-up: code object, first allocations)
            s = Sampler(prob, mu0, n_chains=chains, gibbs_iter=S, trace_len=S)
            t0 = time.perf_counter()
            s.run(S)
            s.sync()
            t1 = time.perf_counter()
            s.extend()
            t2 = time.perf_counter()
            if rep:
                chain.append(t1 - t0); ext.append(t2 - t1)
            if chains == 4 and rep == REPEATS:
                s.run(S)                                         # the trace is full again: the diagnostics of a stage
                s.sync()
                diag = []
                for r2 in range(REPEATS + 1):
                    t0 = time.perf_counter()
                    cv = gibbs.Convergence(s)
                    d = cv.series(gibbs.SERIES_TRANSCRIPT)
                    t1 = time.perf_counter()
                    cv.close()
                    if r2:
                        diag.append(t1 - t0)
                out["diag"] = diag
                out["diag_judged"] = int((~(d["rhat"] != d["rhat"])).sum())
            s.close()
        out[chains] = (ext, chain)
    prob.close()
    return out


def timing_lines(stderr):
    return [ln for ln in stderr.decode(errors="replace").split("\n") if ln.startswith("[timing]")]


def cli_part(hits, parent_bin):
    sides = {"auto": [MMSEQ, "-gibbs_iter", "1024", "-gibbs_auto", "16384"], "plain": [parent_bin, "-gibbs_iter", "16384"]}
    wall = {k: [] for k in sides}
    logs = {k: [] for k in sides}
    stages = None
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(REPEATS):
            for side, cmd in sides.items():
                base = os.path.join(tmp, "%s%d" % (side, rep))
                t0 = time.perf_counter()
                r = subprocess.run(cmd + [hits, base], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, MMSEQ_TIMING="1"))
                wall[side].append(time.perf_counter() - t0)
                if r.returncode != 0:
                    raise RuntimeError("%s: exit %d\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
                logs[side].append(timing_lines(r.stderr))
                if side == "auto":
                    stages = open(base + ".autolength").read()
                for f in os.listdir(tmp):
                    os.remove(os.path.join(tmp, f))
    return wall, logs, stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--hits", default="")
    ap.add_argument("--parent-bin", default=MMSEQ)
    ap.add_argument("--note", action="append", default=[])
    args = ap.parse_args()
    lib = library_part(args.rows)
    lines = ["# What mmseq -gibbs_auto adds (tools/autolength_probe.py)", "",
             "%d transcripts x %d kept samples (the generated problem of %d reads); host clock around each call, median of %d runs after a" % (N, S, args.rows, REPEATS),
             "warm-up run (the values in brackets), seconds.", "",
             "| call | seconds |", "|---|---|"]
    for chains in (1, 4):
        ext, chain = lib[chains]
        lines.append("| `mmg_sampler_extend`, %d chain%s: %.2f GB of trace moved through a scratch of %.2f GB, moments rebuilt | %s |"
                     % (chains, "" if chains == 1 else "s", 8e-9 * chains * N * S, 8e-9 * N * S / 2, med(ext)))
        lines.append("| the %d iterations in front of it, %d chain%s | %s |" % (S, chains, "" if chains == 1 else "s", med(chain)))
    lines.append("| a stage's diagnostics, 4 chains: `mmg_convergence_create` on the transcripts alone (no isoforms without hits, identical sets or genes)"
                 " and the three columns read out; %d transcripts judged | %s |" % (lib["diag_judged"], med(lib["diag"])))
    if args.hits:
        wall, logs, stages = cli_part(args.hits, args.parent_bin)
        lines += ["", "## The CLI end to end on the file that collapses (58 M reads in 2 M hit sets, `synth_hits -zipf`), one chain", "",
                  "Alternating runs, wall time of the whole process; `plain` is the parent commit's `mmseq -gibbs_iter 16384`.", "",
                  "| run | seconds |", "|---|---|",
                  "| `mmseq -gibbs_iter 1024 -gibbs_auto 16384` | %s |" % med(wall["auto"]),
                  "| `mmseq -gibbs_iter 16384`, parent commit | %s |" % med(wall["plain"]), "",
                  "`BASE.autolength` of the last run:", "", "```", stages.rstrip("\n"), "```"]
        for side in ("auto", "plain"):
            order = sorted(range(REPEATS), key=lambda i: wall[side][i])
            mid = order[REPEATS // 2]
            lines += ["", "Stage timings of the median %s run (%.3f s):" % (side, wall[side][mid]), "", "```"] + logs[side][mid] + ["```"]
    for path in args.note:
        lines += ["", open(path).read().rstrip("\n")]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(MD), exist_ok=True)
    with open(MD, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
