#!/usr/bin/env python
"""Times the posterior distances and correlations between samples (mmg_sim_*) and writes profiles/mmsim_probe.md.

Four rows: 20 000 and 200 000 features with S = 6 and S = 24 samples, T = 1 024 joint draws, three ranks (the percentiles 2.5, 50,
97.5), the centre on the features' means.  The draws are log-normal around two profiles, rounded to six significant digits as a trace
file holds them; 2000 distinct features are generated and tiled, and two host traces serve all the samples in turn (with their own
offsets).  One process; after a warm-up handle each row runs `--runs` times (default 3) and the table states the medians on the
host's clock of: all the set_sample calls (upload from pageable memory + prepare), run() (used features, Gram, reduce, summary) and
the whole call from creation to the summary.  No time is fixed in advance: no earlier figure exists.  The same call then times run()
at 200 000 features for several chunk lengths of the Gram kernel (MMG_OPT_SIM_CHUNK; 100 000 is two chunks a draw) beside the
default, which is what every other figure is measured at.  The kernels' own device times come from a second run under the profiler,
whose trace a third call appends:

    python tools/mmsim_probe.py
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/mmsim_probe.py --no-write --runs 1
    python tools/mmsim_probe.py --kernel-csv DIR/.../*_kernel_trace.csv
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd.similarity import Similarity, percentile_rank  # noqa: E402

MD = os.path.join(ROOT, "profiles", "mmsim_probe.md")
HEAD = "## Kernel times"
T = 1024
SHAPES = ((6, 20000), (24, 20000), (6, 200000), (24, 200000))
DISTINCT = 2000
CHUNKS = (256, 1024, 4096, 16384, 100000)
CHUNK_F = 200000
KERNELS = ("k_sim_prepare", "k_sim_used", "k_sim_zero", "k_sim_gram", "k_sim_reduce", "k_sim_pair", "k_sim_nn")

_BASE = []


def inputs(F):
    """two host traces (T, F) and the features' centre"""
    if not _BASE:
        rng = np.random.default_rng(1234)
        prof = rng.normal(-3.0, 2.0, DISTINCT)
        for shift in (0.0, 0.3):
            x = np.exp((prof + shift * rng.normal(0.0, 1.0, DISTINCT))[None, :] + 0.2 * rng.normal(0.0, 1.0, (T, DISTINCT)))
            _BASE.append(np.array([float("%.6g" % v) for v in x.ravel()]).reshape(x.shape))
        _BASE.append(prof)
    rep = (F + DISTINCT - 1) // DISTINCT
    return [np.ascontiguousarray(np.tile(x, (1, rep))[:, :F]) for x in _BASE[:2]], np.tile(_BASE[2], rep)[:F]


def one(S, F, traces, centre, ranks):
    t0 = time.perf_counter()
    with Similarity(S, F, T, centre=centre) as h:
        t1 = time.perf_counter()
        for s in range(S):
            h.set_sample(s, traces[s & 1], 0.01 * s)
        t2 = time.perf_counter()
        h.run(ranks)
        t3 = time.perf_counter()
        out = h.summary()
        _, n = h.used()
        dev = h.device_bytes()
    t4 = time.perf_counter()
    assert out["status"] == 0 and n == F
    return dict(create=t1 - t0, set=t2 - t1, run=t3 - t2, whole=t4 - t0, dev=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--kernel-csv", nargs="*", default=None)
    args = ap.parse_args()
    if args.kernel_csv is not None:
        return append_kernels(args.kernel_csv)
    ranks = [percentile_rank(p, T) for p in (2.5, 50.0, 97.5)]
    traces, centre = inputs(64)
    one(2, 64, traces, centre, ranks)                          # warm-up: the code object, the first allocations
    rows = []
    for F in sorted(set(f for _, f in SHAPES)):
        traces, centre = inputs(F)
        for S in [s for s, f in SHAPES if f == F]:
            r = [one(S, F, traces, centre, ranks) for _ in range(args.runs)]
            med = {k: float(np.median([x[k] for x in r])) for k in r[0]}
            med["create_range"] = (min(x["create"] for x in r), max(x["create"] for x in r))
            rows.append((S, F, med))
            print("S = %d, F = %d: set_sample %.3f s, run %.3f s, whole %.3f s (create: %s)" % (S, F, med["set"], med["run"], med["whole"],
                                                                                              " ".join("%.3f" % x["create"] for x in r)), flush=True)
    if args.no_write:
        return
    from mmseq_amd import gibbs
    by_chunk = []                                              # (chunk length or None for the default, {S: run and device bytes})
    traces, centre = inputs(CHUNK_F)
    for ch in (None,) + CHUNKS:
        per = {}
        with gibbs.options(**({} if ch is None else dict(sim_chunk=ch))):
            for S in sorted(set(s for s, f in SHAPES if f == CHUNK_F)):
                r = [one(S, CHUNK_F, traces, centre, ranks) for _ in range(args.runs)]
                per[S] = (float(np.median([x["run"] for x in r])), r[0]["dev"])
        by_chunk.append((ch, per))
        print("chunk %s: %s" % (ch, ", ".join("S = %d run %.4f s" % (S, v[0]) for S, v in per.items())), flush=True)
    with open(MD, "w") as f:
        f.write("# mmsim probe: mmg_sim_* on one MI355X\n\n")
        f.write("Measured by `tools/mmsim_probe.py` on the host's clock, medians of %d runs after a warm-up handle.  T = 1024 joint draws,\n"
                "three ranks, the centre on the features' means, draws with six significant digits.  `set_sample`: all S calls, each the upload\n"
                "of 8 T F bytes from pageable memory and the prepare kernel.  `run`: used features, Gram, reduce, summary and the copies back.\n"
                "`create` is given as its least and greatest time, and the whole call also with the least (the median less the median create plus\n"
                "the least): on some visits the first handles of a large size took up to 1.7 s to create, the later ones 1 ms.  No speed bar is\n"
                "set: no earlier figure exists.\n\n" % args.runs)
        f.write("| S | features | create, s | set_sample, s | upload rate, GB/s | run, s | whole call, s | whole call with the least create, s | device bytes |\n|---|---|---|---|---|---|---|---|---|\n")
        for S, F, m in rows:
            f.write("| %d | %d | %.3f to %.3f | %.3f | %.1f | %.4f | %.3f | %.3f | %d |\n" % (
                S, F, m["create_range"][0], m["create_range"][1], m["set"], 8.0 * S * T * F / m["set"] / 1e9, m["run"], m["whole"],
                m["whole"] - m["create"] + m["create_range"][0], int(m["dev"])))
        sizes = sorted(by_chunk[0][1])
        f.write("\n## Chunk length\n\n`run`, s, at %d features with `MMG_OPT_SIM_CHUNK` features per chunk of the Gram kernel (medians of %d runs in the same process;\n"
                "`run` holds the Gram kernel, the reduction over the chunks and the summary).  The first row is the library's own choice.\n\n" % (CHUNK_F, args.runs))
        f.write("| features per chunk | chunks | " + " | ".join("run, s, S = %d | device bytes, S = %d" % (S, S) for S in sizes) + " |\n|---|---|" + "---|---|" * len(sizes) + "\n")
        for ch, per in by_chunk:
            f.write("| %s | %s | " % ("default" if ch is None else ch, "" if ch is None else (CHUNK_F + ch - 1) // ch) +
                    " | ".join("%.4f | %d" % (per[S][0], int(per[S][1])) for S in sizes) + " |\n")
        f.write("\nThe kernels' own times are measured in a profiler run of its own and appended below by `--kernel-csv`; a file without that\n"
                "section has no measured kernel time.\n\n")
    print("wrote", MD)


def append_kernels(paths):
    """the launches of the profiled run in start order: the warm-up handle's first, then every row's (S prepares, then one of each
    kernel of run(); k_sim_zero only when a feature is unused, which the probe's inputs never have)"""
    launches = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name") or ""
                for k in KERNELS:
                    if k in name:
                        launches.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    launches.sort()
    order = [(S, F) for F in sorted(set(f for _, f in SHAPES)) for S in [s for s, f in SHAPES if f == F]]
    per = {}
    at = {k: 0 for k in KERNELS}
    seq = {k: [d for _, kk, d in launches if kk == k] for k in KERNELS}
    for S, F in [(2, 64)] + order:                             # (the warm-up handle comes first)
        row = {}
        for k in KERNELS:
            cnt = S if k == "k_sim_prepare" else 0 if k == "k_sim_zero" else 1
            v = seq[k][at[k]:at[k] + cnt]
            at[k] += cnt
            row[k] = sum(v) if len(v) == cnt else None
        per[(S, F)] = row
    text = open(MD).read()
    if HEAD in text:
        text = text[:text.index(HEAD)]
    text += HEAD + "\n\nMeasured under `rocprofv3 --kernel-trace` (one run of each row after the warm-up handle): device time, ms.  The Gram kernel's\n" \
                   "rate counts the bytes of z once, 8 S T F.\n\n" \
                   "| S | features | k_sim_prepare (S launches) | k_sim_used | k_sim_gram | Gram, GB/s | k_sim_reduce | k_sim_pair | k_sim_nn |\n|---|---|---|---|---|---|---|---|---|\n"
    for S, F in order:
        r = per[(S, F)]
        if any(r[k] is None for k in KERNELS):
            text += "| %d | %d | not in the trace | | | | | | |\n" % (S, F)
            continue
        text += "| %d | %d | %.2f | %.3f | %.2f | %.0f | %.3f | %.3f | %.3f |\n" % (
            S, F, r["k_sim_prepare"], r["k_sim_used"], r["k_sim_gram"], 8.0 * S * T * F / (r["k_sim_gram"] / 1e3) / 1e9, r["k_sim_reduce"], r["k_sim_pair"],
            r["k_sim_nn"])
    open(MD, "w").write(text)
    print("appended kernel times to", MD)


if __name__ == "__main__":
    main()
