#!/usr/bin/env python
"""Times the posterior fold change between two samples (mmg_fold_of_traces) and writes profiles/mmfold_probe.md.

Two rows: 20 000 and 200 000 features x 1024 x 1024 draws, three percentiles (2.5, 50, 97.5) plus the two ranks of gfold 0.01.  The
draws are log-normal, rounded to six significant digits as a trace file holds them; 2000 distinct features are generated and tiled.
One process; after a warm-up handle of 64 features each call runs `--runs` times (default 3) and the table states the median and the
spread (min - max) of the whole call on the host's clock: the checks, the uploads slab by slab, the kernel, the copies back.  No time
is fixed in advance: no earlier figure exists.  The kernel's own device time comes from a second run under the profiler, whose trace
a third call appends:

    python tools/mmfold_probe.py
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/mmfold_probe.py --no-write --runs 1
    python tools/mmfold_probe.py --kernel-csv DIR/.../*_kernel_trace.csv
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd.fold import Fold, percentile_rank  # noqa: E402

MD = os.path.join(ROOT, "profiles", "mmfold_probe.md")
HEAD = "## Kernel times"
S = 1024
SHAPES = (20000, 200000)
DISTINCT = 2000


_BASE = []


def inputs(F):
    if not _BASE:
        rng = np.random.default_rng(1234)
        for shift in (0.0, 0.3):
            x = np.exp(rng.normal(-3.0 + shift, 2.0, DISTINCT)[:, None] + rng.uniform(0.02, 1.0, DISTINCT)[:, None] * rng.normal(0.0, 1.0, (DISTINCT, S)))
            _BASE.append(np.array([float("%.6g" % v) for v in x.ravel()]).reshape(x.shape))
    return tuple(np.ascontiguousarray(np.tile(x, ((F + DISTINCT - 1) // DISTINCT, 1))[:F]) for x in _BASE)


def ranks():
    n = S * S
    return [percentile_rank(p, n) for p in (2.5, 50.0, 97.5, 1.0, 99.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--kernel-csv", nargs="*", default=None)
    args = ap.parse_args()
    if args.kernel_csv is not None:
        return append_kernels(args.kernel_csv)
    rk = ranks()
    a, b = inputs(64)
    Fold.of_traces(a, b, 0.1, rk).close()                      # warm-up: the code object, the first allocations
    rows = []
    for F in SHAPES:
        a, b = inputs(F)
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            h = Fold.of_traces(a, b, 0.1, rk)
            ts.append(time.perf_counter() - t0)
            dev = h.device_bytes()
            s = h.summary()
            h.close()
        assert (s["status"] == 0).all()
        rows.append((F, np.median(ts), min(ts), max(ts), dev, float(np.mean(s["n_eq"] > 0))))
        print("F = %d: %.3f s (%.3f - %.3f), %d runs" % (F, np.median(ts), min(ts), max(ts), args.runs), flush=True)
    if args.no_write:
        return
    with open(MD, "w") as f:
        f.write("# mmfold probe: mmg_fold_of_traces on one MI355X\n\n")
        f.write("Measured by `tools/mmfold_probe.py`: the whole call on the host's clock (checks, uploads slab by slab, the kernel, copies\n"
                "back), median of %d runs after a warm-up handle, spread min - max.  1024 x 1024 draws per feature, five ranks (the percentiles\n"
                "2.5, 50, 97.5 and the two of gfold 0.01), draws with six significant digits.  No speed bar is set: no earlier figure exists.\n\n" % args.runs)
        f.write("| features | pass, s (measured) | spread, s | features / s | peak device bytes | features with ties between the sides |\n|---|---|---|---|---|---|\n")
        for F, med, lo, hi, dev, ties in rows:
            f.write("| %d | %.3f | %.3f - %.3f | %.0f | %d | %.0f %% |\n" % (F, med, lo, hi, F / med, dev, 100 * ties))
        f.write("\nThe input is 16 KiB per feature (two series of 1024 doubles): 200 000 features are 3.3 GB of pageable host memory, uploaded in\n"
                "slabs of 256 MiB; the pass is bounded below by that copy.  The kernel's own time is measured in a profiler run of its own and\n"
                "appended below by `--kernel-csv`; a file without that section has no measured kernel time.\n\n")
    print("wrote", MD)


def append_kernels(paths):
    """the k_fold launches of the profiled run in start order: the warm-up handle's one, then every row's slabs"""
    launches = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                if "k_fold" in (r.get("Kernel_Name") or ""):
                    launches.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    launches = [d for _, d in sorted(launches)]
    cap = (256 << 20) // (8 * 2 * S)
    text = open(MD).read()
    if HEAD in text:
        text = text[:text.index(HEAD)]
    text += HEAD + "\n\nMeasured under `rocprofv3 --kernel-trace` (one run of each row after the warm-up handle; one launch of k_fold per slab of\n" \
                   "%d features): device time, ms.\n\n| features | launches | k_fold total, ms (measured) | longest launch, ms | features / s of kernel time |\n|---|---|---|---|---|\n" % cap
    at = 1
    for F in SHAPES:
        n = (F + cap - 1) // cap
        v = launches[at:at + n]
        at += n
        if len(v) == n:
            text += "| %d | %d | %.2f | %.3f | %.0f |\n" % (F, n, sum(v), max(v), F / (sum(v) / 1e3))
        else:
            text += "| %d | not in the trace | | | |\n" % F
    open(MD, "w").write(text)
    print("appended kernel times to", MD)


if __name__ == "__main__":
    main()
