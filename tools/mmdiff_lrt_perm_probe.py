#!/usr/bin/env python
"""Times mmdiff's permutation null of the likelihood-ratio test (mmg_diff_lrt_perm_create) next to B plain passes
(mmg_diff_lrt_create) on the same data and writes profiles/mmdiff_lrt_perm_probe.md.

Four rows: 20 000 x 6 with the design of `-de 3 3` at B = 100 and B = 1000, 200 000 x 6 at B = 100 (the register instantiation),
20 000 x 24 with `-de 12 12` and three covariates at B = 100 (the workspace instantiation).  One process; after a warm-up handle of 64
features each call runs `--runs` times (default 3) and the table states the median and the spread (min - max) of the whole call on
the host's clock: the checks, the transposition, the allocations, the copies, the kernels, the q-values, the copy back of the
B x F statistics.  The plain pass is timed the same way: through this build, or with `--parent-lib` (the libmmgibbs.so of the parent
commit) in a child process of its own that loads that library alone and runs before this one touches the device; the table says
which.  No time is fixed in advance.  The kernels' own device time comes from a
second run under the profiler, whose trace a third call appends:

    python tools/mmdiff_lrt_perm_probe.py [--parent-lib PATH]
    rocprofv3 --kernel-trace -d DIR -- python tools/mmdiff_lrt_perm_probe.py --no-write --runs 1
    python tools/mmdiff_lrt_perm_probe.py --kernel-db DIR/.../*_results.db

and the counters of k_lrt_perm from counter-only runs (no tracing beside them; at most 8 SQ counters, or 4 TCC and 2 GRBM, per run)
of the rows at B = 100, which a last call appends:

    rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU \
        SQ_THREAD_CYCLES_VALU --output-format csv -d DIR1 -- python tools/mmdiff_lrt_perm_probe.py --no-write --runs 1 --rows 0 3
    rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum --output-format csv -d DIR2 -- python ... (the same)
    python tools/mmdiff_lrt_perm_probe.py --counters-csv DIR1/.../*_counter_collection.csv DIR2/.../*_counter_collection.csv
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmseq_amd import _lib  # noqa: E402
from mmseq_amd.diff import DiffLrt, DiffLrtPerm  # noqa: E402
from mmdiff_lrt_probe import data, de_design, stat  # noqa: E402

MD = os.path.join(ROOT, "profiles", "mmdiff_lrt_perm_probe.md")
HEAD = "## Kernel times"
COUNTERS = "## Counters"
SEED = 1234

SHAPES = (
    ("20 000 x 6, -de 3 3", 20000, (3, 3), 0, 100),
    ("20 000 x 6, -de 3 3", 20000, (3, 3), 0, 1000),
    ("200 000 x 6, -de 3 3", 200000, (3, 3), 0, 100),
    ("20 000 x 24, -de 12 12, three covariates", 20000, (12, 12), 3, 100),
)


def plain_pass(lib, y, e, M, P0, P1, Cl):
    """seconds of one mmg_diff_lrt_create of `lib` (a ctypes library: this build's or the parent commit's), the handle destroyed outside"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    F, N = y.shape
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = lib.mmg_diff_lrt_create(0, F, N, p(y), p(e), M.shape[1], p(M), P0.shape[1], p(P0), P1.shape[1], p(P1), p(Cl), 0, 0, C.byref(h))
    t = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError("mmg_diff_lrt_create returned %d" % rc)
    lib.mmg_diff_lrt_destroy(h)
    return t


def load_plain(path):
    if not path:
        return _lib.load()
    lib = C.CDLL(path)
    for name in ("mmg_diff_lrt_create", "mmg_diff_lrt_destroy"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


def shape_inputs(F, groups, K):
    N = sum(groups)
    M = np.round(np.random.default_rng(K).normal(0.0, 1.0, (N, K)), 3) if K else np.zeros((N, 1))
    M, P0, P1, Cl = de_design(groups, M)
    y, e = data(F, N, groups[0], F + N)
    return y, e, M, P0, np.ascontiguousarray(P1), np.ascontiguousarray(Cl, np.int32)


def plain_times(lib, runs):
    """per row of SHAPES the seconds of `runs` plain passes, after one warm-up pass on 64 features"""
    plain_pass(lib, *shape_inputs(64, (3, 3), 0))
    out = []
    for _, F, groups, K, _ in SHAPES:
        inputs = shape_inputs(F, groups, K)
        out.append([plain_pass(lib, *inputs) for _ in range(runs)])
    return out


def kernel_section(db_path):
    """the launches of k_lrt_perm and k_lrt_perm_count in a rocprofv3 trace of this probe (rocpd: the view `kernels`, durations in ns),
    per instantiation and grid; a row of the table above is the launches of one grid (its slabs) in one call"""
    import sqlite3
    rows = sqlite3.connect(db_path).cursor().execute(
        "select name, grid_x / workgroup_x, grid_y, duration from kernels where name like '%k_lrt%' order by start").fetchall()
    groups = {}
    for name, wgs, copies, ns in rows:
        groups.setdefault((name, wgs, copies), []).append(ns / 1e9)
    lines = [HEAD + " (one run of this probe under `rocprofv3 --kernel-trace --runs 1`: device time of each launch)", "",
             "| kernel | workgroups of 64 features | grid.y (copies of the slab) | launches | median ms (min - max) | sum ms |", "|---|---|---|---|---|---|"]
    for (name, wgs, copies), ts in groups.items():
        lines.append("| `%s` | %d | %d | %d | %s | %.1f |" % (name[:40], wgs, copies, len(ts), stat(ts), sum(ts) * 1e3))
    return "\n".join(lines) + "\n"


def counters_section(paths):
    """the counters of every k_lrt_perm launch in rocprofv3 --pmc csv files of this probe, one line per launch (launches are matched
    across files by kernel, grid and order), and the two ratios read from them"""
    import csv
    launches = {}
    for path in paths:
        seen = {}
        for r in csv.DictReader(open(path)):
            if "k_lrt_perm<" not in r["Kernel_Name"]:
                continue
            kg = (r["Kernel_Name"].split("(")[0].replace("void ", ""), int(r["Grid_Size"]) // int(r["Workgroup_Size"]))
            nth = seen.setdefault(kg, {}).setdefault(r["Dispatch_Id"], len(seen[kg]))
            launches.setdefault(kg + (nth,), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    lines = [COUNTERS + " (`rocprofv3 --pmc`, counter-only runs of the rows at B = 100; sums over the chip)", "",
             "| kernel | workgroups | counters | active lanes per VALU cycle | waiting / issuing / stalled share of wave cycles | L2 hit share |",
             "|---|---|---|---|---|---|"]
    for (name, wgs, _), c in launches.items():
        g = lambda k: c.get(k, float("nan"))
        lanes = g("SQ_THREAD_CYCLES_VALU") / g("SQ_ACTIVE_INST_VALU")
        wc = g("SQ_WAVE_CYCLES")
        shares = "%.0f %% / %.0f %% / %.0f %%" % (100 * g("SQ_WAIT_ANY") / wc, 100 * g("SQ_ACTIVE_INST_ANY") / wc, 100 * g("SQ_WAIT_INST_ANY") / wc)
        hit = 100 * g("TCC_HIT_sum") / (g("TCC_HIT_sum") + g("TCC_MISS_sum"))
        lines.append("| `%s` | %d | %s | %.1f of 64 | %s | %.1f %% |"
                     % (name, wgs, ", ".join("%s %.4g" % kv for kv in sorted(c.items())), lanes, shares, hit))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="time the plain pass through this libmmgibbs.so (the parent commit's build)")
    ap.add_argument("--plain-child", default="", help="(what --parent-lib starts) time the plain passes through this library alone, print JSON")
    ap.add_argument("--no-write", action="store_true", help="run and print, but leave profiles/mmdiff_lrt_perm_probe.md (a run under the profiler)")
    ap.add_argument("--kernel-db", default="", help="no run: append the kernel times of this rocprofv3 trace (.db) of the probe to the file")
    ap.add_argument("--counters-csv", nargs="*", default=[], help="no run: append the counters of these rocprofv3 --pmc csv files of the probe to the file")
    ap.add_argument("--rows", type=int, nargs="*", default=list(range(len(SHAPES))), help="the rows of the table to run (default: all)")
    args = ap.parse_args()
    if args.counters_csv:
        text = open(MD).read().split(COUNTERS)[0].rstrip("\n") + "\n\n" + counters_section(args.counters_csv)
        with open(MD, "w") as f:
            f.write(text)
        print(text)
        return
    if args.kernel_db:
        text = open(MD).read().split(HEAD)[0].rstrip("\n") + "\n\n" + kernel_section(args.kernel_db)
        with open(MD, "w") as f:
            f.write(text)
        print(text)
        return
    if args.plain_child:
        print(json.dumps(plain_times(load_plain(args.plain_child), args.runs)))
        return
    if args.parent_lib:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", args.parent_lib, "--runs", str(args.runs)],
                               stdout=subprocess.PIPE, check=True, timeout=600)
        plain = json.loads(child.stdout.decode().strip().split("\n")[-1])
    else:
        plain = plain_times(_lib.load(), args.runs)
    which = "the parent commit's build, in a process of its own" if args.parent_lib else "this build"
    # warm-up: code objects, the allocator, the sorts
    M, P0, P1, Cl = de_design((3, 3), np.zeros((6, 1)))
    y, e = data(64, 6, 3, 1)
    DiffLrtPerm(y, e, M, P0, P1, Cl, 2).close()
    DiffLrt(y, e, M, P0, P1, Cl).close()
    lines = ["# mmdiff -lrt -lrtperm B next to B plain passes on the same data (tools/mmdiff_lrt_perm_probe.py)", "",
             "One MI355X, one process.  `the null`: the whole mmg_diff_lrt_perm_create call (the observed test, B shuffled copies, the counts, the",
             "q-values, the copy back) on the host's clock, %d runs, median (min - max).  `one pass`: the whole mmg_diff_lrt_create call of %s" % (args.runs, which),
             "on the same data, timed the same way; `B passes` is B times its median.  Status bits: over the 2 B F fits of the copies.",
             "These are the figures of these runs, not bounds.", "",
             "| shape | B | p, classes | copies per slab | the null, ms | one pass, ms | B passes, ms | B passes / the null | status 1 / 2 / 4 of 2 B F fits | device MiB |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for row, ((label, F, groups, K, B), ps) in enumerate(zip(SHAPES, plain)):
        if row not in args.rows:
            continue
        N = sum(groups)
        y, e, M, P0, P1, Cl = shape_inputs(F, groups, K)
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            h = DiffLrtPerm(y, e, M, P0, P1, Cl, B, seed=SEED)
            ts.append(time.perf_counter() - t0)
            r = h.results()
            nbytes = h.device_bytes()
            h.close()
        st = r["null_status"]
        bits = [int(((st >> k) & 1).sum() + ((st >> (4 + k)) & 1).sum()) for k in range(3)]
        p, nc = r["n_cols"], r["n_classes"]
        wslots = 3 * max(nc) + (0 if max(p) <= 4 else max(p) * (max(p) + 1) // 2 + max(p))
        Sc = min(max((1 << 30) // (8 * F * (2 * N + wslots)), 1), B)
        one = sorted(ps)[len(ps) // 2]
        lines.append("| %s | %d | %s, %s | %d | %s | %s | %.1f | %.1f | %d / %d / %d of %d | %.1f |"
                     % (label, B, p, nc, Sc, stat(ts), stat(ps), B * one * 1e3, B * one / sorted(ts)[len(ts) // 2], bits[0], bits[1], bits[2],
                        2 * st.size, nbytes / 2.0 ** 20))
        print(lines[-1], flush=True)
        del r, st
    text = "\n".join(lines) + "\n"
    print(text)
    if args.no_write:
        return
    os.makedirs(os.path.dirname(MD), exist_ok=True)
    with open(MD, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
