"""The timeline of ONE launch of the single-chain sample kernel, from the stamps of a -DMMG_K1_STAMPS build (sell_kernels.h):
    python tools/build_variant.py k1stamps 'Makefile::-Wno-unused-value::-Wno-unused-value -DMMG_K1_STAMPS'
    MMSEQ_AMD_LIB=build_ab/lib_k1stamps.so python tools/k1_timeline.py [--rows R --transcripts T --avg A --lean L --range-cost C]
Prints, for the last of --iters launches: resident workgroups over time; the ramp (first entry -> full residency); the tail (first
exit -> last exit, and last moment of full residency -> last exit); the per-workgroup phases (entry -> window in LDS -> last walk ->
exit); and the ranges' durations against their tiles, their groups and their modelled cost, with the least-squares fit
duration = a + b * tiles + c * groups, whose c / b is what a group costs in tiles (the range cost model's 1 / RANGE_TILE_COST, mmgibbs.hip).  The stamps cost time themselves: the output is for the shape of a launch, not its duration."""
import argparse, ctypes, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mmseq_amd import _lib  # noqa: E402
_lib._share_hip_runtime_with_torch()  # the HIP runtime bench.py and the tests run on, before anything loads another (tools/k1_ab.py)
from mmseq_amd import Problem, Sampler, gibbs  # noqa: E402

WORDS = 8
REALTIME_NS = 10.0  # s_memrealtime counts a constant 100 MHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--transcripts", type=int, default=200_000)
    ap.add_argument("--avg", type=float, default=20.0)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--lean", type=int, default=-1, help="MMG_OPT_K1_LEAN")
    ap.add_argument("--range-cost", type=int, default=-1, help="MMG_OPT_K1_RANGE_COST (0: constant per tile)")
    ap.add_argument("--bins", type=int, default=24)
    a = ap.parse_args()
    probe = ctypes.CDLL(_lib.LIB_PATH)
    if not hasattr(probe, "mmg_selftest_k1_stamps"):
        sys.exit("k1_timeline: %s is not a -DMMG_K1_STAMPS build" % _lib.LIB_PATH)
    with gibbs.options(k1_lean=a.lean, k1_range_cost=a.range_cost):
        prob = Problem.synthetic(a.rows, a.transcripts, a.avg, seed=1234)
    inf, k1 = prob.info, prob.k1_info
    grid = inf.sample_grid
    bound, cum, grp = prob.k1_ranges()
    mu0, _ = prob.start_values()
    s = Sampler(prob, mu0, n_chains=1, gibbs_iter=1024, trace_len=1024, keep_trace=False)
    s.run(a.iters)
    s.sync()
    n = min(grid, 1 << 16)
    raw = np.zeros(n * WORDS, np.uint64)
    fn = probe.mmg_selftest_k1_stamps  # (not in the binding table: the diagnostics build's only)
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_ulonglong]
    if fn(raw.ctypes.data, n) != 0:
        sys.exit("k1_timeline: mmg_selftest_k1_stamps failed")
    st = raw.reshape(n, WORDS)
    ok = st[:, 3] != 0
    tiles = (bound[1:] - bound[:-1]).astype(np.float64)[:n]
    groups = (grp[1:] - grp[:-1]).astype(np.float64)[:n]
    cost = (cum[1:] - cum[:-1]).astype(np.float64)[:n]
    print("# K1 timeline: %d rows x %d transcripts, avg %.1f hits; lean %d, fixed walk %d, ranges cut by %s" %
          (a.rows, a.transcripts, a.avg, k1.lean, k1.fixed_walk, "%d per tile + 1 per group" % k1.range_tile_cost if k1.range_tile_cost else "a constant per tile"))
    print("# grid %d workgroups on %d CUs, %d stamped; modelled range cost: max %d, mean %.1f (max / mean %.3f), longest range %d tiles" %
          (grid, inf.cu_count, int(ok.sum()), k1.range_cost_max, k1.range_cost_mean, k1.range_cost_max / max(k1.range_cost_mean, 1e-9), k1.range_tiles_max))
    if not ok.any():
        sys.exit("k1_timeline: no stamps")
    st, tiles, groups, cost = st[ok], tiles[ok], groups[ok], cost[ok]
    t0 = st[:, 4].min()
    ent = (st[:, 4] - t0).astype(np.float64) * REALTIME_NS * 1e-3  # us
    ext = (st[:, 5] - t0).astype(np.float64) * REALTIME_NS * 1e-3
    end = ext.max()
    print("launch: first entry -> last exit %.2f us" % end)
    # resident workgroups over time (sweep over the sorted entries and exits)
    ev = np.concatenate([np.stack([ent, np.ones_like(ent)], 1), np.stack([ext, -np.ones_like(ext)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    res = np.cumsum(ev[:, 1])
    peak = res.max()
    full = 0.98 * peak
    t_full = ev[np.argmax(res >= full), 0]
    last_full = ev[len(res) - 1 - np.argmax(res[::-1] >= full), 0]
    print("residency: peak %d workgroups (%.1f per CU)" % (peak, peak / inf.cu_count))
    print("ramp: first entry -> 98 %% of the peak resident %.2f us; -> the peak itself %.2f us" % (t_full, ev[np.argmax(res >= peak), 0]))
    print("tail: first exit -> last exit %.2f us; last moment at 98 %% of the peak -> last exit %.2f us; last entry -> last exit %.2f us" %
          (end - ext.min(), end - last_full, end - ent.max()))
    idle = np.trapezoid(peak - res, ev[:, 0])
    print("workgroup slots idle over the launch: %.1f %% of peak x duration (ramp part %.1f %%, tail part %.1f %%)" %
          (100 * idle / (peak * end), 100 * np.trapezoid((peak - res)[ev[:, 0] <= t_full], ev[ev[:, 0] <= t_full, 0]) / (peak * end),
           100 * np.trapezoid((peak - res)[ev[:, 0] >= last_full], ev[ev[:, 0] >= last_full, 0]) / (peak * end)))
    print("resident workgroups over time (us from the first entry: mean over the bin)")
    edges = np.linspace(0, end, a.bins + 1)
    for b in range(a.bins):
        m = (ev[:, 0] >= edges[b]) & (ev[:, 0] < edges[b + 1])
        r = res[m].mean() if m.any() else (res[np.searchsorted(ev[:, 0], edges[b]) - 1] if edges[b] > 0 else 0)
        print("  %8.2f - %8.2f  %7.0f  %s" % (edges[b], edges[b + 1], r, "#" * int(round(50 * r / peak))))
    # the phases of a workgroup on its own clock, scaled by its own realtime span
    span_rt = ext - ent
    span_mt = (st[:, 3] - st[:, 0]).astype(np.float64)
    tick_us = np.where(span_mt > 0, span_rt / np.maximum(span_mt, 1), 0)
    good = span_rt >= 1.0  # (10 ns steps: shorter spans give no rate)
    rate = np.median(1.0 / tick_us[good]) if good.any() else float("nan")
    print("s_memtime ticks per us (median over workgroups of >= 1 us): %.1f" % rate)
    ph = np.stack([st[:, 1] - st[:, 0], st[:, 2] - st[:, 1], st[:, 3] - st[:, 2]], 1).astype(np.float64) / rate
    for name, col in (("entry -> first window in LDS", 0), ("-> end of the last walk", 1), ("-> exit (flush of the counts)", 2)):
        q = np.percentile(ph[:, col], [10, 50, 90, 99])
        print("phase %-30s mean %7.2f us   p10 %7.2f  p50 %7.2f  p90 %7.2f  p99 %7.2f" % (name, ph[:, col].mean(), *q))
    fixed = ph[:, 0] + ph[:, 2]
    print("per-workgroup prologue + epilogue: mean %.2f us of a mean range duration of %.2f us (%.1f %%)" %
          (fixed.mean(), span_rt.mean(), 100 * fixed.mean() / span_rt.mean()))
    # durations against the model
    dur = span_rt
    q = np.percentile(dur, [1, 10, 50, 90, 99])
    print("range duration (us): mean %.2f  p1 %.2f  p10 %.2f  p50 %.2f  p90 %.2f  p99 %.2f  max %.2f  (p99 / p50 %.3f)" %
          (dur.mean(), *q, dur.max(), q[4] / q[2]))
    # the last generation sets the tail: the workgroups that entered last
    lastgen = ent >= np.percentile(ent, 100.0 * (1 - min(1.0, peak / len(ent))))
    ql = np.percentile(ext[lastgen], [1, 50, 99])
    print("last generation (the %d workgroups that entered last): exits p1 %.2f  p50 %.2f  p99 %.2f  max %.2f us (spread p99 - p1 %.2f us)" %
          (int(lastgen.sum()), ql[0], ql[1], ql[2], ext[lastgen].max(), ql[2] - ql[0]))
    A = np.stack([np.ones_like(tiles), tiles, groups], 1)
    coef, *_ = np.linalg.lstsq(A, dur, rcond=None)
    pred = A @ coef
    r2 = 1 - ((dur - pred) ** 2).sum() / max(((dur - dur.mean()) ** 2).sum(), 1e-30)
    print("fit duration = %.3f + %.4f * tiles + %.4f * groups us (R^2 %.3f): a group costs %.2f tiles" %
          (coef[0], coef[1], coef[2], r2, coef[2] / coef[1] if coef[1] else float("nan")))
    for name, x in (("tiles", tiles), ("groups", groups), ("modelled cost", cost)):
        c = np.corrcoef(x, dur)[0, 1] if x.std() > 0 else float("nan")
        print("correlation of range duration with %-14s %.3f   (%s per range: min %.0f  mean %.1f  max %.0f)" % (name + ":", c, name, x.min(), x.mean(), x.max()))
    gpt = groups / np.maximum(tiles, 1)
    print("range duration by groups per tile of the range (full-length ranges: at least half the longest)")
    longr = tiles >= 0.5 * tiles.max()
    for lo, hi in ((0, 3), (3, 4), (4, 4.5), (4.5, 5), (5, 5.5), (5.5, 6), (6, 6.5), (6.5, 7), (7, 99)):
        m = longr & (gpt >= lo) & (gpt < hi)
        if m.any():
            print("  groups/tile [%4.1f, %4.1f)  %6d ranges  %6.1f tiles  duration mean %7.2f us  per tile %.4f us" %
                  (lo, hi, int(m.sum()), tiles[m].mean(), dur[m].mean(), (dur[m] / tiles[m]).mean()))
    xcc = (st[:, 7] >> np.uint64(32)).astype(np.int64) & 0xf
    print("workgroups per XCC: " + "  ".join("%d: %d" % (x, int((xcc == x).sum())) for x in np.unique(xcc)))


if __name__ == "__main__":
    main()
