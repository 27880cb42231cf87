"""Cost of the posterior summary over all chains (mmg_pooled_create) next to mmg_summary_finish (one chain's columns) and
mmg_convergence_create of the same run, at the size of the issue: n transcripts with genes of 1-5 consecutive members, every fifth gene
with an isoform without hits, and some identical pairs; C chains x S kept samples of a synthetic problem (gibbs_iter = trace_len: the
traces fill in about a second).  Every call is timed twice (the first also loads the code object); prints one JSON line per measurement
and writes the table to profiles/pooled_probe.md (or the path given).
usage: pooled_probe.py [n chains samples [out.md]]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from mmseq_amd import gibbs  # noqa: E402

n, C, S = (int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (200000, 4, 1024)
out_md = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "pooled_probe.md")
rng = np.random.default_rng(3)
prob = gibbs.Problem.synthetic(rows=25 * n, n=n, avg_hits=3.0, seed=11, gene_size=4)
mu0, _ = prob.start_values()
s = gibbs.Sampler(prob, mu0, seed=5, n_chains=C, gibbs_iter=S, trace_len=S)
t0 = time.time()
s.run(S)
s.sync()
records = [dict(stage="chain", n=n, chains=C, samples=S, wall_s=round(time.time() - t0, 3))]
print(json.dumps(records[-1]), flush=True)
genes, vid, i = [], [], 0
while i < n:
    sz = int(rng.integers(1, 6))
    ms = list(range(i, min(n, i + sz)))
    if len(genes) % 5 == 0:
        ms.append(n + len(vid))
        vid.append(10 * n + len(vid))
    genes.append(ms)
    i += sz
vscale = rng.uniform(0.01, 2.0, len(vid))
identical = [[j, j + 1] for j in range(0, n - 1, 50)]
desc = dict(virtual_id=vid, virtual_scale=vscale, identical=identical, genes=genes)
series = n + len(vid) + len(genes) + len(identical)
pct1 = [int(round(p / 100.0 * (S - 1))) for p in (5, 25, 50, 75, 95)]
pctN = [int(round(p / 100.0 * (C * S - 1))) for p in (5, 25, 50, 75, 95)]

for rep in range(2):
    q = gibbs.Summary(s, chain=0, percentile_index=pct1, staged=True, **desc)
    q.advance(S)
    t0 = time.time()
    q.finish()
    records.append(dict(stage="mmg_summary_finish (chain 0)", rep=rep, wall_s=round(time.time() - t0, 3), series=series))
    print(json.dumps(records[-1]), flush=True)
    q.close()
for rep in range(2):
    t0 = time.time()
    cv = gibbs.Convergence(s, **desc)
    records.append(dict(stage="mmg_convergence_create", rep=rep, wall_s=round(time.time() - t0, 3), series=series))
    print(json.dumps(records[-1]), flush=True)
    cv.close()
for rep in range(2):
    t0 = time.time()
    ps = gibbs.PooledSummary(s, percentile_index=pctN, **desc)
    dt = time.time() - t0
    r = ps.series(gibbs.SERIES_TRANSCRIPT)
    records.append(dict(stage="mmg_pooled_create", rep=rep, wall_s=round(dt, 3), series=series, device_bytes=ps.device_bytes(),
                        tau_median=float(np.nanmedian(r["tau"])), rc_nonzero=int(np.sum(r["rc"] != 0))))
    print(json.dumps(records[-1]), flush=True)
    ps.close()

with open(out_md, "w") as f:
    f.write("# The summary over all chains next to one chain's summary and the convergence diagnostics\n\n")
    f.write("`tools/pooled_probe.py %d %d %d`: %d transcripts, %d isoforms without hits, %d genes, %d identical sets; %d chains x %d samples.\n"
            "Wall time of each call from Python, two calls each (the first also loads the code object); one run.\n\n" %
            (n, C, S, n, len(vid), len(genes), len(identical), C, S))
    f.write("| call | first (s) | second (s) |\n|---|---|---|\n")
    for stage in ("mmg_summary_finish (chain 0)", "mmg_convergence_create", "mmg_pooled_create"):
        t = [r["wall_s"] for r in records if r["stage"] == stage]
        f.write("| `%s` | %.3f | %.3f |\n" % (stage, t[0], t[1]))
    f.write("\nDevice memory held by `mmg_pooled_create` while it runs: %d bytes.\n" % records[-1]["device_bytes"])
