"""Cost of the convergence diagnostics across chains (mmg_convergence_create) at the size of the issue: n transcripts with genes of
1-5 consecutive members and some identical pairs, C chains x S kept samples of a synthetic problem (gibbs_iter = trace_len: the traces
fill in about a second).  Times create() over the transcripts alone and over every level, twice each (the first call also loads the
code object); prints one JSON line per measurement and the scratch bytes the call allocates (the formula of convergence.hip).
usage: convergence_probe.py [n chains samples]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from mmseq_amd import gibbs  # noqa: E402

n, C, S = (int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (200000, 4, 1024)
rng = np.random.default_rng(3)
prob = gibbs.Problem.synthetic(rows=25 * n, n=n, avg_hits=3.0, seed=11, gene_size=4)
mu0, _ = prob.start_values()
s = gibbs.Sampler(prob, mu0, seed=5, n_chains=C, gibbs_iter=S, trace_len=S)
t0 = time.time()
s.run(S)
s.sync()
print(json.dumps(dict(stage="chain", n=n, chains=C, samples=S, wall_s=round(time.time() - t0, 3))), flush=True)
genes, i = [], 0
while i < n:
    sz = int(rng.integers(1, 6))
    genes.append(list(range(i, min(n, i + sz))))
    i += sz
identical = [[j, j + 1] for j in range(0, n - 1, 50)]


def scratch_bytes(count, groups):
    per = C * S * 8
    cap = max(1, min(count, (256 << 20) // per))
    b = cap * per + 3 * cap * 8 + (cap * S * 8 if groups else 0)
    if C * S > 8192:
        p = 2 * C * (S // 2)
        pp = 1 << (p - 1).bit_length()
        b += 2 * pp * 8 * max(1, min(1024, cap, (256 << 20) // (16 * pp)))
    return b


for label, kw, count in (("transcripts", {}, n), ("all_levels", dict(identical=identical, genes=genes), n)):
    for rep in range(2):
        t0 = time.time()
        cv = gibbs.Convergence(s, **kw)
        dt = time.time() - t0
        r = cv.series(gibbs.SERIES_TRANSCRIPT)
        rec = dict(stage=label, rep=rep, create_s=round(dt, 3), series=n + (len(genes) + len(identical) if kw else 0),
                   scratch_bytes=scratch_bytes(count, bool(kw)), rhat_median=float(np.nanmedian(r["rhat"])),
                   ess_bulk_median=float(np.nanmedian(r["ess_bulk"])), ess_tail_median=float(np.nanmedian(r["ess_tail"])),
                   rhat_above_1_01=int(np.sum(r["rhat"] > 1.01)))
        print(json.dumps(rec), flush=True)
        cv.close()
