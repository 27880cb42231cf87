"""Phase timings of mmdiff on the device (mmg_diff_*): burn-in + pseudopriors, the tuning batches, sampling, at F features and N samples
of generated estimates (a -de split in two halves, 20 % of the features shifted by 1.5 in the first half), default iteration counts.
Prints one JSON line per size.
usage: mmdiff_probe.py [F N [burnin iters]] ..."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import mmdiff_ref as R  # noqa: E402
from mmseq_amd.diff import Diff  # noqa: E402


def probe(F, N, burnin=8192, iters=16384):
    rng = np.random.default_rng(5)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, N))
    y[: F // 5, : N // 2] += 1.5
    e = rng.uniform(0.05, 0.5, (F, N))
    M, P0, P1, C = R.de_design([N // 2, N - N // 2])
    t0 = time.time()
    d = Diff(y, e, M, P0, P1, C)
    t1 = time.time()
    d.burnin(burnin)
    t2 = time.time()
    nb = d.tune()
    t3 = time.time()
    d.sample(iters)
    t4 = time.time()
    r = d.results()
    t5 = time.time()
    out = dict(F=F, N=N, burnin=burnin, iters=iters, device_bytes=d.device_bytes(), create_s=round(t1 - t0, 3), burnin_s=round(t2 - t1, 3),
               tune_batches=nb, tune_s=round(t3 - t2, 3), sample_s=round(t4 - t3, 3), results_s=round(t5 - t4, 3),
               us_per_feature_iteration=round((t2 - t1 + t4 - t3) / F / (burnin + iters) * 1e6, 4),
               mean_gamma_planted=round(float(r["gamma_mean"][: F // 5].mean()), 3), mean_gamma_null=round(float(r["gamma_mean"][F // 5:].mean()), 3))
    d.close()
    print(json.dumps(out), flush=True)


args = [int(a) for a in sys.argv[1:]]
sizes = [args[i:i + 2] for i in range(0, len(args), 2)] if args else [[20000, 6], [20000, 24], [200000, 6], [200000, 24]]
for F, N in sizes:
    probe(F, N)
