"""Stage timings of mmcollapse on the device: correlations (upload + centring + V + row maxima), the greedy loop, the output stage
(mmg_collapse_summarize), at C candidates and S samples of generated traces; then the CLI end to end on the three-sample fixture of
tests/test_gpu_mmcollapse.py (MMSEQ_TIMING stage lines).  Prints one JSON line per measurement.
usage: mmcollapse_probe.py [C S merges] [workdir]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from mmseq_amd.collapse import Collapse, summarize  # noqa: E402

C, S, M = (int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (20000, 8, 2000)
work = sys.argv[4] if len(sys.argv) > 4 else "/tmp/mmcollapse_probe"
N = 1024
rng = np.random.default_rng(5)
obs = rng.random((C, S)) > 0.05
tr = [rng.gamma(1.0, 1.0, (N, C)) for _ in range(S)]
t0 = time.time()
h = Collapse(tr, obs)
t1 = time.time()
thr = h.threshold(0.975)
t2 = time.time()
pairs, vals, stopped = h.run(thr, max_merges=M)
t3 = time.time()
groups = [[j] for j in range(C)]
lm, var, tau, rc = summarize(tr[0], groups)
t4 = time.time()
print(json.dumps(dict(stage="synthetic", C=C, S=S, device_bytes=h.device_bytes(), correlate_s=round(t1 - t0, 3),
                      threshold_s=round(t2 - t1, 3), merges=int(len(pairs)), stopped=stopped, loop_s=round(t3 - t2, 3),
                      loop_ms_per_merge=round(1e3 * (t3 - t2) / max(1, len(pairs)), 3), summarize_one_sample_s=round(t4 - t3, 3))), flush=True)
h.close()
del tr

import test_gpu_mmcollapse as T  # noqa: E402
from oracle import host_oracle as H  # noqa: E402

os.makedirs(work, exist_ok=True)
bin_dir = os.path.join(ROOT, "mmseq_amd", "csrc")
bases = []
for s in range(3):
    p = os.path.join(work, "s%d.hits" % s)
    open(p, "wb").write(H.write_hits_text(T._families(100 + s)))
    base = os.path.join(work, "s%d" % s)
    subprocess.run([os.path.join(bin_dir, "mmseq"), p, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    bases.append(base)
t0 = time.time()
r = subprocess.run([os.path.join(bin_dir, "mmcollapse")] + bases, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                   env=dict(os.environ, MMSEQ_TIMING="1"))
t1 = time.time()
stages = {ln.split()[1]: float(ln.split()[-2]) for ln in r.stderr.decode().split("\n") if ln.startswith("[timing]") and len(ln.split()) >= 4}
print(json.dumps(dict(stage="cli_fixture", rc=r.returncode, wall_s=round(t1 - t0, 3), timing=stages)), flush=True)
