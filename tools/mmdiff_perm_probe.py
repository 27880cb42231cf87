"""What a permutation null costs when it rides in the launches of the observed run, at tools/mmdiff_probe.py's workload (F features x N
samples, the default 8192 + 16 384 iterations, tuning to the reference's stop rule): burn-in, tuning and sampling of a DiffPerm handle
with B shuffled replicas next to the plain run of another build of the library (--parent-lib: the parent commit's libmmgibbs.so) and
next to one plain run on shuffled data (what `-permute` costs once), alternating, `repeats` runs each in a process of its own; the
time of mmg_diff_perm_qvalues and the device bytes.  Every time is a host clock around calls that end in a synchronise.  Writes the
note --out (profiles/mmdiff_perm_probe.md).
usage: mmdiff_perm_probe.py [--parent-lib PATH] [--out FILE] [F N [B [repeats]]]
       mmdiff_perm_probe.py --one plain|permute|perm F N B      (one run, one JSON line: what the tool starts for every measurement)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BURNIN, ITERS, MAXBATCHES = 8192, 16384, 8192


def one(mode, F, N, B):
    import numpy as np
    import mmdiff_ref as R
    from mmseq_amd import _lib
    if mode != "perm":      # the parent's library has no permutation entries, and a plain run calls none: they are not bound
        for name in [k for k in _lib.SYMBOLS if k.startswith("mmg_diff_perm") or k == "mmg_qvalues"]:
            del _lib.SYMBOLS[name]
    from mmseq_amd.diff import Diff, DiffPerm
    rng = np.random.default_rng(5)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, N))
    y[: F // 5, : N // 2] += 1.5
    e = rng.uniform(0.05, 0.5, (F, N))
    if mode == "permute":   # every feature's samples shuffled (numpy's shuffle: the cost of the chain does not depend on which one)
        idx = rng.permuted(np.tile(np.arange(N), (F, 1)), axis=1)
        y, e = np.take_along_axis(y, idx, 1), np.take_along_axis(e, idx, 1)
    design = R.de_design([N // 2, N - N // 2])

    def make(yy, ee):
        return DiffPerm(yy, ee, *design, B) if mode == "perm" else Diff(yy, ee, *design)

    warm = make(y[:64], e[:64])      # the code objects are loaded and the kernels have run once before anything is timed
    warm.burnin(1024)
    warm.tune_batch()
    warm.sample(8)
    if mode == "perm":
        warm.qvalues()
    warm.close()
    t0 = time.time()
    d = make(y, e)
    t1 = time.time()
    d.burnin(BURNIN)
    t2 = time.time()
    nb = d.tune(MAXBATCHES)
    t3 = time.time()
    d.sample(ITERS)
    t4 = time.time()
    out = dict(mode=mode, F=F, N=N, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
               create_s=round(t1 - t0, 4), burnin_s=round(t2 - t1, 4), tune_s=round(t3 - t2, 4), sample_s=round(t4 - t3, 4),
               chain_s=round(t4 - t1, 4), device_bytes=d.device_bytes())
    if mode == "perm":
        t0 = time.time()
        _lib.check(_lib.load().mmg_diff_perm_qvalues(d._h))
        t1 = time.time()
        q = d.qvalues()
        out.update(B=B, tune_batches=nb, qvalues_s=round(t1 - t0, 4), q_below_0_05=int((q["q"] < 0.05).sum()),
                   q_below_0_05_planted=int((q["q"][: F // 5] < 0.05).sum()), gamma_mean=round(float(d.results(0)["gamma_mean"].mean()), 6))
    else:
        out.update(tune_batches=nb, gamma_mean=round(float(d.results()["gamma_mean"].mean()), 6))
    d.close()
    print(json.dumps(out), flush=True)


def main(argv):
    if argv and argv[0] == "--one":
        return one(argv[1], int(argv[2]), int(argv[3]), int(argv[4]))
    parent, out_path = None, os.path.join(ROOT, "profiles", "mmdiff_perm_probe.md")
    while argv and argv[0] in ("--parent-lib", "--out"):
        if argv[0] == "--parent-lib":
            parent = os.path.abspath(argv[1])
        else:
            out_path = argv[1]
        argv = argv[2:]
    a = [int(v) for v in argv]
    F, N, B, reps = (a + [20000, 6, 10, 3][len(a):])[:4]
    runs = [("this build, the data and %d permutations" % B, "perm", None), ("this build, plain", "plain", None),
            ("this build, plain on shuffled data (-permute once)", "permute", None)]
    if parent:
        runs.append(("parent build, plain", "plain", parent))
    lines = {name: [] for name, _, _ in runs}
    for rep in range(reps):            # alternating: a drift of the machine touches every variant alike
        for name, mode, lib in runs:
            env = dict(os.environ)
            env.pop("MMSEQ_AMD_LIB", None)
            if lib:
                env["MMSEQ_AMD_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, str(F), str(N), str(B)], env=env, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=600)
            if r.returncode != 0:      # a run that fails ends the probe: nothing more is started on the device
                sys.stderr.write(r.stderr.decode()[-2000:])
                return r.returncode
            rec = json.loads(r.stdout.decode().strip().split("\n")[-1])
            print(name, json.dumps(rec), flush=True)
            lines[name].append(rec)
    pm = lines[runs[0][0]]
    plain = [rec for name, mode, _ in runs if mode == "plain" for rec in lines[name]]
    assert len({rec["gamma_mean"] for rec in plain + pm}) == 1, "replica 0 is not the plain run"
    med = lambda v: sorted(v)[len(v) // 2]
    text = ["# mmdiff -permutations: what %d shuffled replicas cost in the launches of the observed run, on one MI355X" % B, "",
            "Command: `python tools/mmdiff_perm_probe.py --parent-lib <the parent commit's libmmgibbs.so> %d %d %d %d`." % (F, N, B, reps),
            "Workload of `tools/mmdiff_probe.py`: %d features x %d samples, `-de`, %d burn-in and %d sampling iterations, tuning to the"
            % (F, N, BURNIN, ITERS),
            "reference's stop rule (a replica ends when none of its features is untuned; all stop at %d batches).  Each run is a process of" % MAXBATCHES,
            "its own, after a warm-up handle of 64 features; the variants alternate.  Seconds, host clock around calls that end in a synchronise;",
            "`chain_s` is burn-in + tuning + sampling.", "", "```"]
    for name, _, _ in runs:
        text += ["%s %s" % (name, json.dumps(rec)) for rec in lines[name]]
    text += ["```", "", "| variant | burn-in | tuning (batches) | sampling | burn-in + tuning + sampling (runs) | median |", "|---|---|---|---|---|---|"]
    for name, _, _ in runs:
        recs = lines[name]
        nb = recs[0]["tune_batches"]
        text.append("| %s | %.3f | %.3f (%s) | %.3f | %s | %.3f |" % (
            name, med([r["burnin_s"] for r in recs]), med([r["tune_s"] for r in recs]),
            "%d to %d" % (min(nb), max(nb)) if isinstance(nb, list) else str(nb), med([r["sample_s"] for r in recs]),
            ", ".join("%.3f" % r["chain_s"] for r in recs), med([r["chain_s"] for r in recs])))
    ref = med([r["chain_s"] for r in lines[runs[-1][0] if parent else runs[1][0]]])
    once = med([r["chain_s"] for r in lines[runs[2][0]]])
    mine = med([r["chain_s"] for r in pm])
    text += ["", "* The data and %d permutations in one run: %.2f x the %s plain run, against %.2f x for that run and %d runs of `-permute`"
             % (B, mine / ref, "parent build's" if parent else "same build's", (ref + B * once) / ref, B),
             "  one after the other (medians).",
             "* `mmg_diff_perm_qvalues` (%d x %d statistics, two sorts, the search, the scan): %s s (median %.4f)."
             % (B + 1, F, ", ".join("%.4f" % r["qvalues_s"] for r in pm), med([r["qvalues_s"] for r in pm])),
             "* Device bytes: %d for the handle of %d replicas, %d for the plain handle." % (pm[0]["device_bytes"], B + 1, plain[0]["device_bytes"]),
             "* q < 0.05: %d features, %d of them among the %d planted ones.  The mean of gamma of replica 0 is that of the plain run (%.6f)."
             % (pm[0]["q_below_0_05"], pm[0]["q_below_0_05_planted"], F // 5, pm[0]["gamma_mean"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
