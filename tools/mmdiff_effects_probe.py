"""What mmdiff's effects cost, at tools/mmdiff_probe.py's workload (F features x N samples, the default 8192 + 16 384 iterations, no
tuning, every = 16: 1024 rows): the sampling phase with effects open next to the untraced sampling phase of another build of the
library (--parent-lib: the parent commit's libmmgibbs.so) and of this one, alternating, `repeats` runs each in a process of its own;
mmg_diff_effects_summarize and mmg_effects_get; the device bytes.  Every time is a host clock around calls that end in a synchronise.
Writes the note --out (profiles/mmdiff_effects_probe.md).
usage: mmdiff_effects_probe.py [--parent-lib PATH] [--out FILE] [F N [repeats]]
       mmdiff_effects_probe.py --one plain|effects F N      (one run, one JSON line: what the tool starts for every measurement)"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BURNIN, ITERS, EVERY = 8192, 16384, 16
PCT = (2.5, 50.0, 97.5)


def one(mode, F, N):
    import numpy as np
    import mmdiff_ref as R
    from mmseq_amd import _lib
    from mmseq_amd.diff import Diff, _effects_out, _ptr
    if mode == "plain":      # the parent's library has no effects entries, and a plain run calls none: they are not bound
        for name in [k for k in _lib.SYMBOLS if "effects" in k]:
            del _lib.SYMBOLS[name]
    rng = np.random.default_rng(5)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, N))
    y[: F // 5, : N // 2] += 1.5
    e = rng.uniform(0.05, 0.5, (F, N))
    M, P0, P1, Cl = R.de_design([N // 2, N - N // 2])
    warm = Diff(y[:64], e[:64], M, P0, P1, Cl)      # the code objects are loaded and the kernels have run once before anything is timed
    if mode == "effects":
        warm.open_effects(1, 8)
    warm.burnin(104)
    warm.sample(8)
    if mode == "effects":
        warm.effects(PCT)
    warm.close()
    d = Diff(y, e, M, P0, P1, Cl)
    base = d.device_bytes()
    out = dict(mode=mode, F=F, N=N, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH))
    if mode == "effects":
        d.open_effects(EVERY, ITERS // EVERY)
        out["rows_device_bytes"] = d.device_bytes() - base
    t0 = time.time()
    d.burnin(BURNIN)
    t1 = time.time()
    d.sample(ITERS)
    t2 = time.time()
    out.update(burnin_s=round(t1 - t0, 4), sample_s=round(t2 - t1, 4), state_device_bytes=base)
    if mode == "effects":
        lib = _lib.load()
        pct = np.array(PCT)
        h = C.c_void_p()
        t0 = time.time()
        _lib.check(lib.mmg_diff_effects_summarize(d._h, len(pct), _ptr(pct), C.byref(h)))
        t1 = time.time()
        fx = _effects_out(lib, h, d.trace_names()[:-1], F, pct)
        t2 = time.time()
        out.update(summarize_s=round(t1 - t0, 4), get_s=round(t2 - t1, 4), effects_device_bytes=fx["device_bytes"], rows=ITERS // EVERY,
                   params=len(fx["names"]), n1_mean=round(float(fx["n"][1].mean()), 1))
    out["gamma_mean"] = round(float(d.results()["gamma_mean"].mean()), 6)
    d.close()
    print(json.dumps(out), flush=True)


def main(argv):
    if argv and argv[0] == "--one":
        return one(argv[1], int(argv[2]), int(argv[3]))
    parent, out_path = None, os.path.join(ROOT, "profiles", "mmdiff_effects_probe.md")
    while argv and argv[0] in ("--parent-lib", "--out"):
        if argv[0] == "--parent-lib":
            parent = os.path.abspath(argv[1])
        else:
            out_path = argv[1]
        argv = argv[2:]
    a = [int(v) for v in argv]
    F, N, reps = (a + [20000, 6, 3][len(a):])[:3]
    runs = [("this build, effects open", "effects", None), ("this build, untraced", "plain", None)]
    if parent:
        runs.append(("parent build, untraced", "plain", parent))
    lines = {name: [] for name, _, _ in runs}
    for rep in range(reps):            # alternating: a drift of the machine touches every variant alike
        for name, mode, lib in runs:
            env = dict(os.environ)
            env.pop("MMSEQ_AMD_LIB", None)
            if lib:
                env["MMSEQ_AMD_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, str(F), str(N)], env=env, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=600)
            if r.returncode != 0:      # a run that fails ends the probe: nothing more is started on the device
                sys.stderr.write(r.stderr.decode()[-2000:])
                return r.returncode
            rec = json.loads(r.stdout.decode().strip().split("\n")[-1])
            print(name, json.dumps(rec), flush=True)
            lines[name].append(rec)
    fx = lines["this build, effects open"]
    assert len({rec["gamma_mean"] for recs in lines.values() for rec in recs}) == 1, "the chains of the variants differ"
    med = lambda v: sorted(v)[len(v) // 2]
    text = ["# mmdiff -effects: recording and summary cost on one MI355X", "",
            "Command: `python tools/mmdiff_effects_probe.py --parent-lib <the parent commit's libmmgibbs.so> %d %d %d`." % (F, N, reps),
            "Workload of `tools/mmdiff_probe.py`: %d features x %d samples, `-de`, %d burn-in and %d sampling iterations, no tuning; effects"
            % (F, N, BURNIN, ITERS),
            "every %d iterations: %d rows of %d parameters and gamma.  Each run is a process of its own, after a warm-up handle of 64"
            % (EVERY, fx[0]["rows"], fx[0]["params"]),
            "features; the variants alternate.  Seconds, host clock around calls that end in a synchronise.", "", "```"]
    for name, _, _ in runs:
        text += ["%s %s" % (name, json.dumps(rec)) for rec in lines[name]]
    text += ["```", "", "| variant | sampling phase, s (runs) | median |", "|---|---|---|"]
    for name, _, _ in runs:
        v = [rec["sample_s"] for rec in lines[name]]
        text.append("| %s | %s | %.3f |" % (name, ", ".join("%.3f" % x for x in v), med(v)))
    text += ["", "* `mmg_diff_effects_summarize`: %s s (median %.4f); `mmg_effects_get` of every array: median %.4f s."
             % (", ".join("%.4f" % rec["summarize_s"] for rec in fx), med([rec["summarize_s"] for rec in fx]), med([rec["get_s"] for rec in fx])),
             "* Device bytes: the handle's state %d, the resident rows and their descriptor %d, the results of the summary %d."
             % (fx[0]["state_device_bytes"], fx[0]["rows_device_bytes"], fx[0]["effects_device_bytes"]),
             "* The mean of gamma over all features is the same in every run (%.6f): recording draws nothing." % fx[0]["gamma_mean"], ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
