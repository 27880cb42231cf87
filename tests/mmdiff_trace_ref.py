"""numpy restatement of mmdiff's trace files (the reference's -tracedir: BMS::initialise_streams, print, printtune, print_pseudo of
src/bms.cpp, driven as src/mmdiff.cpp:733-862) on top of tests/mmdiff_ref.py, which it does not change: a BMS that keeps the state
after the recorded iterations, the tuning rows, the pseudoprior table, and the writer of the files."""
import numpy as np

import mmdiff_ref as R


def param_names(K, L, nc):
    """BMS::initialise_streams' order, gamma last."""
    names = ["alpha0", "alpha1"]
    names += ["beta%d_%d" % (m, i) for m in range(2) for i in range(K)]
    names += ["eta%d_%d" % (m, l) for m in range(2) for l in range(L[m])]
    names += ["lambda%d_%d" % (m, l) for m in range(2) for l in range(L[m])]
    names += ["sigmasq%d_%d" % (m, c) for m in range(2) for c in range(nc[m])]
    return names + ["rho0", "rho1", "gamma"]


class TracedBMS(R.BMS):
    """R.BMS recording the state after every every_burnin-th burn-in iteration and every every_sample-th sampling iteration (counted
    from the first sampling iteration): rows[phase] is a list of (P, F) arrays, gamma (as 0.0 / 1.0) the last slot of sampling rows."""

    def __init__(self, *args, every_burnin=1, every_sample=1, **kw):
        super().__init__(*args, **kw)
        self.every = (int(every_burnin), int(every_sample))
        self.rows = ([], [])
        self.tune_rows = []          # (meanLO, logitp) before tuning batch b = 1, 2, ...
        self._phase = None
        self._tt = 0

    def names(self):
        return param_names(self.K, self.L, self.nc)

    def snapshot(self, phase):
        st = self.st
        cols = [st[0]["alpha"], st[1]["alpha"]]
        for key, n in (("beta", (self.K, self.K)), ("eta", self.L), ("lam", self.L), ("sig", self.nc)):
            for m in range(2):
                cols += [st[m][key][:, i] for i in range(n[m])]
        cols += [st[0]["rho"], st[1]["rho"]]
        if phase:
            cols.append(self.gam.astype(np.float64))
        return np.stack([np.array(c, np.float64) for c in cols])

    def iteration(self, lanes, it, inburnin, rec):
        super().iteration(lanes, it, inburnin, rec)
        if self._phase is None:
            return
        if self._tt % self.every[self._phase] == 0:
            self.rows[self._phase].append(self.snapshot(self._phase))
        self._tt += 1

    def burnin(self, iters):
        self._phase, self._tt = 0, 0
        super().burnin(iters)
        self._phase = None

    def sample(self, iters):
        self._phase, self._tt = 1, self.sampled
        super().sample(iters)
        self._phase = None

    def tune_state(self):
        """What BMS::printtune prints: LOsum / 128 and logit p' as they stand."""
        return self.LOsum / float(R.BATCH), self.logitp.copy()

    def tune_batch(self):
        if self.batches > 0:
            self.tune_rows.append(self.tune_state())
        return super().tune_batch()

    def pseudo(self):
        """The columns of BMS::print_pseudo, (Q, F)."""
        cols = []
        for m in range(2):
            S = self.st[m]
            cols += [S["A"], S["Va"]]
            for k in range(self.K):
                cols += [S["B"][:, k], S["Vb"][:, k]]
            for l in range(self.L[m]):
                cols += [S["Fm"][:, l], S["Ve"][:, l], 1.0 / S["Si"][:, l]]
            for c in range(self.nc[m]):
                cols += [S["J"][:, c], S["Lm"][:, c]]
            cols += [S["Q"], S["R"]]
        return np.stack([np.array(c, np.float64) for c in cols])

    def stacked(self, phase):
        P = len(self.names()) - (0 if phase else 1)
        return np.stack(self.rows[phase]) if self.rows[phase] else np.empty((0, P, self.F))


def pseudo_header(K, L, nc):
    out = ""
    for m in range(2):
        out += "A%d\tValpha%d\t" % (m, m)
        out += "".join("B%d_%d\tVbeta%d_%d\t" % (m, l, m, l) for l in range(K))
        out += "".join("F%d_%d\tVeta%d_%d\tS%d_%d\t" % (m, l, m, l, m, l) for l in range(L[m]))
        out += "".join("J%d_%d\tL%d_%d\t" % (m, c, m, c) for c in range(nc[m]))
        out += "Q%d\tR%d\t" % (m, m)
    return out + "\n"


def line(values, as_int=False):
    return "".join(("%d " % int(v)) if as_int else R.fmt(v) + " " for v in values) + "\n"


def trace_files(names, burn_rows, samp_rows, tune_rows, pseudo, K, L, nc):
    """name -> text of every file in the trace directory.  burn_rows (Rb, P - 1, F), samp_rows (Rs, P, F), tune_rows a list of
    (meanLO, logitp), pseudo (Q, F).  print() ends a line in every stream but logitp (and gamma in burn-in), so meanLO-burnin and meanLO
    get an empty line per recorded iteration; sigar<model>.txt is not written."""
    files = {}
    for s, name in enumerate(names[:-1]):
        files[name + "-burnin"] = "".join(line(r[s]) for r in burn_rows)
    files["gamma-burnin"] = ""
    files["logitp-burnin"] = ""
    files["meanLO-burnin"] = "\n" * len(burn_rows)
    for s, name in enumerate(names):
        files[name] = "".join(line(r[s], as_int=(name == "gamma")) for r in samp_rows)
    files["logitp"] = "".join(line(lp) for _, lp in tune_rows)
    files["meanLO"] = "".join(line(lo) for lo, _ in tune_rows) + "\n" * len(samp_rows)
    files["pseudo"] = pseudo_header(K, L, nc) + "".join("".join(R.fmt(v) + "\t" for v in pseudo[:, f]) + "\n" for f in range(pseudo.shape[1]))
    return files


def run_traced(y, e, M, P0, P1, C, burnin, iters, tune=True, batches=None, every_burnin=None, every_sample=None, **kw):
    """The run the CLI makes (every = burnin / 1024 and iters / 1024 unless given).  batches: that many tuning batches instead of the
    CLI's stop rule."""
    b = TracedBMS(y, e, M, P0, P1, C, every_burnin=every_burnin or burnin // R.OUTLEN, every_sample=every_sample or iters // R.OUTLEN, **kw)
    b.burnin(burnin)
    pseudo = b.pseudo()
    if batches is not None:
        for _ in range(batches):
            b.tune_batch()
    elif tune:
        untuned, nb = b.tune_batch(), 1
        while untuned > 0 and nb != R.MAXBATCHES:
            untuned, nb = b.tune_batch(), nb + 1
    b.sample(iters)
    return b, pseudo


def files_of(b, pseudo):
    return trace_files(b.names(), b.stacked(0), b.stacked(1), b.tune_rows, pseudo, b.K, b.L, b.nc)
