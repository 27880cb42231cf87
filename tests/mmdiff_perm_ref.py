"""numpy restatement of `mmdiff -permutations B` on top of tests/mmdiff_ref.py: replica b's data is the
-permute shuffle of the seed seed ^ (b << 32), its chain is that module's BMS with b in the stream key, the tables are formatted as the
CLI prints them (tests/mmdiff_chains_ref.py's table), and the two appended columns come from tests/qvalue_ref.py applied to the log
Bayes factors.  Also the device-memory formula of the handle."""
import numpy as np

import mmdiff_chains_ref as CR
import mmdiff_ref as R
import qvalue_ref as Q
from mmdiff_poly_ref import nslot


def replica_data(y, e, seed, b):
    """(y_b, e_b): replica 0 the data itself, replica b >= 1 every feature's samples shuffled as -permute shuffles them with the seed
    seed ^ (b << 32)."""
    y, e = np.array(y, np.float64), np.array(e, np.float64)
    if b == 0:
        return y, e
    yb, eb = y.copy(), e.copy()
    for f in range(y.shape[0]):
        idx = R.permutation(seed ^ (b << 32), f, y.shape[1])
        yb[f], eb[f] = y[f, idx], e[f, idx]
    return yb, eb


def statistic(gamma_mean, logitp):
    """T = log(g) - log(1 - g) - logit p' with the library's log; NaN where logit p' is not finite."""
    g, o = np.asarray(gamma_mean, np.float64), np.asarray(logitp, np.float64)
    with np.errstate(all="ignore"):
        t = R.dlog(g) - R.dlog(1.0 - g) - o
    return np.where(np.isfinite(o), t, np.nan)


def run_replicas_untuned(B, y, e, M, P0, P1, Cl, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, burnin=8192, iters=16384):
    """The B + 1 replicas without tuning, side by side as lanes of one BMS: per replica (view of its chain, results, y_b, e_b)."""
    F = y.shape[0]
    data = [replica_data(y, e, seed, b) for b in range(B + 1)]
    with CR.chains_as_lanes(B + 1, F):
        bms = R.BMS(np.concatenate([yb for yb, _ in data]), np.concatenate([eb for _, eb in data]), M, P0, P1, Cl, d, s, pdash, fixalpha, seed)
        bms.burnin(burnin)
        bms.sample(iters)
    r = bms.results()
    out = []
    for b in range(B + 1):
        sl = slice(b * F, (b + 1) * F)
        out.append((CR._Chain(bms, b, F), {k: v[..., sl] for k, v in r.items()}) + data[b])
    return out


def mmdiff_perm(files, B, groups=None, design=None, p=0.1, d=1.4, s=2.0, fixalpha=False, normalise_=True, pdash=0.5, burnin=8192,
                iters=16384, seed=1234):
    """`mmdiff -permutations B -permout BASE -notune` on these tables (no -range, -useprops, -uhfrac): the stdout, the B tables of
    the shuffled replicas, and (stat (B + 1, F), null_ge, q)."""
    tabs = [R.read_table(f) for f in files]
    feats = tabs[0][0]
    y = np.stack([t[1] for t in tabs], 1)
    e = np.stack([t[2] for t in tabs], 1)
    uh = np.stack([t[3] for t in tabs], 1)
    S = len(files)
    if normalise_:
        y, _ = R.normalise(y, uh, max(0.2, float(S - S * S // 160) / float(S)))
    M, P0, P1, Cl = R.de_design(groups) if design is None else design
    runs = run_replicas_untuned(B, y, e, M, P0, P1, Cl, d, s, pdash, fixalpha, seed & 0xFFFFFFFF, burnin, iters)
    tables = [CR.table(feats, files, c, r, yb, eb, p, fixalpha) for c, r, yb, eb in runs]
    stat = np.stack([statistic(r["gamma_mean"], r["logitp"]) for _, r, _, _ in runs])
    ge, q = Q.qvalues(stat[0], stat[1:].ravel())
    lines = tables[0].split("\n")
    lines[1] += "\tperm_ge\tq_value"
    for f in range(len(feats)):
        lines[2 + f] += "\t%d\t%s" % (ge[f], R.fmt(q[f]))
    return "\n".join(lines), tables[1:], (stat, ge, q)


def perm_device_bytes(F, N, K, L0, L1, nc0, nc1, Mnil, B):
    """8 (2 R F N + N K + N L0 + N L1 + R F (nslot + 1) + 2 F) + 4 (2 N + 2 R F) + 488 R with R = B + 1."""
    Rr = B + 1
    doubles = 2 * Rr * F * N + N * K + N * L0 + N * L1 + Rr * F * (nslot(K, L0, L1, nc0, nc1, Mnil) + 1) + 2 * F
    return 8 * doubles + 4 * (2 * N + 2 * Rr * F) + 488 * Rr
