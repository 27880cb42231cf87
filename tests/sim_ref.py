"""The specification of mmg_sim_* (include/mmgibbs.h) and of the mmsim CLI in numpy.  No device.

Input: S samples; per sample s the draws v_s[t][f] (T joint draws of F features, the rows of a trace file) and an offset off_s on the
natural-log scale; per run a centre c[F] (None: zeros), a mask[F] (None: ones), the flag `logged`, and zero-based ranks.

Values:      x = log v (the library's dlog through the oracle's log_v, as tests/fold_ref.py takes it, so bits can be compared), or
             x = v with `logged`; z_s[t][f] = ((x + off_s) - c[f]) + 0.0, each operation rounded once.
Used:        mask[f] != 0 and every one of the feature's S T values valid: finite and > 0, or just finite with `logged`; checked before
             the logarithm.  n = their number.  z is 0.0 at every unused feature.  n < 2: status bit 0, every summary NaN, counts 0.
Stage 1:     G[t][r][s] = sum over the used f of z_r[t][f] z_s[t][f], m[t][r] = sum of z_r[t][f].  The device's order of summation is
             its own; `gram` here sums in np.longdouble, so a comparison carries the bound of a dot product (tests/test_gpu_sim.py).
Stage 2:     from G, m as float64, exactly these operations, each rounded once (`summary_from_gram`):
             D[t] = sqrt(max(0, (G_rr + G_ss) - 2 G_rs) / n)
             R[t] = (G_rs - m_r m_s / n) / sqrt((G_rr - m_r m_r / n) (G_ss - m_s m_s / n)); a variance term <= 0 or an R that is not
                    finite in any draw: pair status bit 1, every R output of the pair NaN
             nn[a][b] = #{t: b = argmin over b' != a of (G_aa + G_b'b') - 2 G_ab'}, ties to the smallest b'
Per pair:    r < s, r-major, over the T draws: mean = lsum(x) / T, ss = lsum((x - mean) * (x - mean)) with pairs_ref.lsum (the order
             of a wave with one lane per draw), of D and of R; q[k] = np.sort(x)[ranks[k]], NaN for a rank >= T.
Derived:     sd = sqrt(ss / (T - 1)), p_nearest = nn / T.

The CLI's rules: `default_uhfrac` and `offsets` (mmdiff's normalisation, tests/mmdiff_ref.normalise, over the features whose log_mu
is finite in every sample; off_s = minus the sample's median), `feature_mask`, `centre_of`, `percentile_rank`, `table` and `matrix`,
the texts mmsim writes.
"""
import numpy as np

from mmdiff_ref import dlog
from pairs_ref import lsum

FEW_FEATURES, PAIR_NO_R = 1, 2
SUMMARY_KEYS = ("mean_D", "ss_D", "q_D", "mean_R", "ss_R", "q_R", "nn", "pair_status", "status")


def pairs_of(S):
    return [(r, s) for r in range(S) for s in range(r + 1, S)]


def values(traces, offs, centre=None, mask=None, logged=False, log=dlog):
    """traces: (S, T, F) -> z (S, T, F) with the unused features zeroed, used (F,) uint8, n"""
    v = np.asarray(traces, np.float64)
    S, T, F = v.shape
    c = np.zeros(F) if centre is None else np.asarray(centre, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) if logged else (np.isfinite(v) & (v > 0))
    used = ok.all(axis=(0, 1))
    if mask is not None:
        used &= np.asarray(mask) != 0
    z = np.zeros_like(v)
    cols = np.flatnonzero(used)
    for s in range(S):
        w = np.ascontiguousarray(v[s][:, cols])
        x = w if logged else np.asarray(log(w.ravel()), np.float64).reshape(w.shape)
        z[s][:, cols] = ((x + np.float64(offs[s])) - c[cols]) + 0.0
    return z, used.astype(np.uint8), int(used.sum())


def gram(z, used):
    """G (T, S, S), m (T, S) over the used features, summed in np.longdouble"""
    zl = np.asarray(z, np.float64)[:, :, np.asarray(used) != 0].astype(np.longdouble)
    G = np.einsum("rtf,stf->trs", zl, zl)
    m = zl.sum(axis=2).T
    return G, m


def summary_from_gram(G, m, n, ranks):
    """every output of mmg_sim_get from the stage-1 numbers as float64"""
    G, m = np.asarray(G, np.float64), np.asarray(m, np.float64)
    T, S = m.shape
    P = S * (S - 1) // 2
    ranks = [int(k) for k in ranks]
    out = dict(mean_D=np.full(P, np.nan), ss_D=np.full(P, np.nan), q_D=np.full((P, len(ranks)), np.nan), mean_R=np.full(P, np.nan),
               ss_R=np.full(P, np.nan), q_R=np.full((P, len(ranks)), np.nan), nn=np.zeros((S, S), np.uint32),
               pair_status=np.zeros(P, np.uint8), status=0)
    if n < 2:
        out["status"] = FEW_FEATURES
        return out
    nf = np.float64(n)

    def moments(x):
        mean = lsum(x) / np.float64(T)
        d = x - mean
        return mean, lsum(d * d)

    with np.errstate(all="ignore"):
        for p, (r, s) in enumerate(pairs_of(S)):
            grr, gss, grs, mr, ms = G[:, r, r], G[:, s, s], G[:, r, s], m[:, r], m[:, s]
            num = (grr + gss) - 2.0 * grs
            D = np.sqrt(np.where(num < 0.0, 0.0, num) / nf) + 0.0
            va, vb = grr - mr * mr / nf, gss - ms * ms / nf
            R = (grs - mr * ms / nf) / np.sqrt(va * vb) + 0.0
            out["mean_D"][p], out["ss_D"][p] = moments(D)
            Ds = np.sort(D)
            for k, rk in enumerate(ranks):
                if rk < T:
                    out["q_D"][p, k] = Ds[rk]
            if (~(va > 0.0) | ~(vb > 0.0) | ~np.isfinite(R)).any():
                out["pair_status"][p] = PAIR_NO_R
                continue
            out["mean_R"][p], out["ss_R"][p] = moments(R)
            Rs = np.sort(R)
            for k, rk in enumerate(ranks):
                if rk < T:
                    out["q_R"][p, k] = Rs[rk]
        diag = np.einsum("tii->ti", G)
        for a in range(S):
            d = (diag[:, a][:, None] + diag) - 2.0 * G[:, a, :]
            d[:, a] = np.inf
            best = np.argmin(d, axis=1)                        # the first of equals
            out["nn"][a] = np.bincount(best, minlength=S).astype(np.uint32)
    return out


def derived(dev, T):
    with np.errstate(all="ignore"):
        return dict(sd_D=np.sqrt(dev["ss_D"] / np.float64(T - 1)), sd_R=np.sqrt(dev["ss_R"] / np.float64(T - 1)),
                    p_nearest=dev["nn"].astype(np.float64) / np.float64(T))


def sim_ref(traces, offs, ranks, centre=None, mask=None, logged=False, log=dlog):
    """z, used, n, G and m (longdouble), and the summary of G and m rounded to float64, with the derived columns"""
    z, used, n = values(traces, offs, centre, mask, logged, log)
    G, m = gram(z, used)
    out = summary_from_gram(G.astype(np.float64), m.astype(np.float64), n, ranks)
    out.update(derived(out, z.shape[1]))
    out.update(z=z, used=used, n=n, G=G, m=m)
    return out


# ---- the CLI's rules
def default_uhfrac(S):
    """mmdiff's default: max(0.2, (S - S * S / 160) / S), the inner division an integer one"""
    return max(0.2, float(S - S * S // 160) / float(S))


def offsets(log_mu, uh, uhfrac=None):
    """log_mu, uh: (F, S).  mmdiff's normalisation over the features with a unique hit in at least uhfrac of the samples (and a finite
    log_mu in every sample): the median (the upper one of an even count) of log_mu[:, s] minus the features' means; off_s is minus
    it.  Fewer than 100 such features: no normalisation.  Returns (offsets, the number of features, or None if skipped)."""
    y, uh = np.asarray(log_mu, np.float64), np.asarray(uh)
    F, S = y.shape
    if uhfrac is None:
        uhfrac = default_uhfrac(S)
    use = [i for i in range(F) if float((uh[i] > 0).sum()) / float(S) >= uhfrac and np.isfinite(y[i]).all()]
    if len(use) < 100:
        return [0.0] * S, None
    means = []
    for i in use:
        sm = 0.0
        for j in range(S):
            sm += y[i, j]
        means.append(sm / float(S))
    offs = []
    for j in range(S):
        dif = sorted(y[i, j] - means[k] for k, i in enumerate(use))
        offs.append(-float(dif[len(dif) // 2]))
    return offs, len(use)


def feature_mask(log_mu, uh, traced, uhmin=1):
    """unique_hits >= uhmin and a finite log_mu in every table, and a column in every trace file (traced: (F, S))"""
    return (np.asarray(uh) >= uhmin).all(axis=1) & np.isfinite(np.asarray(log_mu, np.float64)).all(axis=1) & np.asarray(traced, bool).all(axis=1)


def centre_of(log_mu, offs, mask):
    """c[f] = the mean over the samples of log_mu + off_s, added in the samples' order; 0.0 outside the mask"""
    y = np.asarray(log_mu, np.float64)
    F, S = y.shape
    c = np.zeros(F)
    for f in np.flatnonzero(mask):
        sm = 0.0
        for s in range(S):
            sm += y[f, s] + offs[s]
        c[f] = sm / float(S)
    return c


def percentile_rank(p, T):
    """C's round(p / 100 * (T - 1)): halves away from zero"""
    v = float(p) / 100.0 * float(T - 1)
    fl = np.floor(v)
    return int(fl) + (1 if v - fl >= 0.5 else 0)


def fmt(v):
    """printf's %g; NaN as "nan" """
    return "nan" if np.isnan(v) else "%g" % v


def table(bases, level, T, n_used, F, offs, centre, percentiles, out):
    """The text mmsim writes.  out: the summary (with the derived columns) for the ranks of the percentiles."""
    S = len(bases)
    pc = ",".join(fmt(p) for p in percentiles)
    L = ["# mmsim: posterior distance (root-mean-square log ratio) and correlation between samples, from their joint posterior draws",
         "# level: %s" % level, "# T: %d" % T, "# features: %d/%d" % (n_used, F), "# centre: %s" % centre]
    L += ["# sample %d: %s offset %s" % (s, bases[s], fmt(offs[s])) for s in range(S)]
    L.append("sample_a\tsample_b\tdist\tdist_sd\tdist_percentiles" + pc + "\tcor\tcor_sd\tcor_percentiles" + pc + "\tnearest_a\tnearest_b\tstatus")
    for p, (a, b) in enumerate(pairs_of(S)):
        L.append("\t".join([bases[a], bases[b], fmt(out["mean_D"][p]), fmt(out["sd_D"][p]), ",".join(fmt(v) for v in out["q_D"][p]),
                            fmt(out["mean_R"][p]), fmt(out["sd_R"][p]), ",".join(fmt(v) for v in out["q_R"][p]),
                            fmt(out["p_nearest"][a, b] if out["status"] == 0 else np.nan), fmt(out["p_nearest"][b, a] if out["status"] == 0 else np.nan),
                            str(int(out["pair_status"][p]) | int(out["status"]))]))
    return ("\n".join(L) + "\n").encode()


def matrix(bases, out):
    """The text of -matrix FILE: the mean distances, zeros on the diagonal"""
    S = len(bases)
    M = np.zeros((S, S))
    for p, (a, b) in enumerate(pairs_of(S)):
        M[a, b] = M[b, a] = out["mean_D"][p]
    L = ["\t" + "\t".join(bases)] + ["\t".join([bases[a]] + ["0" if a == b else fmt(M[a, b]) for b in range(S)]) for a in range(S)]
    return ("\n".join(L) + "\n").encode()
