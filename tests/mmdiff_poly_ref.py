"""numpy restatement of `mmdiff -polyclass` (polyclass() of the reference's src/R/mmseq.R as DESIGN.md section 10 defines it): the
posterior probabilities of models 0..J from J mmdiff tables, the output text byte for byte; and the device-memory formula of the
polytomous handle."""
import math

import numpy as np

from mmdiff_ref import fmt


def read_mmdiff(text):
    """(header, rows) of an mmdiff table: '#' lines and empty lines skipped, cells split on tabs."""
    lines = [ln for ln in text.split("\n") if ln and not ln.startswith("#")]
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def posteriors(bf, prior):
    """bf, prior: (n,) with bf[0] = 1; the posterior model probabilities and whether a warning goes with them."""
    bf = np.asarray(bf, np.float64)
    prior = np.asarray(prior, np.float64)
    inf = np.isinf(bf)
    if np.isnan(bf).any():
        return np.full(bf.size, np.nan), True
    if inf.sum() == 1:
        return np.where(inf, 1.0, 0.0), False
    if inf.sum() > 1:
        return np.where(inf, np.nan, 0.0), True
    w = bf * prior
    sm = np.float64(0.0)
    for v in w:                      # index order
        sm = sm + v
    if sm == 0.0:
        return np.full(bf.size, np.nan), True
    return w / sm, False


def polyclass(texts, prior=None):
    """The stdout of `mmdiff -polyclass [-prior ...]` on tables with these contents, and the number of warned rows."""
    J = len(texts)
    n = J + 1
    if prior is None:
        prior = [1.0 / float(n)] * n
    tabs = [read_mmdiff(t) for t in texts]
    hdr, rows = tabs[0]
    fi = hdr.index("feature_id")
    kept = [i for i, c in enumerate(hdr) if c.startswith("mu_") or c.startswith("sd_")]
    bfs = []
    for h, r in tabs:
        bi = h.index("bayes_factor")
        bfs.append([float(row[bi]) for row in r])
    out = ["#prior_probabilities=" + ",".join(fmt(v) for v in prior) + "\n"]
    out.append("\t".join(["feature_id"] + [hdr[i] for i in kept] + ["postprob_model%d" % j for j in range(n)]) + "\n")
    warned = 0
    for k, row in enumerate(rows):
        post, w = posteriors([1.0] + [bfs[j][k] for j in range(J)], prior)
        warned += int(w)
        out.append("\t".join([row[fi]] + [row[i] for i in kept] + [fmt(v) for v in post]) + "\n")
    return "".join(out), warned


def recompute_pp(bf, prior):
    """The reference README's recompute_pp: 1 / (1 + exp(-(log(bf) + log(prior) - log(1 - prior))))."""
    return 1.0 / (1.0 + math.exp(-(math.log(bf) + math.log(prior) - math.log(1.0 - prior))))


def nslot(K, L0, L1, nc0, nc1, Mnil):
    """State and workspace slots per feature of one comparison."""
    per_model = lambda L, nc: 11 + 6 * K + 11 * L + 5 * nc
    return per_model(L0, nc0) + per_model(L1, nc1) + 3 + (0 if Mnil else 5 * K * K + 2 * K) + 2 * max(nc0, nc1)


def poly_device_bytes(F, N, K, L0, nc0, Mnil, alts):
    """alts: (L1, nc1) per comparison.  8 (2 F N + N K + N L0 + sum_j (F nslot_j + N L1_j)) + 4 sum_j (2 N + 2 F) + 488 J."""
    J = len(alts)
    doubles = 2 * F * N + N * K + N * L0 + sum(F * nslot(K, L0, L1, nc0, nc1, Mnil) + N * L1 for L1, nc1 in alts)
    return 8 * doubles + 4 * J * (2 * N + 2 * F) + 488 * J


def single_device_bytes(F, N, K, L0, L1, nc0, nc1, Mnil):
    """One mmg_diff handle: 8 (2 F N + F nslot + N K + N L0 + N L1) + 4 (2 N + 2 F + 1)."""
    return 8 * (2 * F * N + F * nslot(K, L0, L1, nc0, nc1, Mnil) + N * K + N * L0 + N * L1) + 4 * (2 * N + 2 * F + 1)
