"""numpy restatement of `mmdiff -chains C`: chain c is tests/mmdiff_ref.py's BMS with the chain put into the
stream key, the pooling is restated with that module's dlog / dexp operation for operation as mmseq_amd/csrc/diff_kernels.h
(k_dfc_pool) performs it, and the tables are formatted as the CLI prints them.  Also the device-memory formula of the handle."""
import contextlib
import math

import numpy as np

import mmdiff_ref as R
from mmdiff_poly_ref import nslot

NB = 16          # batches of the sampling run


@contextlib.contextmanager
def chain_streams(c):
    """Inside, mmdiff_ref keys its TAG_DIFF streams with chain c instead of 0; the -permute shuffle (TAG_DIFF_PERM) stays on chain 0."""
    orig = R.stream_key
    R.stream_key = lambda seed, chain, tag: orig(seed, c if tag == R.TAG_DIFF else chain, tag)
    try:
        yield
    finally:
        R.stream_key = orig


def run_chain(c, y, e, M, P0, P1, C, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, burnin=8192, iters=16384, tune=True,
              max_batches=R.MAXBATCHES):
    """Chain c driven as the handle drives it: (BMS, results, batch sums of gamma [16][F], tuning batches)."""
    with chain_streams(c):
        b = R.BMS(y, e, M, P0, P1, C, d, s, pdash, fixalpha, seed)
        b.burnin(burnin)
        if tune:
            untuned, nb = b.tune_batch(), 1
            while untuned > 0 and nb != max_batches:
                untuned, nb = b.tune_batch(), nb + 1
        gb = []
        for _ in range(NB):
            before = b.gsum.copy()
            b.sample(iters // NB)
            gb.append(b.gsum - before)
    return b, b.results(), np.array(gb), b.batches


def _philox_lanes(c0, c1, c2, c3, k0, k1):
    """mmdiff_ref.philox with a key per lane (uint64 arrays holding 32-bit words)."""
    M32 = R.M32
    x, y, z, w = (np.asarray(v, np.uint64) & M32 for v in (c0, c1, c2, c3))
    x, y, z, w = np.broadcast_arrays(x, y, z, w)
    k0, k1 = np.asarray(k0, np.uint64), np.asarray(k1, np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * x
        p1 = np.uint64(0xCD9E8D57) * z
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        x, y, z, w = hi1 ^ y ^ k0, lo1, hi0 ^ w ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return [v.astype(np.uint32) for v in (x, y, z, w)]


@contextlib.contextmanager
def chains_as_lanes(C, F):
    """Inside, a BMS over C F lanes is C chains of F features side by side: lane c F + f draws from Stream(seed, c, tag, f, it).  The
    restatement's cost is per iteration, not per lane, so this runs C chains of equal length in the time of one."""
    class LaneStreams(R.Streams):
        def __init__(self, seed, tag, ids, it):
            ids = np.asarray(ids, np.uint64)
            super().__init__(seed, tag, ids % np.uint64(F), it)
            keys = [R.stream_key(seed, c, tag) for c in range(C)]
            self.k0 = np.array([keys[int(c)][0] for c in ids // np.uint64(F)], np.uint64)
            self.k1 = np.array([keys[int(c)][1] for c in ids // np.uint64(F)], np.uint64)

        def pair(self, idx):
            r = _philox_lanes(self.ids[idx] & R.M32, self.ids[idx] >> np.uint64(32), np.uint64(self.it), self.c3[idx], self.k0[idx], self.k1[idx])
            self.c3[idx] += np.uint64(1)
            return R.u52(r[0], r[1]), R.u52(r[2], r[3])

    orig = R.Streams
    R.Streams = LaneStreams
    try:
        yield
    finally:
        R.Streams = orig


class _Chain:
    """Chain c's view of a BMS that holds C chains as lanes: what table() and pooled_means() read."""

    def __init__(self, b, c, F):
        sl = slice(c * F, (c + 1) * F)
        self.Mnil, self.Pnil, self.K, self.L = b.Mnil, b.Pnil, b.K, b.L
        self.st = [{k: v[sl] for k, v in b.st[m].items()} for m in range(2)]
        self.gsum, self.logitp, self.batches = b.gsum[sl], b.logitp[sl], b.batches


def run_chains_untuned(C, y, e, M, P0, P1, Cl, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, burnin=8192, iters=16384):
    """run_chain for c = 0 .. C - 1 without tuning, the chains side by side: the same tuples."""
    F = y.shape[0]
    with chains_as_lanes(C, F):
        b = R.BMS(np.tile(y, (C, 1)), np.tile(e, (C, 1)), M, P0, P1, Cl, d, s, pdash, fixalpha, seed)
        b.burnin(burnin)
        gb = []
        for _ in range(NB):
            before = b.gsum.copy()
            b.sample(iters // NB)
            gb.append(b.gsum - before)
    gb, r = np.array(gb), b.results()
    out = []
    for c in range(C):
        sl = slice(c * F, (c + 1) * F)
        out.append((_Chain(b, c, F), {k: v[..., sl] for k, v in r.items()}, gb[:, sl], 0))
    return out


def sigmoid(x):
    with np.errstate(all="ignore"):
        return np.where(x > 0, 1.0 / (1.0 + R.dexp(-x)), R.dexp(x) / (1.0 + R.dexp(x)))


def pool(G, o, gb, T):
    """G, o: (C, F) the chains' sums of gamma and logit p'; gb: (C, 16, F) their batch sums; T the sampling length.
    log_bf, log_bf_sd, log_bf_mcse, chains_mixed, each (F,)."""
    G, o, gb = np.asarray(G, np.float64), np.asarray(o, np.float64), np.asarray(gb, np.float64)
    C, F = G.shape
    Td, bl = float(T), float(T // NB)
    sumG = np.zeros(F)
    for c in range(C):
        sumG = sumG + G[c]
    mixed = (G > 0.0) & (G < Td)
    n = mixed.sum(0)
    finite = np.isfinite(o).all(0)
    with np.errstate(all="ignore"):
        target = sumG / Td
        lo, hi = np.full(F, -1024.0), np.full(F, 1024.0)
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            sm = np.zeros(F)
            for c in range(C):
                sm = sm + sigmoid(mid + o[c])
            below = (sm - target) < 0.0
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        b = 0.5 * (lo + hi)
        b = np.where(sumG == 0.0, -np.inf, np.where(sumG == float(C) * Td, np.inf, b))
        # the between-chain sd of logit(g_c) - o_c over the mixed chains, two passes
        ell = [(R.dlog(G[c] / Td) - R.dlog(1.0 - G[c] / Td)) - o[c] for c in range(C)]
        sm = np.zeros(F)
        for c in range(C):
            sm = np.where(mixed[c], sm + ell[c], sm)
        mean = sm / n.astype(np.float64)
        ss = np.zeros(F)
        for c in range(C):
            ss = np.where(mixed[c], ss + (ell[c] - mean) * (ell[c] - mean), ss)
        sd = np.where(n >= 2, np.sqrt(ss / (n - 1).astype(np.float64)), np.nan)
        # the sandwich standard error from the batch means
        sv, sw = np.zeros(F), np.zeros(F)
        for c in range(C):
            g = G[c] / Td
            acc = np.zeros(F)
            for k in range(NB):
                dv = gb[c, k] / bl - g
                acc = acc + dv * dv
            sv = sv + acc / float(NB - 1) / float(NB)
            sg = sigmoid(b + o[c])
            sw = sw + sg * (1.0 - sg)
        mcse = np.where(np.isinf(b), np.nan, np.sqrt(sv) / sw)
    nan = np.full(F, np.nan)
    return dict(log_bf=np.where(finite, b, nan), log_bf_sd=np.where(finite, sd, nan), log_bf_mcse=np.where(finite, mcse, nan),
                chains_mixed=n.astype(np.int64))


def pooled_means(chains):
    """The chains' summed sums over their summed counts, laid out as BMS.results lays the means out."""
    def ratio(m, S, N):
        s_ = np.zeros_like(chains[0].st[m][S])
        n_ = np.zeros_like(s_)
        for b in chains:
            s_ = s_ + b.st[m][S]
            n_ = n_ + b.st[m][N]
        with np.errstate(all="ignore"):
            return s_ / n_
    return dict(alpha=np.stack([ratio(m, "aS", "aN") for m in range(2)]),
                beta=np.stack([ratio(m, "bS", "bN").T for m in range(2)]),
                eta=np.concatenate([ratio(m, "eS", "eN").T for m in range(2)]))


def bayes_factor(log_bf):
    b = float(log_bf)
    if math.isnan(b):
        return b
    if math.isinf(b):
        return 0.0 if b < 0 else b
    return float(R.dexp(np.array([b]))[0])


def table(feats, files, b, r, y, e, p, fixalpha, pooled=None):
    """An mmdiff table as the CLI prints it: of one chain (r its results), or with `pooled` (the dict of pool()) the pooled table."""
    out = ["#prior_probability=%s\n" % R.fmt(p)]
    hdr = "feature_id\tbayes_factor\tposterior_probability\t"
    for m in range(2):
        if not fixalpha:
            hdr += "alpha%d\t" % m
        if not b.Mnil:
            hdr += "".join("beta%d_%d\t" % (m, l) for l in range(b.K))
        if not b.Pnil[m]:
            hdr += "".join("eta%d_%d\t" % (m, l) for l in range(b.L[m]))
    names = [f[f.rfind("/") + 1:f.rfind(".")] if f.endswith(".mmseq") else f for f in files]
    hdr += "".join("mu_%s\t" % n for n in names) + "\t".join("sd_%s" % n for n in names)
    out.append(hdr + ("\tlog_bf\tlog_bf_sd\tlog_bf_mcse\tchains_mixed\n" if pooled else "\n"))
    logp, log1mp = math.log(p) if p > 0 else -math.inf, math.log1p(-p) if p < 1 else -math.inf
    for f in range(len(feats)):
        if pooled:
            BF = bayes_factor(pooled["log_bf"][f])
        else:
            g, lg = float(r["gamma_mean"][f]), float(r["logitp"][f])
            pp_ = 1.0 / (1.0 + math.exp(-lg)) if lg > 0 else math.exp(lg) / (1.0 + math.exp(lg))
            with np.errstate(all="ignore"):
                BF = float(np.float64(g) / np.float64(1.0 - g) * np.float64(1.0 - pp_) / np.float64(pp_))
        lb = math.log(BF) if BF > 0 else (-math.inf if BF == 0 else math.nan)
        plo = lb + logp - log1mp
        try:
            pp = 1.0 / (1.0 + math.exp(-plo))
        except OverflowError:
            pp = 0.0
        if BF >= 1.7976931348623157e308:
            pp = 1.0
        row = "%s\t%s\t%s\t" % (feats[f], R.fmt(BF), R.fmt(pp))
        for m in range(2):
            if not fixalpha:
                row += R.fmt(r["alpha"][m, f]) + "\t"
            if not b.Mnil:
                row += "".join(R.fmt(r["beta"][m, l, f]) + "\t" for l in range(b.K))
            if not b.Pnil[m]:
                off = b.L[0] if m else 0
                row += "".join(R.fmt(r["eta"][off + l, f]) + "\t" for l in range(b.L[m]))
        row += "".join(R.fmt(v) + "\t" for v in y[f]) + "\t".join(R.fmt(v) for v in e[f])
        if pooled:
            row += "\t" + "\t".join(R.fmt(pooled[k][f]) for k in ("log_bf", "log_bf_sd", "log_bf_mcse")) + "\t%d" % pooled["chains_mixed"][f]
        out.append(row + "\n")
    return "".join(out)


def mmdiff_chains(files, C, groups=None, design=None, p=0.1, d=1.4, s=2.0, fixalpha=False, normalise_=True, pdash=0.5, tune=True,
                  burnin=8192, iters=16384, seed=1234, permute=False, max_batches=R.MAXBATCHES):
    """`mmdiff -chains C -chainout BASE` on these tables (C >= 2; no -range, -useprops, -uhfrac): the pooled stdout, the C chain
    tables, the tuning batches of each chain and the pooled columns."""
    tabs = [R.read_table(f) for f in files]
    feats = tabs[0][0]
    y = np.stack([t[1] for t in tabs], 1)
    e = np.stack([t[2] for t in tabs], 1)
    uh = np.stack([t[3] for t in tabs], 1)
    S = len(files)
    if normalise_:
        y, _ = R.normalise(y, uh, max(0.2, float(S - S * S // 160) / float(S)))
    if permute:
        for f in range(y.shape[0]):
            idx = R.permutation(seed & 0xFFFFFFFF, f, S)
            y[f] = y[f, idx]
            e[f] = e[f, idx]
    M, P0, P1, Cl = R.de_design(groups) if design is None else design
    if tune:
        runs = [run_chain(c, y, e, M, P0, P1, Cl, d, s, pdash, fixalpha, seed & 0xFFFFFFFF, burnin, iters, tune, max_batches) for c in range(C)]
    else:       # chains of equal length: side by side
        runs = run_chains_untuned(C, y, e, M, P0, P1, Cl, d, s, pdash, fixalpha, seed & 0xFFFFFFFF, burnin, iters)
    chains = [table(feats, files, b, r, y, e, p, fixalpha) for b, r, _, _ in runs]
    cols = pool([b.gsum for b, _, _, _ in runs], [b.logitp for b, _, _, _ in runs], [gb for _, _, gb, _ in runs], iters)
    text = table(feats, files, runs[0][0], pooled_means([b for b, _, _, _ in runs]), y, e, p, fixalpha, cols)
    return text, chains, [nb for _, _, _, nb in runs], cols


def chains_device_bytes(F, N, K, L0, L1, nc0, nc1, Mnil, C):
    """8 (2 F N + N K + N L0 + N L1 + C F (nslot + 16) + F (8 + 4 K + 2 L0 + 2 L1)) + 4 (2 N + 2 C F) + 488 C."""
    doubles = 2 * F * N + N * K + N * L0 + N * L1 + C * F * (nslot(K, L0, L1, nc0, nc1, Mnil) + NB) + F * (8 + 4 * K + 2 * L0 + 2 * L1)
    return 8 * doubles + 4 * (2 * N + 2 * C * F) + 488 * C
