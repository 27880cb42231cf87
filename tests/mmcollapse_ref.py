"""numpy restatement of mmcollapse (src/mmcollapse.cpp), the yardstick of tests/test_mmcollapse_cli.py and
tests/test_gpu_mmcollapse.py.  Written from the reference's algorithm: candidates (:117-396, :620-698), mean correlations
(:483-561), threshold (:713-747), greedy loop with collapse() (:398-441, :758-819), output tables (:827-1107).  Sokal's estimator
is the oracle's restatement (oracle/binding.py: sokal)."""
import gzip
import math

import numpy as np

TRACELEN = 1024
IACTTHRES = 1.1


# ------------------------------------------------------------------------------------------ correlations and the loop
def centre(traces):
    """S arrays (N, C) -> centred float64 copies."""
    return [np.asarray(t, np.float64) - np.asarray(t, np.float64).mean(axis=0) for t in traces]


def _corr(Xc_s, a_cols, b_cols=None, fixed_order=False):
    """Covariances of the columns a_cols with b_cols (all).  BLAS sums in an order that depends on an entry's position, so a column
    scaled by 2^k need not give bit-identical correlations; fixed_order sums over the trace rows in ascending order for every entry,
    which keeps such exact ties (the device's order is fixed too)."""
    N = Xc_s.shape[0]
    A = Xc_s[:, a_cols]
    B = Xc_s if b_cols is None else Xc_s[:, b_cols]
    with np.errstate(all="ignore"):
        if fixed_order:
            cov = np.zeros((A.shape[1], B.shape[1]))
            for k in range(N):
                cov += A[k][:, None] * B[k][None, :]
            cov /= N - 1
        else:
            cov = A.T @ B / (N - 1)
        cov[~np.isfinite(cov)] = 0.0
    return cov


def mean_corr(Xc, observed, fixed_order=False):
    """V (C x C): masked mean over samples of cov / sqrt(var_i) / sqrt(var_j); non-finite covariances -> 0."""
    observed = np.asarray(observed, bool)
    C = observed.shape[0]
    num = np.zeros((C, C))
    cnt = np.zeros((C, C))
    for s, X in enumerate(Xc):
        cov = _corr(X, slice(None), fixed_order=fixed_order)
        d = np.sqrt(np.diag(cov).copy())
        with np.errstate(all="ignore"):
            r = cov / d[:, None] / d[None, :]
        u = np.outer(observed[:, s], observed[:, s])
        r[~u] = 0.0
        num += r
        cnt += u
    with np.errstate(all="ignore"):
        return num / cnt


def row_max(V):
    """Per row the off-diagonal maximum starting from -1, NaN skipped (:719-730)."""
    W = np.array(V, copy=True)
    np.fill_diagonal(W, -np.inf)
    W[np.isnan(W)] = -np.inf
    return np.maximum(W.max(axis=1), -1.0)


def threshold_index(C, thres):
    return min(int(math.floor(C * thres)), C - 1)


def threshold(rmax, thres):
    return -np.sort(rmax)[threshold_index(len(rmax), thres)]


def vmin(V):
    """Armadillo's V.min(row, col): NaN skipped, ties to the first entry in column-major order.  (value, row, col) or None."""
    flat = V.T.ravel()           # column-major
    if np.all(np.isnan(flat)):
        return None
    k = int(np.nanargmin(flat))
    C = V.shape[0]
    return flat[k], k % C, k // C


def second_gap(V, a, b):
    """Distance from the minimum to the smallest entry outside the pair (a, b) / (b, a) that is not bit-equal to V(a, b) or V(b, a),
    and the number of entries that are (exact ties, which the column-major rule decides)."""
    W = np.array(V, copy=True)
    W[a, b] = W[b, a] = np.nan
    same = (W == V[a, b]) | (W == V[b, a])
    ties = int(np.count_nonzero(same))
    W[same] = np.nan
    if np.all(np.isnan(W)):
        return np.inf, ties
    return np.nanmin(W) - V[a, b], ties


class Greedy:
    """The loop of :758-819 on centred traces: merge the pair at the minimum into the lower index (summed traces, the lower
    member's mask), the higher index NaN, rows / columns of both recomputed (:483-512 with ts = {a, b})."""

    def __init__(self, traces, observed, names=None, fixed_order=False):
        self.Xc = centre(traces)
        self.obs = np.array(observed, bool)
        self.C = self.obs.shape[0]
        self.fixed_order = fixed_order
        self.V = mean_corr(self.Xc, self.obs, fixed_order)
        self.dead = np.zeros(self.C, bool)
        self.names = list(names) if names is not None else [str(i) for i in range(self.C)]
        self.exact_ties = 0          # picks of run(tie_tol=...) where another entry equalled the minimum bit for bit

    def merge(self, a, b):
        for X in self.Xc:
            X[:, a] += X[:, b]
        self.dead[b] = True
        num = np.zeros(self.C)
        cnt = np.zeros(self.C)
        for s, X in enumerate(self.Xc):
            cov = _corr(X, [a], fixed_order=self.fixed_order)[0]
            va = cov[a]
            dj = ((X * X).sum(axis=0) if self.fixed_order else np.einsum("ij,ij->j", X, X)) / (X.shape[0] - 1)
            dj[~np.isfinite(dj)] = 0.0
            dj[a] = va
            with np.errstate(all="ignore"):
                r = cov / np.sqrt(va) / np.sqrt(dj)
            u = self.obs[a, s] & self.obs[:, s]
            r[~u] = 0.0
            num += r
            cnt += u
        with np.errstate(all="ignore"):
            row = num / cnt
        row[self.dead] = np.nan
        self.V[a, :] = row
        self.V[:, a] = row
        self.V[b, :] = np.nan
        self.V[:, b] = np.nan
        t = sorted([self.names[a], self.names[b]])
        self.names[a] = t[0] + "*" + t[1]
        self.names[b] = "NA"

    def run(self, thr, tie_tol=None, max_merges=None):
        """Returns the merge list [(a, b, value)]; with tie_tol, asserts no decision lies within tie_tol of a tie (the pick, and
        the stop against thr).  Entries bit-equal to the minimum are exact ties, not near ones: vmin's column-major rule decides
        them, and they are counted in self.exact_ties.  With max_merges, returns after that many merges; a later call continues."""
        merges = []
        while max_merges is None or len(merges) < max_merges:
            m = vmin(self.V)
            if m is None:
                break
            v, r, c = m
            if tie_tol is not None:
                assert abs(v - thr) > tie_tol, "the stop is within %g of the threshold" % tie_tol
            if not v < thr:
                break
            a, b = min(r, c), max(r, c)
            if tie_tol is not None:
                gap, ties = second_gap(self.V, a, b)
                assert gap > tie_tol, "pick %d is within %g of a tie" % (len(merges), tie_tol)
                self.exact_ties += ties > 0
            merges.append((a, b, v))
            self.merge(a, b)
        return merges

    def replay(self, thr, pairs, tol):
        """Replays another merge list: each pick must be within tol of that step's minimum; returns whether the loop would stop
        after the last pair (the minimum is not below thr)."""
        for k, (a, b) in enumerate(pairs):
            v, _, _ = vmin(self.V)
            assert self.V[a, b] - v <= tol, "step %d: V(a, b) = %r, the minimum %r" % (k, self.V[a, b], v)
            assert v < thr + tol
            self.merge(int(a), int(b))
        m = vmin(self.V)
        return m is None or not m[0] < thr, (None if m is None else m[0])


# ------------------------------------------------------------------------------------------ files
def _tok(s, d):
    return [t for t in s.split(d) if t != ""]


def read_table(path):
    """comment lines, header, rows (lists of fields)"""
    lines = open(path).read().split("\n")
    com = []
    i = 0
    while i < len(lines) and lines[i].startswith("#"):
        com.append(lines[i]); i += 1
    hdr = _tok(lines[i], "\t")
    rows = [_tok(ln, "\t") for ln in lines[i + 1:]]
    out = []
    for r in rows:
        if not r:
            break
        out.append(r)
    return com, hdr, out


def read_trace(path):
    with gzip.open(path, "rt") as f:
        head = f.readline()
        ids = _tok(head.rstrip("\n"), " ")
        vals = np.array([float(x) if x != "NA" else 0.0 for x in f.read().split()][:TRACELEN * len(ids)], np.float64)
    return ids, vals.reshape(TRACELEN, len(ids)) if ids else np.zeros((TRACELEN, 0))


def candidates(basenames):
    """The candidate rules of :117-396, :620-686; returns a dict of what the later stages use."""
    is_ident = set()
    all_features = []
    cands_all, zeros_all, toremove = None, None, set()
    per = []
    for s, base in enumerate(basenames):
        cands, sd, zeros, zero_efflen = [], [], [], {}
        _, hdr, rows = read_table(base + ".identical.mmseq")
        c = {k: hdr.index(k) for k in ("feature_id", "observed", "sd", "effective_length")}
        for r in rows:
            f = r[c["feature_id"]]
            cands.append(f)
            is_ident.update(_tok(f, "+"))
            if s == 0:
                all_features.append(f)
            if r[c["observed"]] == "0":
                sd.append(math.inf); zeros.append(f); zero_efflen[f] = float(r[c["effective_length"]])
            else:
                sd.append(float(r[c["sd"]]))
        com, hdr, rows = read_table(base + ".mmseq")
        mapped = [int(float(_tok(x, " ")[-1])) for x in com if "Mapped fragments" in x][0]
        c = {k: hdr.index(k) for k in ("feature_id", "unique_hits", "iact", "observed", "sd", "effective_length")}
        max_h1 = 0.0
        for r in rows:
            f = r[c["feature_id"]]
            ident = f in is_ident
            if not ident and s == 0:
                all_features.append(f)
            if r[c["unique_hits"]] == "0" and not ident:
                cands.append(f)
                if r[c["observed"]] == "0":
                    sd.append(math.inf); zeros.append(f); zero_efflen[f] = float(r[c["effective_length"]])
                else:
                    sd.append(float(r[c["sd"]]))
            elif r[c["unique_hits"]] == "1":
                if float(r[c["sd"]]) > max_h1 and float(r[c["iact"]]) < IACTTHRES:
                    max_h1 = float(r[c["sd"]])
                toremove.add(f)
            else:
                toremove.add(f)
        keep = []
        for f, d in zip(cands, sd):
            if d < max_h1 or f in is_ident:
                toremove.add(f)
            else:
                keep.append(f)
        per.append(dict(zeros=zeros, zero_efflen=zero_efflen, mapped=mapped))
        cands_all = set(keep) if cands_all is None else cands_all | set(keep)
        zeros_all = set(zeros) if zeros_all is None else zeros_all & set(zeros)
    cand = sorted(cands_all - zeros_all - toremove)
    idx = {f: i for i, f in enumerate(cand)}
    obs = np.ones((len(cand), len(basenames)), bool)
    for s, p in enumerate(per):
        for z in p["zeros"]:
            if z in idx:
                obs[idx[z], s] = False
    return dict(candidates=cand, observed=obs, all_features=all_features, is_ident=is_ident, per=per)


def sample_traces(base, is_ident):
    ids1, m1 = read_trace(base + ".trace_gibbs.gz")
    ids2, m2 = read_trace(base + ".identical.trace_gibbs.gz")
    keep = [i for i, f in enumerate(ids1) if f not in is_ident]
    return [ids1[i] for i in keep] + ids2, np.concatenate([m1[:, keep], m2], axis=1)


def uh(base, series):
    """unique hits (src/uh.cpp) of each series, given as sets of transcript names"""
    lines = open(base + ".M").read().split("\n")
    names = lines[0].split("\t")[1:]
    of = {}
    for g, members in enumerate(series):
        for m in members:
            of[m] = g
    col = [of.get(n, -1) for n in names]
    rows = {}
    for ln in lines[1:]:
        if ln.strip():
            i, j = map(int, ln.split())
            rows.setdefault(i, []).append(j)
    k = [int(x) for x in open(base + ".k").read().split()]
    res = np.zeros(len(series), np.int64)
    for i in range(len(k)):
        r = rows.get(i, [])
        if not r:
            res += k[i]
            continue
        gs = {col[j] for j in r}
        if len(gs) == 1 and -1 not in gs:
            res[gs.pop()] += k[i]
    return res


SIMU_SEED, ALPHA, BETA = 13837, 0.1, 0.1


def simulated(cd, s, ids):
    """The features of the first sample's list (cd["all_features"]) that sample s's traces (ids) lack, as [(index in that list,
    name, scale)]: scale = 1 / (0.1 + efflen * mapped / 1e9) with the efflen of sample s's zero rows and its "# Mapped fragments"."""
    per, have = cd["per"][s], set(ids)
    return [(f, name, 1.0 / (BETA + per["zero_efflen"][name] * float(per["mapped"]) / 1e9))
            for f, name in enumerate(cd["all_features"]) if name not in have]


def simulate_missing(ids, M, cd, s):
    """The trace matrix of sample s extended by the simulated traces of its features without one (difference
    1): Gamma(0.1) * scale keyed (13837, chain s, TAG_COLLAPSE_SIMU, the feature's index in the first sample's list, the row),
    appended after the real columns in the order of that list."""
    from oracle import binding as B
    sim = simulated(cd, s, ids)
    cols = [B.simu_gamma_trace_keyed(SIMU_SEED, s, B.TAG_COLLAPSE_SIMU, f, ALPHA, sc, M.shape[0]) for f, _, sc in sim]
    return list(ids) + [n for _, n, _ in sim], np.concatenate([M] + [c[:, None] for c in cols], axis=1)


def run(basenames, thres=0.975, tie_tol=None):
    """The whole tool; returns (merges, final candidate names, {base: (comment lines, rows)}) with rows
    [name, log_mu, sd, mcse, iact, unique_hits] sorted by name.  A feature without a trace in a sample gets the simulated trace of
    simulate_missing."""
    from oracle import binding as B
    cd = candidates(basenames)
    cand = cd["candidates"]
    traces = []
    samp = []
    for base in basenames:
        ids, M = sample_traces(base, cd["is_ident"])
        samp.append((ids, M))
        pos = {f: i for i, f in enumerate(ids)}
        X = np.zeros((TRACELEN, len(cand)))
        for j, f in enumerate(cand):
            if f in pos:
                X[:, j] = M[:, pos[f]]
        traces.append(X)
    names = list(cand)
    merges = []
    if len(cand) >= 2:
        g = Greedy(traces, cd["observed"], cand)
        thr = threshold(row_max(g.V), thres)
        merges = g.run(thr, tie_tol)
        names = g.names
    forcollapsing = sorted({n for n in names if "*" in n})
    out = {}
    for s, base in enumerate(basenames):
        ids, M = samp[s]
        ids, M = simulate_missing(ids, M, cd, s)
        tmap = {f: i for i, f in enumerate(ids)}
        shed = set()
        M = M.copy()
        for name in forcollapsing:
            idx = sorted(tmap[t] for t in name.split("*"))
            for t in idx[1:]:
                M[:, idx[0]] += M[:, t]
                shed.add(t)
            ids[idx[0]] = name
        cols = sorted((ids[c], c) for c in range(len(ids)) if c not in shed)
        series = [{x for p in _tok(n, "+") for x in _tok(p, "*")} for n, _ in cols]
        u = uh(base, series)
        rows = []
        for (n, c), hits in zip(cols, u):
            y = np.log(M[:, c])
            rc, var, tau, _ = B.sokal(y)
            mcse, iact = (TRACELEN, float("nan")) if rc else (math.sqrt(tau * var / TRACELEN), tau)
            rows.append([n, float(y.mean()), math.sqrt(var), mcse, iact, int(hits)])
        com, _, _ = read_table(base + ".mmseq")
        out[base] = (com, rows)
    return merges, names, out
