"""numpy restatement of mmdiff (src/mmdiff.cpp driving src/bms.cpp) as the device runs it: vectorised over features, bit-exact by
construction -- every fp64 operation in the order mmseq_amd/csrc/diff_kernels.h performs it, the keyed streams of mmg_math.h
restated with a numpy Philox4x32-10 (checked against the oracle), dlog / dexp through the oracle's log_v / exp_v.

Rejection samplers draw per lane: each feature has its own block counter c3, and a lane that rejects draws again while the others
wait behind a mask."""
import math
import os

import numpy as np

TAG_DIFF, TAG_DIFF_PERM = 7, 8
OUTLEN, MAXBATCHES, BATCH = 1024, 8192, 128
LOGIT07 = 0.8472979
M32 = np.uint64(0xFFFFFFFF)


def _B():
    from oracle import binding
    return binding


def dlog(x):
    return _B().log_v(np.asarray(x, np.float64))


def dexp(x):
    return _B().exp_v(np.asarray(x, np.float64))


# ----------------------------------------------------------------------------- Philox4x32-10 and the keyed stream
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 arrays (broadcast), keys scalars: the four output words."""
    x, y, z, w = (np.asarray(v, np.uint64) & M32 for v in (c0, c1, c2, c3))
    x, y, z, w = np.broadcast_arrays(x, y, z, w)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * x
        p1 = np.uint64(0xCD9E8D57) * z
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        x, y, z, w = hi1 ^ y ^ np.uint64(k0), lo1, hi0 ^ w ^ np.uint64(k1), lo0
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in (x, y, z, w)]


def u52(a, b):
    v = ((np.asarray(a, np.uint64) >> np.uint64(6)) << np.uint64(26)) | (np.asarray(b, np.uint64) >> np.uint64(6))
    return (v.astype(np.float64) + 0.5) * 2.0 ** -52


def stream_key(seed, chain, tag):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, ((seed >> 32) ^ (chain & 0x00FFFFFF) ^ (tag << 24)) & 0xFFFFFFFF


class Streams:
    """Stream(seed, 0, tag, id, it) for a vector of ids at one iteration; c3 per lane."""

    def __init__(self, seed, tag, ids, it):
        self.k0, self.k1 = stream_key(seed, 0, tag)
        self.ids = np.asarray(ids, np.uint64)
        self.it = it
        self.c3 = np.zeros(self.ids.size, np.uint64)

    def pair(self, idx):
        r = philox(self.ids[idx] & M32, self.ids[idx] >> np.uint64(32), np.uint64(self.it), self.c3[idx], self.k0, self.k1)
        self.c3[idx] += np.uint64(1)
        return u52(r[0], r[1]), u52(r[2], r[3])

    def uniform(self, act):
        out = np.full(self.ids.size, np.nan)
        idx = np.nonzero(act)[0]
        if idx.size:
            out[idx] = self.pair(idx)[0]
        return out

    def normal(self, act):
        out = np.full(self.ids.size, np.nan)
        pend = np.array(act, bool)
        while pend.any():
            idx = np.nonzero(pend)[0]
            ua, ub = self.pair(idx)
            v1, v2 = 2.0 * ua - 1.0, 2.0 * ub - 1.0
            r2 = v1 * v1 + v2 * v2
            ok = ~((r2 >= 1.0) | (r2 == 0.0))
            if ok.any():
                r = r2[ok]
                out[idx[ok]] = v1[ok] * np.sqrt(-2.0 * dlog(r) / r)
            pend[idx[ok]] = False
        return out

    def gamma_unit(self, act, a_in):
        """mmg_math.h gamma_unit, the host form (Marsaglia-Tsang over the polar normal; a < 1 boosted)."""
        n = self.ids.size
        a_in = np.broadcast_to(np.asarray(a_in, np.float64), (n,)).copy()
        out = np.full(n, np.nan)
        with np.errstate(all="ignore"):
            a = np.where(a_in < 1.0, a_in + 1.0, a_in)
            d = a - 1.0 / 3.0
            c = (1.0 / 3.0) / np.sqrt(d)
        active = np.array(act, bool)
        x = np.zeros(n)
        v = np.zeros(n)
        while active.any():
            pend = active.copy()
            while pend.any():
                z = self.normal(pend)
                x[pend] = z[pend]
                v[pend] = 1.0 + c[pend] * x[pend]
                pend &= v <= 0.0
            idx = np.nonzero(active)[0]
            vv = v[idx] * v[idx] * v[idx]
            ua, _ = self.pair(idx)
            x2 = x[idx] * x[idx]
            acc = ua < 1.0 - 0.0331 * x2 * x2
            with np.errstate(all="ignore"):
                acc2 = dlog(ua) < 0.5 * x2 + d[idx] * (1.0 - vv + dlog(vv))
            done = acc | acc2
            out[idx[done]] = d[idx[done]] * vv[done]
            active[idx[done]] = False
        small = np.array(act, bool) & (a_in < 1.0)
        if small.any():
            idx = np.nonzero(small)[0]
            ua, _ = self.pair(idx)
            out[idx] = out[idx] * dexp(dlog(ua) / a_in[idx])
        return out


def seq_uniforms(seed, tag, ident, n):
    """SeqStream over Stream(seed, 0, tag, ident, 0): the first uniform of each pair, then the second."""
    k0, k1 = stream_key(seed, 0, tag)
    out = []
    c3 = 0
    while len(out) < n:
        r = philox(ident & 0xFFFFFFFF, ident >> 32, 0, c3, k0, k1)
        c3 += 1
        out.append(float(u52(r[0], r[1])))
        out.append(float(u52(r[2], r[3])))
    return out[:n]


def permutation(seed, feature, S):
    """mmdiff -permute: Fisher-Yates keyed (seed, 0, TAG_DIFF_PERM, feature, 0)."""
    idx = list(range(S))
    u = seq_uniforms(seed, TAG_DIFF_PERM, feature, max(S - 1, 0))
    for n, j in enumerate(range(S - 1, 0, -1)):
        k = min(int(u[n] * float(j + 1)), j)
        idx[j], idx[k] = idx[k], idx[j]
    return idx


# ----------------------------------------------------------------------------- dlgamma and the moment matching
def dlgamma(x):
    x = np.array(x, np.float64, ndmin=1, copy=True)
    bad = ~(x > 0.0)                       # x <= 0 and NaN: NaN; +inf: +inf (mmg_math.h dlgamma)
    posinf = x == np.inf
    x[bad | posinf] = 8.0
    prod = np.ones_like(x)
    m = x < 8.0
    while m.any():
        prod[m] = prod[m] * x[m]
        x[m] = x[m] + 1.0
        m = x < 8.0
    z = 1.0 / x
    z2 = z * z
    ser = z * (1.0 / 12.0 + z2 * (-1.0 / 360.0 + z2 * (1.0 / 1260.0 + z2 * (-1.0 / 1680.0 + z2 * (1.0 / 1188.0
          + z2 * (-691.0 / 360360.0 + z2 * (1.0 / 156.0 + z2 * (-3617.0 / 122400.0))))))))
    out = ((((x - 0.5) * dlog(x) - x) + 0.91893853320467274178) + ser) - dlog(prod)
    out[bad] = np.nan
    out[posinf] = np.inf
    return out


def shape_from(res, res2):
    """Gamma shape by moment matching from the mean and the mean log: (3 - s + sqrt((s - 3)^2 + 24 s)) / (12 s), s = log(res) - res2."""
    s_ = dlog(res) - res2
    t = s_ - 3.0
    return ((3.0 - s_) + np.sqrt(t * t + 24.0 * s_)) / (12.0 * s_)


def is_nil(X):
    X = np.asarray(X, np.float64)
    return X.shape[1] == 1 and X.max() - X.min() < 0.00001


# ----------------------------------------------------------------------------- the sampler
class BMS:
    def __init__(self, y, e, M, P0, P1, C, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234):
        self.y = np.ascontiguousarray(y, np.float64)
        e = np.asarray(e, np.float64)
        self.esq = e * e
        self.F, self.N = self.y.shape
        self.M = np.asarray(M, np.float64)
        self.P = [np.asarray(P0, np.float64), np.asarray(P1, np.float64)]
        self.C = np.asarray(C, np.int64)
        self.K = self.M.shape[1]
        self.L = [self.P[0].shape[1], self.P[1].shape[1]]
        self.nc = [int(self.C[:, m].max()) + 1 for m in range(2)]
        self.Mnil = is_nil(self.M)
        self.Pnil = [is_nil(self.P[0]), is_nil(self.P[1])]
        self.d, self.s, self.fixalpha, self.seed = float(d), float(s), bool(fixalpha), int(seed)
        self.v_beta = 25.0 if fixalpha else 4.0
        F, K = self.F, self.K
        self.st = []
        for m in range(2):
            L, nc = self.L[m], self.nc[m]
            z = lambda *sh: np.zeros((F,) + sh)
            f = lambda v, *sh: np.full((F,) + sh, v)
            self.st.append(dict(alpha=z(), A=z(), Va=f(25.0), aS=z(), aSS=z(), aN=z(), rho=f(0.2), Q=f(2.0), R=f(10.0), rS=z(), rlS=z(),
                                beta=z(K), B=z(K), Vb=f(1.0, K), bS=z(K), bSS=z(K), bN=z(K),
                                eta=z(L), Fm=z(L), Ve=f(1.0, L), eS=z(L), eSS=z(L), eN=z(L),
                                lam=f(self.s / (self.d - 1.0), L), D=z(L), Si=f(1.0 / self.s, L), lS=z(L), llS=z(L),
                                sig=f(0.5, nc), J=f(2.0, nc), Lm=f(0.5, nc), sS=z(nc), slS=z(nc)))
        self.gam = np.zeros(F, np.int64)
        self.tuned = np.zeros(F, bool)
        self.gsum = np.zeros(F)
        self.logitp = np.full(F, math.log(pdash) - math.log(1.0 - pdash) if 0 < pdash < 1 else
                              (-math.inf if pdash == 0 else math.inf))
        self.LOsum = np.zeros(F)
        self.burnin_iters = 0
        self.batches = 0
        self.sampled = 0

    # per-sample helpers: (F, N)
    def mb(self, m):
        if self.Mnil:
            return np.zeros((self.F, self.N))
        acc = np.zeros((self.F, self.N))
        for j in range(self.K):
            acc = acc + self.M[None, :, j] * self.st[m]["beta"][:, j:j + 1]
        return acc

    def pe(self, m):
        if self.Pnil[m]:
            return np.zeros((self.F, self.N))
        P = self.P[m]
        acc = np.zeros((self.F, self.N))
        for l in range(self.L[m]):
            acc = acc + P[None, :, l] * self.st[m]["eta"][:, l:l + 1]
        return acc

    def ec(self, m):
        return self.esq + self.st[m]["sig"][:, self.C[:, m]]

    def upd_alpha(self, m, fit, pse, rec, rs):
        if self.fixalpha:
            return
        S = self.st[m]
        ec, mb, pe = self.ec(m), self.mb(m), self.pe(m)
        V = np.zeros(self.F)
        for i in range(self.N):
            V = V + 1.0 / ec[:, i]
        V = V + 1.0 / 25.0
        V = 1.0 / V
        sm = np.zeros(self.F)
        for i in range(self.N):
            sm = sm + ((self.y[:, i] - mb[:, i]) - pe[:, i]) / ec[:, i]
        zf, zp = rs.normal(fit), rs.normal(pse)
        a = np.where(fit, zf * np.sqrt(V) + V * sm, zp * np.sqrt(S["Va"]) + S["A"])
        lanes = fit | pse
        S["alpha"] = np.where(lanes, a, S["alpha"])
        if rec:
            S["aS"] = np.where(fit, S["aS"] + a, S["aS"])
            S["aSS"] = np.where(fit, S["aSS"] + a * a, S["aSS"])
            S["aN"] = np.where(fit, S["aN"] + 1.0, S["aN"])

    def upd_beta(self, m, fit, pse, rec, rs):
        if self.Mnil:
            return
        S, K, M = self.st[m], self.K, self.M
        F = self.F
        ec, pe = self.ec(m), self.pe(m)
        alpha = S["alpha"]
        G = [[np.zeros(F) for _ in range(K)] for _ in range(K)]
        t = [np.zeros(F) for _ in range(K)]
        for i in range(self.N):
            w = 1.0 / ec[:, i]
            r = (self.y[:, i] - alpha) - pe[:, i]
            for a in range(K):
                mw = M[i, a] * w
                for b in range(K):
                    G[a][b] = G[a][b] + mw * M[i, b]
                t[a] = t[a] + mw * r
        for a in range(K):
            G[a][a] = G[a][a] + 1.0 / self.v_beta

        def chol(A):
            Lc = [[None] * K for _ in range(K)]
            for j in range(K):
                sd = A[j][j]
                for k in range(j):
                    sd = sd - Lc[j][k] * Lc[j][k]
                Lc[j][j] = np.sqrt(sd)
                for i in range(j + 1, K):
                    u = A[i][j]
                    for k in range(j):
                        u = u - Lc[i][k] * Lc[j][k]
                    Lc[i][j] = u / Lc[j][j]
            return Lc

        with np.errstate(all="ignore"):
            Lg = chol(G)
            Li = [[None] * K for _ in range(K)]
            for j in range(K):
                Li[j][j] = 1.0 / Lg[j][j]
                for i in range(j + 1, K):
                    u = np.zeros(F)
                    for k in range(j, i):
                        u = u - Lg[i][k] * Li[k][j]
                    Li[i][j] = u / Lg[i][i]
            V = [[None] * K for _ in range(K)]
            for a in range(K):
                for b in range(K):
                    u = np.zeros(F)
                    for k in range(max(a, b), K):
                        u = u + Li[k][a] * Li[k][b]
                    V[a][b] = u
            Lv = chol(V)
        z = [rs.normal(fit) for _ in range(K)]
        newb = S["beta"].copy()
        for a in range(K):
            c = np.zeros(F)
            for b in range(a + 1):
                c = c + Lv[a][b] * z[b]
            mu = np.zeros(F)
            for b in range(K):
                mu = mu + V[a][b] * t[b]
            newb[:, a] = np.where(fit, c + mu, newb[:, a])
        for a in range(K):
            zp = rs.normal(pse)
            newb[:, a] = np.where(pse, zp * np.sqrt(S["Vb"][:, a]) + S["B"][:, a], newb[:, a])
        S["beta"] = newb
        if rec:
            lanes = (fit | pse)[:, None]
            S["bS"] = np.where(lanes, S["bS"] + newb, S["bS"])
            S["bSS"] = np.where(lanes, S["bSS"] + newb * newb, S["bSS"])
            S["bN"] = np.where(lanes, S["bN"] + 1.0, S["bN"])

    def upd_eta(self, m, fit, pse, rec, rs):
        if self.Pnil[m]:
            return
        S, P = self.st[m], self.P[m]
        alpha = S["alpha"]
        mb = self.mb(m)
        for l in range(self.L[m]):
            ec = self.ec(m)
            pe = self.pe(m)
            V = 1.0 / S["lam"][:, l]
            for i in range(self.N):
                V = V + (P[i, l] * P[i, l]) / ec[:, i]
            V = 1.0 / V
            el = S["eta"][:, l]
            sm = np.zeros(self.F)
            for i in range(self.N):
                pev = pe[:, i] - P[i, l] * el
                sm = sm + (P[i, l] * (((self.y[:, i] - mb[:, i]) - alpha) - pev)) / ec[:, i]
            zf, zp = rs.normal(fit), rs.normal(pse)
            new = np.where(fit, zf * np.sqrt(V) + V * sm, np.where(pse, zp * np.sqrt(S["Ve"][:, l]) + S["Fm"][:, l], el))
            S["eta"] = S["eta"].copy()
            S["eta"][:, l] = new
        if rec:
            f2 = fit[:, None]
            e = S["eta"]
            S["eS"] = np.where(f2, S["eS"] + e, S["eS"])
            S["eSS"] = np.where(f2, S["eSS"] + e * e, S["eSS"])
            S["eN"] = np.where(f2, S["eN"] + 1.0, S["eN"])

    def upd_lambda(self, m, fit, pse, rec, rs):
        if self.Pnil[m]:
            return
        S = self.st[m]
        lam = S["lam"].copy()
        for l in range(self.L[m]):
            e = S["eta"][:, l]
            gf = rs.gamma_unit(fit, self.d + 0.5)
            gp = rs.gamma_unit(pse, S["D"][:, l])
            with np.errstate(all="ignore"):
                vf = 1.0 / (gf * (1.0 / (self.s + (0.5 * e) * e)))
                vp = 1.0 / (gp * S["Si"][:, l])
            lam[:, l] = np.where(fit, vf, np.where(pse, vp, lam[:, l]))
        S["lam"] = lam
        if rec:
            lanes = (fit | pse)[:, None]
            tmp = 1.0 / lam
            S["lS"] = np.where(lanes, S["lS"] + tmp, S["lS"])
            S["llS"] = np.where(lanes, S["llS"] + dlog(tmp), S["llS"])

    def upd_sigmasq(self, m, fit, pse, rec, rs):
        S = self.st[m]
        nc, k, g = self.nc[m], 4.0, 2.0
        alpha, rho = S["alpha"], S["rho"]
        sig = S["sig"].copy()
        with np.errstate(all="ignore"):
            lsig = [dlog(sig[:, c]) for c in range(nc)]
            lprop, prop = [], []
            for c in range(nc):
                z = rs.normal(fit)
                lprop.append(z * g + lsig[c])
                prop.append(dexp(lprop[c]))
            mb, pe = self.mb(m), self.pe(m)
            sm = [np.zeros(self.F) for _ in range(nc)]
            for i in range(self.N):
                c = int(self.C[i, m])
                tmp = ((self.y[:, i] - alpha) - mb[:, i]) - pe[:, i]
                es, sc = self.esq[:, i], sig[:, c]
                sm[c] = sm[c] + (dlog(es + prop[c]) - dlog(es + sc)) + (tmp * tmp) * ((1.0 / (es + prop[c])) - (1.0 / (es + sc)))
            for c in range(nc):
                sc = sig[:, c]
                logar = ((-0.5 * sm[c]) - ((0.5 * k) * rho) * ((1.0 / prop[c]) - (1.0 / sc))) - (0.5 * k) * (lprop[c] - lsig[c])
                u = rs.uniform(fit)
                acc = fit & (logar > dlog(u))
                sig[:, c] = np.where(acc, prop[c], sig[:, c])
            for c in range(nc):
                gp = rs.gamma_unit(pse, S["J"][:, c])
                sig[:, c] = np.where(pse, 1.0 / (gp * (1.0 / S["Lm"][:, c])), sig[:, c])
        S["sig"] = sig
        if rec:
            lanes = (fit | pse)[:, None]
            tmp = 1.0 / sig
            S["sS"] = np.where(lanes, S["sS"] + tmp, S["sS"])
            S["slS"] = np.where(lanes, S["slS"] + dlog(tmp), S["slS"])

    def upd_rho(self, m, fit, pse, rec, rs):
        S = self.st[m]
        nc, k, q, r = self.nc[m], 4.0, 1.2, 2.0
        sm = np.zeros(self.F)
        for c in range(nc):
            sm = sm + 1.0 / S["sig"][:, c]
        gf = rs.gamma_unit(fit, (float(nc) * 0.5) * k + q)
        gp = rs.gamma_unit(pse, S["Q"])
        with np.errstate(all="ignore"):
            rho = np.where(fit, gf * (1.0 / (r + (0.5 * k) * sm)), np.where(pse, gp * (1.0 / S["R"]), S["rho"]))
        S["rho"] = rho
        if rec:
            lanes = fit | pse
            S["rS"] = np.where(lanes, S["rS"] + rho, S["rS"])
            S["rlS"] = np.where(lanes, S["rlS"] + dlog(rho), S["rlS"])

    def log_posterior(self, m):
        S = self.st[m]
        k, q, r = 4.0, 1.2, 2.0
        alpha, rho = S["alpha"], S["rho"]
        ec, mb, pe = self.ec(m), self.mb(m), self.pe(m)
        sm = np.zeros(self.F)
        sm2 = np.zeros(self.F)
        for i in range(self.N):
            sm = sm + dlog(ec[:, i])
            dd = ((self.y[:, i] - alpha) - mb[:, i]) - pe[:, i]
            sm2 = sm2 + (dd * dd) / ec[:, i]
        res = np.zeros(self.F)
        res = res + ((-0.5 * sm) - 0.5 * sm2)
        res = res + ((-0.5 * alpha) * alpha) / 25.0
        if not self.Mnil:
            ss = np.zeros(self.F)
            for j in range(self.K):
                ss = ss + S["beta"][:, j] * S["beta"][:, j]
            res = res + (-0.5 / self.v_beta) * ss
        sm = np.zeros(self.F)
        if not self.Pnil[m]:
            lgd = float(dlgamma(self.d)[0])
            lss = float(dlog(np.array([self.s]))[0])
            for l in range(self.L[m]):
                e, lam = S["eta"][:, l], S["lam"][:, l]
                # src/bms.cpp:948-949 adds the column's whole term to the sum: `sum += a - b + c - d - e`, so s / lambda is taken from
                # the term, not from the running sum (the two differ in the last bits from the second column on)
                sm = sm + ((((((-0.5 * e) * e) / lam - (1.5 + self.d) * dlog(lam)) + self.d * lss) - lgd) - self.s / lam)
        for c in range(self.nc[m]):
            sg = S["sig"][:, c]
            sm = sm + (((k / 2.0) * dlog(rho) - (k * rho) / (2.0 * sg)) - (1.0 + k / 2.0) * dlog(sg))
        res = res + sm
        nc = float(self.nc[m])
        res = res + (((k * nc) / 2.0) * float(dlog(np.array([k / 2.0]))[0]) - nc * float(dlgamma(k / 2.0)[0]))
        res = res + ((q - 1.0) * dlog(rho) - r * rho)
        return res

    def log_pseudo(self, m):
        S = self.st[m]
        res = np.zeros(self.F)
        if not self.fixalpha:
            da, va = S["alpha"] - S["A"], S["Va"]
            res = res + ((-0.5 * dlog(va)) - (0.5 * (da * da)) / va)
        if not self.Mnil:
            for l in range(self.K):
                db, vb = S["beta"][:, l] - S["B"][:, l], S["Vb"][:, l]
                res = res + ((-0.5 * dlog(vb)) - (0.5 * (db * db)) / vb)
        sm = np.zeros(self.F)
        if not self.Pnil[m]:
            for l in range(self.L[m]):
                de, ve = S["eta"][:, l] - S["Fm"][:, l], S["Ve"][:, l]
                D, Si, lam = S["D"][:, l], S["Si"][:, l], S["lam"][:, l]
                sm = sm + ((-0.5 * dlog(ve)) - (0.5 * (de * de)) / ve)
                sm = sm + (D * dlog(1.0 / Si) - (D + 1.0) * dlog(lam))
                sm = sm + ((-dlgamma(D)) - 1.0 / (Si * lam))
        for c in range(self.nc[m]):
            J, L, sg = S["J"][:, c], S["Lm"][:, c], S["sig"][:, c]
            sm = sm + (J * dlog(L) - dlgamma(J))
            sm = sm + ((-J - 1.0) * dlog(sg) - L / sg)
        res = res + sm
        Q, R, rho = S["Q"], S["R"], S["rho"]
        res = res + (Q * dlog(R) - dlgamma(Q))
        res = res + ((Q - 1.0) * dlog(rho) - R * rho)
        return res

    def iteration(self, lanes, it, inburnin, rec):
        rs = Streams(self.seed, TAG_DIFF, np.arange(self.F), it)
        g = self.gam
        fits = [lanes & (inburnin | (g == m)) for m in range(2)]
        pses = [lanes & ~fits[m] for m in range(2)]
        with np.errstate(all="ignore"):
            for upd in (self.upd_alpha, self.upd_beta, self.upd_eta, self.upd_lambda, self.upd_sigmasq, self.upd_rho):
                for m in range(2):
                    upd(m, fits[m], pses[m], rec, rs)
            if not inburnin:
                LO = (((self.log_posterior(1) + self.log_pseudo(0)) - self.log_posterior(0)) - self.log_pseudo(1)) + self.logitp
                u = rs.uniform(lanes)
                x = dlog(u) - dlog(1.0 - u)
                self.LOsum = np.where(lanes, self.LOsum + LO, self.LOsum)
                ng = (x < LO).astype(np.int64)
                self.gam = np.where(lanes, ng, self.gam)
                if rec:
                    self.gsum = np.where(lanes, self.gsum + ng, self.gsum)

    # ---- phases, as the mmg_diff_* entries drive them
    def burnin(self, iters):
        allf = np.ones(self.F, bool)
        for t in range(iters):
            self.iteration(allf, t, True, t >= OUTLEN // 10)
        n = float(iters - OUTLEN // 10)
        with np.errstate(all="ignore"):
            for m in range(2):
                S = self.st[m]
                if not self.fixalpha:
                    S["A"] = S["aS"] / n
                    S["Va"] = (S["aSS"] - (S["aS"] * S["aS"]) / n) / (n - 1.0)
                if not self.Mnil:
                    S["B"] = S["bS"] / n
                    S["Vb"] = (S["bSS"] - (S["bS"] * S["bS"]) / n) / (n - 1.0)
                if not self.Pnil[m]:
                    S["Fm"] = S["eS"] / n
                    S["Ve"] = (S["eSS"] - (S["eS"] * S["eS"]) / n) / (n - 1.0)
                    res, res2 = S["lS"] / n, S["llS"] / n
                    D = np.stack([shape_from(res[:, l], res2[:, l]) for l in range(self.L[m])], 1)
                    S["D"], S["Si"] = D, res / D
                res, res2 = S["sS"] / n, S["slS"] / n
                J = np.stack([shape_from(res[:, c], res2[:, c]) for c in range(self.nc[m])], 1)
                S["J"], S["Lm"] = J, J / res
                res, res2 = S["rS"] / n, S["rlS"] / n
                Q = shape_from(res, res2)
                S["Q"], S["R"] = Q, Q / res
                for key in ("aS", "aSS", "aN", "rS", "rlS", "bS", "bSS", "bN", "eS", "eSS", "eN", "lS", "llS", "sS", "slS"):
                    S[key] = np.zeros_like(S[key])
        self.gsum = np.zeros(self.F)
        self.burnin_iters = iters

    def tune_batch(self):
        b = self.batches
        t0 = b * BATCH
        it0 = self.burnin_iters + t0
        lanes = np.ones(self.F, bool)
        first = lanes.copy()
        if b > 0:
            lanes = ~self.tuned
            mp = self.LOsum / float(BATCH)
            now = lanes & (mp > -LOGIT07) & (mp < LOGIT07)
            step = 1.0 / math.sqrt(float(2 + t0 // BATCH))
            adj = lanes & ~now
            self.logitp = np.where(adj & (mp > 0), self.logitp - step, np.where(adj, self.logitp + step, self.logitp))
            self.LOsum = np.where(adj, 0.0, self.LOsum)
            self.tuned = self.tuned | now
            first = lanes
            lanes = adj
        untuned = int(lanes.sum())
        for j in range(BATCH):
            act = first if j == 0 else lanes
            if act.any():
                self.iteration(act, it0 + j, False, False)
        self.batches += 1
        return untuned

    def sample(self, iters):
        t_first = self.batches * BATCH + self.sampled
        allf = np.ones(self.F, bool)
        for j in range(iters):
            self.iteration(allf, self.burnin_iters + t_first + j, False, True)
        self.sampled += iters

    def results(self):
        with np.errstate(all="ignore"):
            gm = self.gsum / float(self.sampled)
            alpha = np.stack([self.st[m]["aS"] / self.st[m]["aN"] for m in range(2)])
            beta = np.stack([(self.st[m]["bS"] / self.st[m]["bN"]).T for m in range(2)])
            eta = np.concatenate([(self.st[m]["eS"] / self.st[m]["eN"]).T for m in range(2)])
        return dict(gamma_mean=gm, logitp=self.logitp.copy(), alpha=alpha, beta=beta, eta=eta)


def run_bms(y, e, M, P0, P1, C, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, burnin=8192, iters=16384, tune=True,
            max_batches=MAXBATCHES):
    b = BMS(y, e, M, P0, P1, C, d, s, pdash, fixalpha, seed)
    b.burnin(burnin)
    if tune:
        untuned = b.tune_batch()
        nb = 1
        while untuned > 0 and nb != max_batches:
            untuned = b.tune_batch()
            nb += 1
    b.sample(iters)
    return b, b.results()


# ----------------------------------------------------------------------------- the CLI around it
def fmt(x):
    x = float(x)
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%g" % x


def read_table(path, useprops=False):
    with open(path) as f:
        lines = f.read().split("\n")
    i = 0
    while lines[i].startswith("#"):
        i += 1
    hdr = [t for t in lines[i].split("\t") if t]
    ycol = "mean_probit_proportion" if useprops else "log_mu"
    ecol = "sd_probit_proportion" if useprops else "sd"
    fi, yi, ei, ui = (hdr.index(c) for c in ("feature_id", ycol, ecol, "unique_hits"))
    feats, y, e, uh = [], [], [], []
    for ln in lines[i + 1:-1]:           # the reference drops a last line without a newline
        tok = [t for t in ln.split("\t") if t]
        feats.append(tok[fi])
        y.append(float(tok[yi]))
        e.append(float(tok[ei]))
        uh.append(float(tok[ui]))
    return feats, np.array(y), np.array(e), np.array(uh)


def normalise(y, uh, uhfrac):
    F, S = y.shape
    use = [i for i in range(F) if sum(1 for j in range(S) if uh[i, j] > 0) / float(S) >= uhfrac]
    if len(use) < 100:
        return y, None
    y = y.copy()
    means = []
    for i in use:
        sm = 0.0
        for j in range(S):
            sm += y[i, j]
        means.append(sm / float(S))
    factors = []
    for j in range(S):
        dif = sorted(y[i, j] - means[n] for n, i in enumerate(use))
        mf = dif[len(dif) // 2]
        factors.append(mf)
        y[:, j] = y[:, j] - mf
    return y, factors


def de_design(groups):
    S = sum(groups)
    G = len(groups)
    M = np.zeros((S, 1))
    P0 = np.zeros((S, 1))
    P1 = np.zeros((S, G if G > 2 else 1))
    C = np.zeros((S, 2), np.int64)
    k = 0
    for i, n in enumerate(groups):
        for _ in range(n):
            C[k, 1] = i
            P0[k, 0] = 1.0
            if G > 2:
                P1[k, i] = 1.0
            else:
                P1[k, 0] = 0.5 if i == 0 else -0.5
            k += 1
    return M, P0, P1, C


def mmdiff(files, groups=None, design=None, p=0.1, d=1.4, s=2.0, fixalpha=False, normalise_=True, pdash=0.5, tune=True,
           uhfrac=None, burnin=8192, iters=16384, seed=1234, permute=False, max_batches=MAXBATCHES):
    """The stdout of `mmdiff` on these tables (no -range, no -useprops): the formatted table as one string."""
    tabs = [read_table(f) for f in files]
    feats = tabs[0][0]
    y = np.stack([t[1] for t in tabs], 1)
    e = np.stack([t[2] for t in tabs], 1)
    uh = np.stack([t[3] for t in tabs], 1)
    S = len(files)
    if uhfrac is None:
        uhfrac = max(0.2, float(S - S * S // 160) / float(S))
    if normalise_:
        y, _ = normalise(y, uh, uhfrac)
    if permute:
        for f in range(y.shape[0]):
            idx = permutation(seed & 0xFFFFFFFF, f, S)
            y[f] = y[f, idx]
            e[f] = e[f, idx]
    M, P0, P1, C = de_design(groups) if design is None else design
    b, r = run_bms(y, e, M, P0, P1, C, d, s, pdash, fixalpha, seed & 0xFFFFFFFF, burnin, iters, tune, max_batches)
    out = ["#prior_probability=%s\n" % fmt(p)]
    hdr = "feature_id\tbayes_factor\tposterior_probability\t"
    for m in range(2):
        if not fixalpha:
            hdr += "alpha%d\t" % m
        if not b.Mnil:
            hdr += "".join("beta%d_%d\t" % (m, l) for l in range(b.K))
        if not b.Pnil[m]:
            hdr += "".join("eta%d_%d\t" % (m, l) for l in range(b.L[m]))
    names = []
    for f in files:
        n = f
        if f.endswith(".mmseq"):
            n = f[f.rfind("/") + 1:f.rfind(".")]
        names.append(n)
    hdr += "".join("mu_%s\t" % n for n in names) + "\t".join("sd_%s" % n for n in names) + "\n"
    out.append(hdr)
    logp, log1mp = math.log(p) if p > 0 else -math.inf, math.log1p(-p) if p < 1 else -math.inf
    for f in range(len(feats)):
        g = float(r["gamma_mean"][f])
        lg = float(r["logitp"][f])
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
        row = "%s\t%s\t%s\t" % (feats[f], fmt(BF), fmt(pp))
        for m in range(2):
            if not fixalpha:
                row += fmt(r["alpha"][m, f]) + "\t"
            if not b.Mnil:
                row += "".join(fmt(r["beta"][m, l, f]) + "\t" for l in range(b.K))
            if not b.Pnil[m]:
                off = b.L[0] if m else 0
                row += "".join(fmt(r["eta"][off + l, f]) + "\t" for l in range(b.L[m]))
        row += "".join(fmt(v) + "\t" for v in y[f]) + "\t".join(fmt(v) for v in e[f]) + "\n"
        out.append(row)
    return "".join(out)
