"""Restatement of `mmdiff -lrt FILE -lrtperm B` on top of the restatements it joins: copy b's data is
tests/mmdiff_perm_ref.py's replica b, each copy's test is tests/mmdiff_lrt_ref.py's `lrt`, the per-feature counts and perm_p are plain
loops written from include/mmgibbs.h, the pooled columns are tests/qvalue_ref.py's.  Also the FILE formatter and the device-memory
formula of the handle."""
import numpy as np

import mmdiff_lrt_ref as L
import qvalue_ref as Q
from mmdiff_perm_ref import replica_data
from mmdiff_ref import fmt

SLAB_BYTES = 1 << 30
MAX_PERMS = 65535


def counts(obs, null):
    """obs (F,), null (B, F): perm_ge, perm_n (uint64) and perm_p.  A NaN copy counts in neither; -0.0 equals 0.0 (IEEE >=); an
    observed NaN gives perm_ge 0 and perm_p NaN."""
    obs, null = np.asarray(obs, np.float64), np.asarray(null, np.float64)
    B, F = null.shape
    ge, n, p = np.zeros(F, np.uint64), np.zeros(F, np.uint64), np.full(F, np.nan)
    for f in range(F):
        t0 = float(obs[f])
        g = m = 0
        for b in range(B):
            t = float(null[b, f])
            if t != t:
                continue
            m += 1
            if t0 == t0 and t >= t0:
                g += 1
        ge[f], n[f] = g, m
        if t0 == t0:
            p[f] = float(1 + g) / float(1 + m)
    return ge, n, p


def null_fits(y, e, M, P0, P1, C, B, seed, fixalpha=False, max_iters=0):
    """stat (B, F) and status (B, F) uint8 = status0 | status1 << 4 of the test on copies 1 .. B."""
    F = np.asarray(y).shape[0]
    stat, status = np.empty((B, F)), np.empty((B, F), np.uint8)
    for b in range(1, B + 1):
        yb, eb = replica_data(y, e, seed, b)
        r = L.lrt(yb, eb, M, P0, P1, C, fixalpha, max_iters)
        stat[b - 1] = r["stat"]
        status[b - 1] = (r["status"][0] | (r["status"][1] << 4)).astype(np.uint8)
    return stat, status


def lrt_perm(y, e, M, P0, P1, C, B, fixalpha=False, max_iters=0, seed=1234):
    """What DiffLrtPerm(...).results() returns."""
    r = L.lrt(y, e, M, P0, P1, C, fixalpha, max_iters)
    r["null_stat"], r["null_status"] = null_fits(y, e, M, P0, P1, C, B, seed, fixalpha, max_iters)
    r["perm_ge"], r["perm_n"], r["perm_p"] = counts(r["stat"], r["null_stat"])
    r["null_ge"], r["q_perm"] = Q.qvalues(r["stat"], r["null_stat"].ravel())
    return r


def lrt_perm_file(feats, r, M, P0, P1, fixalpha):
    """The text of `mmdiff -lrt FILE -lrtperm B` for the results r of `lrt_perm` (or of DiffLrtPerm): the plain file's lines with
    perm_ge, perm_p, null_ge, q_perm appended."""
    lines = L.lrt_file(feats, r, M, P0, P1, fixalpha).split("\n")
    assert lines[-1] == "" and len(lines) == len(feats) + 2
    lines[0] += "\tperm_ge\tperm_p\tnull_ge\tq_perm"
    for f in range(len(feats)):
        lines[1 + f] += "\t%d\t%s\t%d\t%s" % (r["perm_ge"][f], fmt(r["perm_p"][f]), r["null_ge"][f], fmt(r["q_perm"][f]))
    return "\n".join(lines)


def lrt_device_bytes(F, N, p, nc):
    """mmg_diff_lrt_device_bytes (include/mmgibbs.h)."""
    pm = max(p)
    W = 2 * max(nc) + (0 if pm <= 4 else pm * (pm + 1) // 2)
    return 8 * (2 * F * N + (N + F) * sum(p) + F * sum(nc) + 2 * F + F * W) + 4 * (2 * N + 4 * F)


def perm_wslots(p, nc):
    pm = max(p)
    return 3 * max(nc) + (0 if pm <= 4 else pm * (pm + 1) // 2 + pm)


def slab_copies(F, N, p, nc, B, asked=0):
    """The copies of one slab: what was asked for, or as many as keep 8 F (2 N + W') bytes per copy under 1 GiB; at least 1, at most B."""
    Sc = asked if asked else SLAB_BYTES // (8 * F * (2 * N + perm_wslots(p, nc)))
    return min(max(Sc, 1), B)


def perm_device_bytes(F, N, p, nc, B, asked=0):
    """mmg_diff_lrt_perm_device_bytes: the observed test's + 8 Sc F (2 N + W') + 9 B F + 48 F."""
    return lrt_device_bytes(F, N, p, nc) + 8 * slab_copies(F, N, p, nc, B, asked) * F * (2 * N + perm_wslots(p, nc)) + 9 * B * F + 48 * F
