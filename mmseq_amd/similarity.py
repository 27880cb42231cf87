"""Posterior distances and correlations between samples, from their joint draws (thin mirror of the mmg_sim_* entries of
include/mmgibbs.h).

Samples are independent given their reads, so draw t of every one of S samples together is one draw from the joint posterior of all S
expression profiles.  Per draw the device takes the Gram matrix of the S profiles over the used features (fp64, on the matrix cores)
and from it, per pair of samples, the root-mean-square log ratio D[t] and Pearson's correlation R[t] across the features, and per
sample its nearest neighbour.  Over the T draws come, per pair r < s (r-major): the means and centred sums of squares of D and R,
their order statistics at the requested zero-based ranks, a status byte (bit 1: R is undefined in some draw, every R output NaN),
and the counts nn[a][b] of the draws in which b is a's nearest.  `summary()` adds sd_D, sd_R and p_nearest = nn / T with IEEE
arithmetic.  A feature is used when the mask keeps it and all its S T values are valid; with fewer than two used features the status
has bit 0 and everything is NaN.  The specification is restated in tests/sim_ref.py.  No CPU path exists: without a device every call
raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

LOGGED = 1
MAX_RANKS = 64
DEVICE_COLUMNS = ("mean_D", "ss_D", "q_D", "mean_R", "ss_R", "q_R", "nn", "pair_status")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def percentile_rank(p, T):
    """the zero-based rank of percentile p among T draws: mmseq -percentiles' rule (C's round: halves away from zero)"""
    v = float(p) / 100.0 * float(T - 1)
    fl = np.floor(v)
    return int(fl) + (1 if v - fl >= 0.5 else 0)


def pairs_of(S):
    """the pairs (r, s), r < s, in the order of the per-pair outputs"""
    return [(r, s) for r in range(S) for s in range(r + 1, S)]


class Similarity:
    def __init__(self, S, F, T, centre=None, mask=None, logged=False, device=0):
        """S samples of T joint draws of F features; centre: (F,) subtracted from every log value (None: zeros); mask: (F,), zero
        where a feature is left out (None: none is); logged: the traces are on the log scale already"""
        self._lib = _lib.load()
        self._h = None
        self.S, self.F, self.T = int(S), int(F), int(T)
        self.ranks = np.zeros(0, np.uint32)
        if centre is not None:
            centre = np.ascontiguousarray(centre, np.float64)
            if centre.shape != (self.F,):
                raise ValueError("centre must have one entry per feature")
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            if mask.shape != (self.F,):
                raise ValueError("mask must have one entry per feature")
        for v, what in ((S, "S"), (F, "F"), (T, "T")):
            if not 0 <= int(v) <= 0xffffffff:
                raise ValueError("%s must fit 32 unsigned bits" % what)
        h = C.c_void_p()
        check(self._lib.mmg_sim_create(int(device), self.S, self.F, self.T, _ptr(centre), _ptr(mask), LOGGED if logged else 0, C.byref(h)))
        self._h = h

    def set_sample(self, s, trace, offset=0.0):
        """trace: (T, F), the rows of a trace file; offset on the natural-log scale.  A sample may be set again before run()."""
        trace = np.ascontiguousarray(trace, np.float64)
        if trace.shape != (self.T, self.F):
            raise ValueError("trace must be (T, F)")
        if not 0 <= int(s) <= 0xffffffff:
            raise ValueError("s must fit 32 unsigned bits")
        check(self._lib.mmg_sim_set_sample(self._h, int(s), _ptr(trace), float(offset)))

    def run(self, ranks=()):
        """both stages; ranks: zero-based ranks among the T draws (a rank >= T gives NaN)"""
        arr = np.asarray(ranks, np.int64).reshape(-1)
        if arr.size and (arr.min() < 0 or arr.max() > 0xffffffff):
            raise ValueError("ranks must fit 32 unsigned bits")
        r = np.ascontiguousarray(arr, np.uint32)
        check(self._lib.mmg_sim_run(self._h, r.size, _ptr(r)))
        self.ranks = r
        return self

    def used(self):
        """(used, n): the (F,) 0 / 1 bytes of the last run and their count"""
        u = np.empty(self.F, np.uint8)
        n = C.c_uint64()
        check(self._lib.mmg_sim_get_used(self._h, _ptr(u), C.byref(n)))
        return u, int(n.value)

    def z(self, s):
        """(T, F): the centred log values of sample s as they stand on the device (0.0 at the unused features once run() has run)"""
        out = np.empty((self.T, self.F))
        check(self._lib.mmg_sim_get_z(self._h, int(s), 0, self.T, _ptr(out)))
        return out

    def gram(self):
        """(G, m): (T, S, S) and (T, S), the stage-1 numbers of the last run"""
        G, m = np.empty((self.T, self.S, self.S)), np.empty((self.T, self.S))
        check(self._lib.mmg_sim_get_gram(self._h, 0, self.T, _ptr(G), _ptr(m)))
        return G, m

    def summary(self):
        """the device columns per pair (q_D, q_R: (pairs, n_ranks); nn: (S, S)), `status`, and sd_D, sd_R, p_nearest derived"""
        P, nr = self.S * (self.S - 1) // 2, self.ranks.size
        out = {k: np.empty(P) for k in ("mean_D", "ss_D", "mean_R", "ss_R")}
        out["q_D"], out["q_R"] = np.empty((P, nr)), np.empty((P, nr))
        out["nn"] = np.empty((self.S, self.S), np.uint32)
        out["pair_status"] = np.empty(P, np.uint8)
        st = np.empty(1, np.uint8)
        check(self._lib.mmg_sim_get(self._h, *([_ptr(out[k]) for k in DEVICE_COLUMNS] + [_ptr(st)])))
        out["status"] = int(st[0])
        out.update(derived(out, self.T))
        return out

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_sim_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_sim_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def derived(dev, T):
    """sd = sqrt(ss / (T - 1)) of D and of R, p_nearest = nn / T"""
    with np.errstate(all="ignore"):
        return dict(sd_D=np.sqrt(dev["ss_D"] / np.float64(T - 1)), sd_R=np.sqrt(dev["ss_R"] / np.float64(T - 1)),
                    p_nearest=dev["nn"].astype(np.float64) / np.float64(T))
