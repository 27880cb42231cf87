"""The posterior log fold change of features between two samples, from all pairs of their draws (thin mirror of the mmg_fold_*
entries of include/mmgibbs.h).

Two samples are independent given their reads, so every pair (draw i of A, draw j of B) is a draw from the joint posterior of the log
fold change: Sa * Sb draws per feature.  This is the posterior given the reads of these two libraries; it says nothing about
biological variability -- for groups with replicates the tool is mmdiff.  From the device come, per feature: the means and centred
sums of squares of x = log a and y = log b + offset, the exact counts n_gt and n_eq of pairs with x_i > y_j and x_i == y_j, exact
order statistics of d_ij = x_i - y_j at the requested zero-based ranks, and a status byte (bit 0: a draw of A, bit 1: a draw of B is
not finite and > 0; such a feature is NaN with zero counts).  `summary()` adds lfc, sd and p_gt with IEEE arithmetic, `gfold(c)` the
conservative fold change from two of the ranks.  `Fold.of_traces` takes series-major host traces, `Fold.of_samplers` reads the
resident traces of two samplers that are past their last kept sample.  The specification is restated in tests/fold_ref.py.  No CPU
path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

DEVICE_COLUMNS = ("mean_a", "mean_b", "ss_a", "ss_b", "n_gt", "n_eq", "quantiles", "status")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u32(v, what):
    arr = np.asarray(v, np.int64).reshape(-1)
    if arr.size and (arr.min() < 0 or arr.max() > 0xffffffff):
        raise ValueError("%s must fit 32 unsigned bits" % what)
    return np.ascontiguousarray(arr, np.uint32)


def percentile_rank(p, n_pairs):
    """the zero-based rank of percentile p among n_pairs differences: mmseq -percentiles' rule with n_pairs - 1 for trace_len - 1
    (C's round: halves away from zero)"""
    v = float(p) / 100.0 * float(n_pairs - 1)
    fl = np.floor(v)
    return int(fl) + (1 if v - fl >= 0.5 else 0)


class Fold:
    def __init__(self, handle, n_features, Sa, Sb, ranks):
        self._lib = _lib.load()
        self._h = handle
        self.n_features, self.Sa, self.Sb = int(n_features), int(Sa), int(Sb)
        self.ranks = ranks

    @classmethod
    def of_traces(cls, a, b, offset=0.0, ranks=(), device=0):
        """a: (n_features, Sa), b: (n_features, Sb) draws on the mu scale; ranks: zero-based ranks among the Sa * Sb differences"""
        a = np.ascontiguousarray(a, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
            raise ValueError("a and b must be (n_features, Sa) and (n_features, Sb)")
        r = _u32(ranks, "ranks")
        h = C.c_void_p()
        check(_lib.load().mmg_fold_of_traces(int(device), a.shape[0], a.shape[1], _ptr(a), b.shape[1], _ptr(b), float(offset), r.size, _ptr(r), C.byref(h)))
        return cls(h, a.shape[0], a.shape[1], b.shape[1], r)

    @classmethod
    def of_samplers(cls, sampler_a, sampler_b, ia, ib, offset=0.0, ranks=(), chain_a=0, chain_b=0):
        """feature f: transcript ia[f] of `chain_a` of sampler_a against ib[f] of `chain_b` of sampler_b, the caller's numbering"""
        ia, ib, r = _u32(ia, "ia"), _u32(ib, "ib"), _u32(ranks, "ranks")
        if ia.size != ib.size:
            raise ValueError("ia and ib must have one entry per feature")
        h = C.c_void_p()
        check(_lib.load().mmg_fold_create(sampler_a._h, int(chain_a), sampler_b._h, int(chain_b), ia.size, _ptr(ia), _ptr(ib), float(offset), r.size,
                                          _ptr(r), C.byref(h)))
        return cls(h, ia.size, sampler_a.trace_len, sampler_b.trace_len, r)

    def summary(self):
        """the device columns per feature (quantiles: (n_features, n_ranks)), and lfc, sd, p_gt derived from them"""
        F = self.n_features
        out = {k: np.empty(F) for k in DEVICE_COLUMNS[:4]}
        out["n_gt"] = np.empty(F, np.uint32)
        out["n_eq"] = np.empty(F, np.uint32)
        out["quantiles"] = np.empty((F, self.ranks.size))
        out["status"] = np.empty(F, np.uint8)
        check(self._lib.mmg_fold_get(self._h, *[_ptr(out[k]) for k in DEVICE_COLUMNS]))
        out.update(derived(out, self.Sa, self.Sb))
        return out

    def gfold(self, c, summary=None):
        """lo if lo > 0, hi if hi < 0, else 0, with lo and hi the order statistics at the ranks of the percentiles 100 c and
        100 (1 - c); both ranks must have been requested.  NaN for an invalid feature."""
        s = summary if summary is not None else self.summary()
        n = self.Sa * self.Sb
        ranks = list(self.ranks)
        lo = s["quantiles"][:, ranks.index(percentile_rank(100.0 * c, n))]
        hi = s["quantiles"][:, ranks.index(percentile_rank(100.0 * (1.0 - c), n))]
        return gfold_of(lo, hi)

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_fold_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_fold_destroy(self._h)
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


def derived(dev, Sa, Sb):
    """lfc = mean_a - mean_b, sd = sqrt(ss_a / (Sa - 1) + ss_b / (Sb - 1)), p_gt = (n_gt + n_eq / 2) / (Sa Sb); NaN for a feature
    whose status is not 0"""
    with np.errstate(all="ignore"):
        p = (dev["n_gt"].astype(np.float64) + dev["n_eq"].astype(np.float64) / 2.0) / np.float64(Sa * Sb)
        return dict(lfc=dev["mean_a"] - dev["mean_b"], sd=np.sqrt(dev["ss_a"] / np.float64(Sa - 1) + dev["ss_b"] / np.float64(Sb - 1)),
                    p_gt=np.where(dev["status"] != 0, np.nan, p))


def gfold_of(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(lo) | np.isnan(hi), np.nan, np.where(lo > 0, lo, np.where(hi < 0, hi, 0.0)))
