"""Posterior isoform usage within groups of transcripts of one sample (thin mirror of the mmg_isoform_* entries of include/mmgibbs.h).

Isoforms of one gene share their reads, so their draws are strongly anti-correlated; which isoform is the major one and with what
probability, whether the gene is dominated by one isoform or spread over several, and with what probability an isoform carries more
than a given share of the gene are questions about the joint draws of the gene's isoforms.  A group is an ordered list of distinct
members.  Per kept sample the device takes the group's total T, the member with the largest draw (`top`, the first of equals) and the
runner-up (`second`), the top member's share P and the entropy H of the shares; per member the exact counts of samples in which it is
the top, the second, and above each threshold share; per group the moments and order statistics of H and P, the major member and the
number of members that are ever the top.  `Isoforms.from_sampler` reads the chain a finished Summary was taken over, on the device;
`Isoforms.from_traces` takes series-major host traces.  `switch_probability` compares the same groups in two samples from their
counts.  The specification is restated in tests/isoforms_ref.py.  No CPU path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

NONE = 0xffffffff   # `second` of a group of one member; `top` and `second` of a group that is not valid


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(g) for g in lists])
    mem = np.array([m for g in lists for m in g], np.int64)
    if mem.size and (mem.min() < 0 or mem.max() > 0xffffffff):
        raise ValueError("members must fit 32 unsigned bits")
    return ptr, np.ascontiguousarray(mem, np.uint32)


def _ranks(v):
    arr = np.asarray(v, np.int64).reshape(-1)
    if arr.size and (arr.min() < 0 or arr.max() > 0xffffffff):
        raise ValueError("ranks must fit 32 unsigned bits")
    return np.ascontiguousarray(arr, np.uint32)


class Isoforms:
    def __init__(self, handle, ptr, n_samples, thresholds, ranks):
        self._lib = _lib.load()
        self._h = handle
        self.ptr = ptr
        self.n_groups, self.n_members, self.S = int(ptr.size - 1), int(ptr[-1]), int(n_samples)
        self.thresholds, self.ranks = thresholds, ranks

    @staticmethod
    def _desc(groups, thresholds, ranks):
        """groups: lists of members; the arrays are returned too (the description points into them)"""
        ptr, mem = _csr(groups)
        th = np.ascontiguousarray(np.asarray(thresholds, np.float64).reshape(-1))
        rk = _ranks(ranks)
        keep = (ptr, mem, th, rk)
        return _lib.IsoformDesc(len(groups), _ptr(ptr), _ptr(mem), th.size, _ptr(th), rk.size, _ptr(rk)), keep

    @classmethod
    def from_sampler(cls, sampler, summary, groups, thresholds=(), ranks=()):
        """Over the chain of `summary` (a finished gibbs.Summary of `sampler`); a member < n is a transcript, n + v the summary's virtual
        transcript v.  The sampler must outlive the handle."""
        d, keep = cls._desc(groups, thresholds, ranks)
        h = C.c_void_p()
        check(_lib.load().mmg_isoform_create(sampler._h, summary._h, C.byref(d), C.byref(h)))
        return cls(h, keep[0], sampler.trace_len, keep[2], keep[3])

    @classmethod
    def from_traces(cls, traces, groups, thresholds=(), ranks=(), device=0):
        """traces: (n_series, S), as Sampler.trace returns a chain; members index its rows."""
        tr = np.ascontiguousarray(traces, np.float64)
        if tr.ndim != 2:
            raise ValueError("traces must be (n_series, S)")
        d, keep = cls._desc(groups, thresholds, ranks)
        h = C.c_void_p()
        check(_lib.load().mmg_isoform_of_traces(int(device), tr.shape[1], tr.shape[0], _ptr(tr), C.byref(d), C.byref(h)))
        return cls(h, keep[0], tr.shape[1], keep[2], keep[3])

    def members(self):
        """n_top, n_second (n_members,), n_above (n_members, n_thresholds) in the flat order of the groups' lists, and the shares
        p_top, p_second, p_above = count / S"""
        m = self.n_members
        out = dict(n_top=np.empty(m, np.uint32), n_second=np.empty(m, np.uint32), n_above=np.empty((m, self.thresholds.size), np.uint32))
        check(self._lib.mmg_isoform_get_members(self._h, _ptr(out["n_top"]), _ptr(out["n_second"]), _ptr(out["n_above"])))
        s = np.float64(self.S)
        out.update(p_top=out["n_top"] / s, p_second=out["n_second"] / s, p_above=out["n_above"] / s)
        return out

    def groups(self):
        """The device columns per group (q_H, q_P: (n_groups, n_ranks)) and, derived with IEEE arithmetic: sd_H, sd_P =
        sqrt(ss / (S - 1)), eff_isoforms = exp(mean_H), and the major member's p_top, p_second and p_above (n_groups, n_thresholds);
        NaN for a group whose status is not 0"""
        g = self.n_groups
        out = dict(status=np.empty(g, np.uint8), major=np.empty(g, np.uint32), n_distinct=np.empty(g, np.uint32), mean_H=np.empty(g),
                   ss_H=np.empty(g), mean_P=np.empty(g), ss_P=np.empty(g), q_H=np.empty((g, self.ranks.size)), q_P=np.empty((g, self.ranks.size)))
        check(self._lib.mmg_isoform_get_groups(self._h, *[_ptr(out[k]) for k in ("status", "major", "n_distinct", "mean_H", "ss_H", "mean_P", "ss_P",
                                                                                  "q_H", "q_P")]))
        out.update(derived(out, self.members(), self.ptr, self.S))
        return out

    def rows(self, first=0, count=None):
        """top, second (uint32), H, P of the groups [first, first + count), each (count, S): computed again on the device"""
        count = self.n_groups - first if count is None else count
        out = dict(top=np.empty((count, self.S), np.uint32), second=np.empty((count, self.S), np.uint32), H=np.empty((count, self.S)),
                   P=np.empty((count, self.S)))
        check(self._lib.mmg_isoform_get_rows(self._h, int(first), int(count), _ptr(out["top"]), _ptr(out["second"]), _ptr(out["H"]), _ptr(out["P"])))
        return out

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_isoform_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_isoform_destroy(self._h)
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


def derived(grp, mem, ptr, S):
    """What the wrapper and the CLI compute from the device columns"""
    at = np.asarray(ptr[:-1], np.int64) + grp["major"].astype(np.int64)
    bad = grp["status"] != 0
    with np.errstate(all="ignore"):
        d = np.float64(S - 1)
        return dict(sd_H=np.sqrt(grp["ss_H"] / d), sd_P=np.sqrt(grp["ss_P"] / d), eff_isoforms=np.exp(grp["mean_H"]),
                    p_top=np.where(bad, np.nan, mem["p_top"][at]), p_second=np.where(bad, np.nan, mem["p_second"][at]),
                    p_above=np.where(bad[:, None], np.nan, mem["p_above"][at]))


def switch_probability(ptr, n_top_a, S_a, n_top_b, S_b):
    """The same groups (offsets `ptr` into the flat member order) in two samples A and B, which are independent given their reads:
    per group the probability that their major isoforms differ, 1 - sum_j nA_top[j] nB_top[j] / (S_A S_B), exactly, over all pairs
    of draws.  Host arithmetic on the counts of Isoforms.members(); NaN for a group whose counts do not sum to S on either side
    (a group that is not valid)."""
    ptr = np.asarray(ptr, np.int64)
    a = np.asarray(n_top_a, np.int64)
    b = np.asarray(n_top_b, np.int64)
    if a.shape != b.shape or a.ndim != 1 or ptr.ndim != 1 or ptr.size < 1 or ptr[-1] != a.size:
        raise ValueError("n_top_a and n_top_b must have one entry per list entry of ptr")
    if S_a < 1 or S_b < 1:
        raise ValueError("S_a and S_b must be at least 1")
    out = np.empty(ptr.size - 1)
    for g in range(ptr.size - 1):
        ga, gb = a[ptr[g]:ptr[g + 1]], b[ptr[g]:ptr[g + 1]]
        if int(ga.sum()) != int(S_a) or int(gb.sum()) != int(S_b):
            out[g] = np.nan
            continue
        same = int((ga * gb).sum())                       # exact: Python integers past 2^53 are not reached (S <= 4096)
        out[g] = (int(S_a) * int(S_b) - same) / float(int(S_a) * int(S_b))
    return out
