"""Posterior log-ratios between sets of transcripts of one sample (thin mirror of the mmg_contrast_* entries of include/mmgibbs.h).

A contrast is a pair of member lists (numerator, denominator); per kept sample r = log(sum of the numerator's traces) - log(sum of the
denominator's), and per contrast the mean of r, Sokal's variance and autocorrelation time of r, order statistics of r and the share
of samples in which the numerator is the larger.  `Contrast.from_sampler` reads the chain a finished Summary was taken over, on the
device; `Contrast.from_traces` takes series-major host traces.  The specification is restated in tests/contrast_ref.py.  No CPU
path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(g) for g in lists])
    mem = np.array([m for g in lists for m in g], np.uint32)
    return ptr, mem


class Contrast:
    def __init__(self, handle, n_contrasts, n_samples, n_percentiles):
        self._lib = _lib.load()
        self._h = handle
        self.n_contrasts, self.S, self.n_percentiles = int(n_contrasts), int(n_samples), int(n_percentiles)

    @staticmethod
    def _desc(contrasts, percentile_index):
        """contrasts: (numerator members, denominator members) pairs; the arrays are returned too (the description points into them)"""
        nptr, nmem = _csr([c[0] for c in contrasts])
        dptr, dmem = _csr([c[1] for c in contrasts])
        pidx = np.ascontiguousarray(percentile_index, np.int32)
        keep = (nptr, nmem, dptr, dmem, pidx)
        return _lib.ContrastDesc(len(contrasts), _ptr(nptr), _ptr(nmem), _ptr(dptr), _ptr(dmem), pidx.size, _ptr(pidx)), keep

    @classmethod
    def from_sampler(cls, sampler, summary, contrasts, percentile_index=()):
        """Over the chain of `summary` (a finished gibbs.Summary of `sampler`); a member < n is a transcript, n + v the summary's virtual
        transcript v.  The sampler must outlive the handle."""
        d, keep = cls._desc(contrasts, percentile_index)
        h = C.c_void_p()
        check(_lib.load().mmg_contrast_create(sampler._h, summary._h, C.byref(d), C.byref(h)))
        return cls(h, len(contrasts), sampler.trace_len, keep[4].size)

    @classmethod
    def from_traces(cls, traces, contrasts, percentile_index=(), device=0):
        """traces: (n_series, S), as Sampler.trace returns a chain; members index its rows."""
        tr = np.ascontiguousarray(traces, np.float64)
        if tr.ndim != 2:
            raise ValueError("traces must be (n_series, S)")
        d, keep = cls._desc(contrasts, percentile_index)
        h = C.c_void_p()
        check(_lib.load().mmg_contrast_of_traces(int(device), tr.shape[1], tr.shape[0], _ptr(tr), C.byref(d), C.byref(h)))
        return cls(h, len(contrasts), tr.shape[1], keep[4].size)

    def summary(self):
        """log_ratio, var, tau, rc, p_gt per contrast and percentiles (n_contrasts, n_percentiles)"""
        c = self.n_contrasts
        lr, var, tau, pgt = np.empty(c), np.empty(c), np.empty(c), np.empty(c)
        rc = np.empty(c, np.int32)
        pct = np.empty((c, self.n_percentiles))
        check(self._lib.mmg_contrast_get(self._h, _ptr(lr), _ptr(var), _ptr(tau), _ptr(rc), _ptr(pgt), _ptr(pct)))
        return dict(log_ratio=lr, var=var, tau=tau, rc=rc, p_gt=pgt, percentiles=pct)

    def rows(self, first=0, count=None):
        """r of the contrasts [first, first + count), shape (count, S): computed again on the device"""
        count = self.n_contrasts - first if count is None else count
        out = np.empty((count, self.S))
        check(self._lib.mmg_contrast_get_rows(self._h, int(first), int(count), _ptr(out)))
        return out

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_contrast_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_contrast_destroy(self._h)
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
