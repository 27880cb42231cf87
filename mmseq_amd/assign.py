"""Posterior assignment probability of every hit (thin mirror of the mmg_assign_* entries of include/mmgibbs.h).

`Assign` holds a hit-set matrix in the caller's order on the device.  `run` takes a sampler's trace on the device (transposed there
into the handle's transcript-major copy, never through the host), `run_trace` a transcript-major host trace; `probabilities` returns,
per hit, the mean over the samples of mu[t] / (the sum of mu over the hits of the row), and `expected_hits` the posterior mean of the reads per transcript that follows from them.  The specification is restated in
tests/assign_ref.py.  No CPU path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Assign:
    def __init__(self, row_ptr, col_idx, n_tx, device=0):
        """row_ptr (n_rows + 1), col_idx: the rows in the caller's order and transcript numbering (columns below n_tx)."""
        self._lib = _lib.load()
        self._h = None
        self._rp = np.ascontiguousarray(row_ptr, np.uint64)
        self._ci = np.ascontiguousarray(col_idx, np.uint32)
        if self._rp.ndim != 1 or self._rp.size < 1 or self._ci.ndim != 1:
            raise ValueError("row_ptr needs n_rows + 1 entries")
        if int(self._rp[-1]) != self._ci.size:
            raise ValueError("row_ptr[-1] must be the number of hits")
        self.n_rows, self.n_hits, self.n_tx = self._rp.size - 1, self._ci.size, int(n_tx)
        h = C.c_void_p()
        check(self._lib.mmg_assign_create(int(device), self.n_rows, self.n_tx, _ptr(self._rp), _ptr(self._ci), C.byref(h)))
        self._h = h

    def run(self, sampler, chain=0, first=0, count=None):
        """Over the samples [first, first + count) of a chain of `sampler` (keep_trace; default: every sample of its trace)."""
        if count is None:
            count = sampler.trace_len - first
        check(self._lib.mmg_assign_run_sampler(self._h, sampler._h, int(chain), int(first), int(count)))

    def run_trace(self, trace, first=0, count=None):
        """Over the samples [first, first + count) of a host trace (n_tx, trace_len), as Sampler.trace returns it."""
        tr = np.ascontiguousarray(trace, np.float64)
        if tr.ndim != 2 or tr.shape[0] != self.n_tx:
            raise ValueError("trace must be (n_tx, trace_len)")
        if count is None:
            count = tr.shape[1] - first
        check(self._lib.mmg_assign_run_host(self._h, _ptr(tr), tr.shape[1], int(first), int(count)))

    def probabilities(self):
        """P per hit, in the order of col_idx."""
        out = np.empty(self.n_hits, np.float64)
        check(self._lib.mmg_assign_get(self._h, 0, self.n_hits, _ptr(out)))
        return out

    def expected_hits(self, k=None):
        """Per transcript the sum of k_i P over its hits, in ascending hit index (k: the rows' multiplicities, default ones)."""
        P = self.probabilities()
        L = np.diff(self._rp.astype(np.int64))
        kk = np.ones(self.n_rows) if k is None else np.asarray(k, np.float64)
        if kk.shape != (self.n_rows,):
            raise ValueError("k needs one entry per row")
        out = np.zeros(self.n_tx)
        np.add.at(out, self._ci.astype(np.int64), np.repeat(kk, L) * P)
        return out

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_assign_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_assign_destroy(self._h)
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
