"""Host-side view of mmcollapse's device stages (thin mirror of the mmg_collapse_* entries of include/mmgibbs.h).

`Collapse` holds the centred candidate traces of every sample and the matrix V of mean correlations on the device
(src/mmcollapse.cpp:483-561), gives V's rows and the row maxima of the threshold (:713-747), and runs the greedy loop (:758-819).
`summarize` is the output stage (:827-1107) on host traces.  No CPU path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Collapse:
    def __init__(self, traces, observed, device=0):
        """traces: S arrays of shape (trace_len, C), raw (not logged) posterior traces of the candidates, one per sample;
        observed: (C, S) booleans, the mask of samples in which a candidate was observed."""
        self._lib = _lib.load()
        self._h = None
        S = len(traces)
        observed = np.ascontiguousarray(observed, np.uint8)
        Cn = observed.shape[0]
        if observed.shape != (Cn, S):
            raise ValueError("observed must have shape (C, S)")
        N = np.asarray(traces[0]).shape[0] if S else 0
        h = C.c_void_p()
        check(self._lib.mmg_collapse_create(device, S, Cn, N, _ptr(observed), C.byref(h)))
        self._h = h
        self.n_cand, self.n_samples, self.trace_len = Cn, S, N
        for s, t in enumerate(traces):
            t = np.ascontiguousarray(t, np.float64)
            if t.shape != (N, Cn):
                raise ValueError("every trace must have shape (trace_len, C)")
            check(self._lib.mmg_collapse_set_sample(h, s, _ptr(t)))
        check(self._lib.mmg_collapse_correlate(h))

    def rows(self, first=0, count=None):
        count = self.n_cand - first if count is None else count
        out = np.empty((count, self.n_cand), np.float64)
        check(self._lib.mmg_collapse_get_rows(self._h, first, count, _ptr(out)))
        return out

    def row_max(self):
        out = np.empty(self.n_cand, np.float64)
        check(self._lib.mmg_collapse_row_max(self._h, _ptr(out)))
        return out

    def threshold(self, thres=0.975):
        """-sorted_rowmax[floor(C thres)], the index clamped to C - 1 (:745)."""
        m = np.sort(self.row_max())
        return -m[min(int(np.floor(self.n_cand * thres)), self.n_cand - 1)]

    def run(self, thr, max_merges=1 << 20):
        """The greedy loop until min V >= thr (or max_merges merges): (pairs (m, 2) uint32 with a < b, values (m,), stopped)."""
        pairs = np.empty((max_merges, 2), np.uint32)
        vals = np.empty(max_merges, np.float64)
        n = C.c_uint32(0)
        stopped = C.c_int32(0)
        check(self._lib.mmg_collapse_run(self._h, thr, max_merges, _ptr(pairs), _ptr(vals), C.byref(n), C.byref(stopped)))
        return pairs[:n.value].copy(), vals[:n.value].copy(), bool(stopped.value)

    def device_bytes(self):
        b = C.c_uint64(0)
        check(self._lib.mmg_collapse_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h is not None:
            self._lib.mmg_collapse_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def summarize(trace, groups, virtual_id=None, virtual_scale=None, alpha=0.1, seed=13837, stream=0, device=0):
    """trace: (trace_len, n_cols) raw traces; groups: list of member lists (member < n_cols a column, n_cols + v virtual trace v).
    Returns (log_mean, var, tau, sokal_rc) per group."""
    lib = _lib.load()
    trace = np.ascontiguousarray(trace, np.float64)
    N, n = trace.shape
    vid = np.ascontiguousarray([] if virtual_id is None else virtual_id, np.uint64)
    vsc = np.ascontiguousarray([] if virtual_scale is None else virtual_scale, np.float64)
    ptr = np.zeros(len(groups) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(g) for g in groups])
    mem = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint32) for g in groups]) if groups else np.zeros(0), np.uint32)
    g = len(groups)
    lm, var, tau = (np.empty(g, np.float64) for _ in range(3))
    rc = np.empty(g, np.int32)
    check(lib.mmg_collapse_summarize(device, N, n, _ptr(trace), vid.size, _ptr(vid), _ptr(vsc), alpha, seed, stream, g, _ptr(ptr), _ptr(mem),
                                     _ptr(lm), _ptr(var), _ptr(tau), _ptr(rc)))
    return lm, var, tau, rc
