"""The posterior correlation of transcripts that share reads (thin mirror of the mmg_pairs_* entries of include/mmgibbs.h).

For ordered pairs (a, b) of transcripts of one sample, from the kept samples of one chain: the means of log x_a, log x_b and
log(x_a + x_b), their centred second moments in two passes and the number of samples with x_a > x_b come from the device;
`summary()` adds cor, sd_a, sd_b, sd_sum and p_gt from them with IEEE sqrt and division.  A strongly negative cor with sd_sum far
below sd_a and sd_b reads "these two are one feature in this sample".  `Pairs.from_sampler` reads a chain of a sampler that is
past its last kept sample, on the device; `Pairs.from_traces` takes series-major host traces.  The specification is restated in
tests/pairs_ref.py.  No CPU path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

DEVICE_COLUMNS = ("mean_a", "mean_b", "mean_sum", "saa", "sbb", "sab", "sss", "n_gt")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _members(pairs):
    """pairs: (a, b) tuples or an (n_pairs, 2) array -> two uint32 arrays"""
    arr = np.asarray(pairs, np.int64).reshape(-1, 2) if len(pairs) else np.zeros((0, 2), np.int64)
    if arr.size and (arr.min() < 0 or arr.max() > 0xffffffff):
        raise ValueError("pair members must fit 32 unsigned bits")
    return np.ascontiguousarray(arr[:, 0], np.uint32), np.ascontiguousarray(arr[:, 1], np.uint32)


class Pairs:
    def __init__(self, handle, n_pairs, n_samples):
        self._lib = _lib.load()
        self._h = handle
        self.n_pairs, self.S = int(n_pairs), int(n_samples)

    @classmethod
    def from_sampler(cls, sampler, pairs, chain=0):
        """Over the trace_len kept samples of `chain` of `sampler`, members in the caller's transcript numbering."""
        a, b = _members(pairs)
        h = C.c_void_p()
        check(_lib.load().mmg_pairs_create(sampler._h, int(chain), a.size, _ptr(a), _ptr(b), C.byref(h)))
        return cls(h, a.size, sampler.trace_len)

    @classmethod
    def from_traces(cls, traces, pairs, device=0):
        """traces: (n_series, S), as Sampler.trace returns a chain; members index its rows."""
        tr = np.ascontiguousarray(traces, np.float64)
        if tr.ndim != 2:
            raise ValueError("traces must be (n_series, S)")
        a, b = _members(pairs)
        h = C.c_void_p()
        check(_lib.load().mmg_pairs_of_traces(int(device), tr.shape[1], tr.shape[0], _ptr(tr), a.size, _ptr(a), _ptr(b), C.byref(h)))
        return cls(h, a.size, tr.shape[1])

    def summary(self):
        """the eight device columns per pair, and cor, sd_a, sd_b, sd_sum, p_gt derived from them"""
        p = self.n_pairs
        out = {k: np.empty(p) for k in DEVICE_COLUMNS[:7]}
        out["n_gt"] = np.empty(p, np.uint32)
        check(self._lib.mmg_pairs_get(self._h, *[_ptr(out[k]) for k in DEVICE_COLUMNS]))
        with np.errstate(all="ignore"):
            d = np.float64(self.S - 1)
            out["cor"] = out["sab"] / (np.sqrt(out["saa"]) * np.sqrt(out["sbb"]))
            out["sd_a"] = np.sqrt(out["saa"] / d)
            out["sd_b"] = np.sqrt(out["sbb"] / d)
            out["sd_sum"] = np.sqrt(out["sss"] / d)
            out["p_gt"] = out["n_gt"].astype(np.float64) / np.float64(self.S)
        return out

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_pairs_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_pairs_destroy(self._h)
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
