"""Host-side view of mmdiff's device sampler (thin mirror of the mmg_diff_* entries of include/mmgibbs.h).

`Diff` holds every feature's MCMC state on the device (src/bms.cpp driven as src/mmdiff.cpp:744-866): `burnin` runs the burn-in and
sets the pseudopriors, `tune_batch` one tuning batch of 128 iterations, `sample` the sampling iterations, `results` the posterior
means.  No CPU path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

MAXBATCHES = 8192


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Diff:
    def __init__(self, y, e, M, P0, P1, classes, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, device=0):
        """y, e: (F, N) estimates and standard deviations; M (N, K), P0 (N, L0), P1 (N, L1); classes (N, 2) the variance class of each
        sample under models 0 and 1."""
        self._lib = _lib.load()
        self._h = None
        self._y = np.ascontiguousarray(y, np.float64)
        self._e = np.ascontiguousarray(e, np.float64)
        self._M = np.ascontiguousarray(M, np.float64)
        self._P = [np.ascontiguousarray(P0, np.float64), np.ascontiguousarray(P1, np.float64)]
        self._C = np.ascontiguousarray(classes, np.int32)
        F, N = self._y.shape
        if self._e.shape != (F, N) or self._M.shape[0] != N or self._P[0].shape[0] != N or self._P[1].shape[0] != N or self._C.shape != (N, 2):
            raise ValueError("inconsistent shapes")
        self.F, self.N, self.K = F, N, self._M.shape[1]
        self.L = (self._P[0].shape[1], self._P[1].shape[1])
        h = C.c_void_p()
        check(self._lib.mmg_diff_create(device, F, N, _ptr(self._y), _ptr(self._e), self.K, _ptr(self._M), self.L[0], _ptr(self._P[0]),
                                        self.L[1], _ptr(self._P[1]), _ptr(self._C), float(d), float(s), float(pdash), int(bool(fixalpha)),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        self._h = h

    def burnin(self, iters):
        check(self._lib.mmg_diff_burnin(self._h, int(iters)))

    def tune_batch(self):
        """One tuning batch; the number of features still untuned."""
        n = C.c_uint32()
        check(self._lib.mmg_diff_tune_batch(self._h, C.byref(n)))
        return n.value

    def tune(self, max_batches=MAXBATCHES):
        """Batches until every feature is tuned or max_batches have run (src/mmdiff.cpp:765-766); the number of batches."""
        untuned, nb = self.tune_batch(), 1
        while untuned > 0 and nb != max_batches:
            untuned, nb = self.tune_batch(), nb + 1
        return nb

    def sample(self, iters):
        check(self._lib.mmg_diff_sample(self._h, int(iters)))

    def results(self):
        F, K, L = self.F, self.K, self.L
        out = dict(gamma_mean=np.empty(F), logitp=np.empty(F), alpha=np.empty((2, F)), beta=np.empty((2, K, F)), eta=np.empty((L[0] + L[1], F)))
        check(self._lib.mmg_diff_get_results(self._h, *(_ptr(out[k]) for k in ("gamma_mean", "logitp", "alpha", "beta", "eta"))))
        return out

    def info(self):
        flags, nc, nb = (C.c_int32 * 3)(), (C.c_uint32 * 2)(), C.c_uint32()
        check(self._lib.mmg_diff_info(self._h, flags, nc, C.byref(nb)))
        return dict(Mnil=bool(flags[0]), Pnil=(bool(flags[1]), bool(flags[2])), n_classes=(nc[0], nc[1]), batches=nb.value)

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_diff_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_diff_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
