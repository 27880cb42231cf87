"""Host-side view of mmdiff's device sampler (thin mirror of the mmg_diff_* entries of include/mmgibbs.h).

`Diff` holds every feature's MCMC state on the device (src/bms.cpp driven as src/mmdiff.cpp:744-866): `burnin` runs the burn-in and
sets the pseudopriors, `tune_batch` one tuning batch of 128 iterations, `sample` the sampling iterations, `results` the posterior
means.  `DiffPoly` runs several alternatives against one model 0 on one handle, `DiffChains` several chains of one comparison, `DiffPerm` the data and
its shuffled copies with q-values (`qvalues` computes them for any two arrays of statistics), `DiffLrt` fits both models by maximum
likelihood and gives the likelihood-ratio test of every feature.  No CPU path exists: without a device every call raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

MAXBATCHES = 8192
TRACE_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_double))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _design(obj, y, e, M, P0, P1, classes):
    """The arguments every two-model class takes, as the contiguous arrays of the create entries: (y, e, M, [P0, P1], classes) with
    y, e (F, N), M (N, K), P0 (N, L0), P1 (N, L1), classes (N, 2); sets obj.F, N, K and L = (L0, L1)."""
    y = np.ascontiguousarray(y, np.float64)
    e = np.ascontiguousarray(e, np.float64)
    M = np.ascontiguousarray(M, np.float64)
    P = [np.ascontiguousarray(P0, np.float64), np.ascontiguousarray(P1, np.float64)]
    Cl = np.ascontiguousarray(classes, np.int32)
    F, N = y.shape
    if e.shape != (F, N) or M.shape[0] != N or P[0].shape[0] != N or P[1].shape[0] != N or Cl.shape != (N, 2):
        raise ValueError("inconsistent shapes")
    obj.F, obj.N, obj.K = F, N, M.shape[1]
    obj.L = (P[0].shape[1], P[1].shape[1])
    return y, e, M, P, Cl


class Diff:
    def __init__(self, y, e, M, P0, P1, classes, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, device=0):
        """y, e: (F, N) estimates and standard deviations; M (N, K), P0 (N, L0), P1 (N, L1); classes (N, 2) the variance class of each
        sample under models 0 and 1."""
        self._lib = _lib.load()
        self._h = None
        y, e, M, P, Cl = _design(self, y, e, M, P0, P1, classes)
        h = C.c_void_p()
        check(self._lib.mmg_diff_create(device, self.F, self.N, _ptr(y), _ptr(e), self.K, _ptr(M), self.L[0], _ptr(P[0]), self.L[1], _ptr(P[1]),
                                        _ptr(Cl), float(d), float(s), float(pdash), int(bool(fixalpha)), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        C.byref(h)))
        self._h = h

    def burnin(self, iters):
        self._run(self._lib.mmg_diff_burnin(self._h, int(iters)))

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
        self._run(self._lib.mmg_diff_sample(self._h, int(iters)))

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

    def trace_names(self):
        """The traced parameters as the reference's trace files are named, in row order; `gamma`, the last, is in sampling rows only."""
        n = C.c_uint32()
        check(self._lib.mmg_diff_trace_layout(self._h, C.byref(n), None))
        buf = C.create_string_buffer(32)
        names = []
        for i in range(n.value):
            check(self._lib.mmg_diff_trace_name(self._h, i, buf, 32))
            names.append(buf.value.decode())
        return names

    def open_traces(self, every_burnin, every_sample, sink=None):
        """Before `burnin`: record every every_burnin-th burn-in and every every_sample-th sampling iteration.  sink(phase, first_row,
        rows) gets the rows of one launch as an array (n, P, F) that is valid during the call (phase 0 burn-in, P without gamma; 1
        sampling) and returns 0, or non-zero to stop the run.  Without a sink the rows are kept: `traces`."""
        P, F = len(self.trace_names()), self.F
        rows_kept = ([], [])

        def keep(phase, first, rows):
            rows_kept[phase].append(rows.copy())
            return 0

        fn = sink or keep

        def cb(user, phase, first, n, ptr):
            try:
                rows = np.ctypeslib.as_array(ptr, shape=(n, P if phase else P - 1, F))
                return int(fn(phase, first, rows) or 0)
            except BaseException as ex:     # an exception cannot cross the C frames: stop the run, raise it from the entry that ran
                self._sink_error = ex
                return -1

        cfn = TRACE_SINK(cb)
        check(self._lib.mmg_diff_trace_open(self._h, int(every_burnin), int(every_sample), C.cast(cfn, C.c_void_p), None))
        self._sink = cfn                # (kept alive with the handle)
        self._rows = None if sink else rows_kept

    def traces(self):
        """The rows kept so far: (burn-in (rows, P - 1, F), sampling (rows, P, F)).  Only after `open_traces` without a sink."""
        if getattr(self, "_rows", None) is None:
            raise RuntimeError("no rows are kept: traces() needs open_traces() without a sink")
        P, F = len(self.trace_names()), self.F
        return tuple(np.concatenate(r) if r else np.empty((0, P - 1 + ph, F)) for ph, r in enumerate(self._rows))

    def open_effects(self, every, max_rows):
        """Before `burnin`: keep every every-th sampling iteration's row (max_rows at most, up to 4096) on the device for `effects`.
        Not together with `open_traces`."""
        check(self._lib.mmg_diff_effects_open(self._h, int(every), int(max_rows)))

    def effects(self, percentiles=(2.5, 50.0, 97.5)):
        """The summary of the rows recorded so far: `effects_of_rows` of them with the models of `trace_names()`."""
        pct = np.ascontiguousarray(percentiles, np.float64).ravel()
        e = C.c_void_p()
        check(self._lib.mmg_diff_effects_summarize(self._h, len(pct), _ptr(pct), C.byref(e)))
        names = self.trace_names()[:-1]
        return _effects_out(self._lib, e, names, self.F, pct)

    def _run(self, rc):
        """check(rc); an exception of the caller's sink, which stopped the run, is raised in place of the library's error."""
        ex, self._sink_error = getattr(self, "_sink_error", None), None
        if rc != 0 and ex is not None:
            raise ex
        check(rc)

    def tune_state(self):
        """(mean log odds of the last batch, logit p') per feature, as they stand: what BMS::printtune prints before a batch's tuning."""
        lo, lp = np.empty(self.F), np.empty(self.F)
        check(self._lib.mmg_diff_get_tune_state(self._h, _ptr(lo), _ptr(lp)))
        return lo, lp

    def pseudo(self):
        """The pseudopriors after the burn-in, (columns of BMS::print_pseudo, F)."""
        n = C.c_uint32()
        check(self._lib.mmg_diff_trace_layout(self._h, None, C.byref(n)))
        out = np.empty((n.value, self.F))
        check(self._lib.mmg_diff_get_pseudo(self._h, _ptr(out)))
        return out

    def close(self):
        if self._h:
            self._lib.mmg_diff_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _effects_out(lib, e, names, F, pct):
    """The results of an mmg_effects handle as a dict of arrays, and the handle destroyed."""
    Q, npct = len(names), len(pct)
    out = dict(names=list(names), percentiles=pct.copy(), n=np.empty((2, F), np.uint32), mean=np.empty((Q, F)), sd=np.empty((Q, F)),
               n_gt=np.empty((Q, F), np.uint32), q=np.empty((Q, npct, F)))
    try:
        check(lib.mmg_effects_get(e, *(_ptr(out[k]) for k in ("n", "mean", "sd", "n_gt", "q"))))
        b = C.c_uint64()
        check(lib.mmg_effects_device_bytes(e, C.byref(b)))
        out["device_bytes"] = b.value
    finally:
        lib.mmg_effects_destroy(e)
    return out


def effects_of_rows(rows, model_of, percentiles=(2.5, 50.0, 97.5), names=None, device=0):
    """Effect summaries of rows (S, P, F), gamma (0.0 / 1.0) as parameter P - 1, model_of (P - 1,) the model of each parameter: per
    parameter and feature, over the rows whose own gamma equals the parameter's model, `n` (2, F), `mean`, `sd`, `n_gt` (P - 1, F)
    and `q` (P - 1, len(percentiles), F), the sorted draw at floor(p / 100 * (n - 1) + 0.5).  tests/mmdiff_effects_ref.py restates it."""
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, np.float64)
    if rows.ndim != 3:
        raise ValueError("rows must be (S, P, F)")
    S, P, F = rows.shape
    model_of = np.ascontiguousarray(model_of, np.uint8).ravel()
    if len(model_of) != max(P - 1, 0):
        raise ValueError("model_of must have P - 1 entries")
    pct = np.ascontiguousarray(percentiles, np.float64).ravel()
    e = C.c_void_p()
    check(lib.mmg_effects_of_rows(device, S, P, F, _ptr(rows), _ptr(model_of), len(pct), _ptr(pct), C.byref(e)))
    return _effects_out(lib, e, names if names is not None else ["param%d" % s for s in range(P - 1)], F, pct)


class _DiffReplicas:
    """What `DiffPoly`, `DiffChains` and `DiffPerm` share: a handle of `_n` replicas (comparisons, chains, data sets) driven through
    the mmg_diff_<_prefix>_* entries, which differ in the handle type alone."""

    _prefix = None
    _h = None

    def _fn(self, name):
        return getattr(self._lib, "mmg_diff_%s_%s" % (self._prefix, name))

    def _create(self, n, *args):
        self._n = int(n)
        h = C.c_void_p()
        check(self._fn("create")(*args, C.byref(h)))
        self._h = h

    def burnin(self, iters):
        check(self._fn("burnin")(self._h, int(iters)))

    def tune_batch(self):
        """One tuning batch for the replicas that have not ended; (untuned counts, ended flags), one entry per replica."""
        n, ended = (C.c_uint32 * self._n)(), (C.c_int32 * self._n)()
        check(self._fn("tune_batch")(self._h, n, ended))
        return list(n), [bool(v) for v in ended]

    def tune(self, max_batches=MAXBATCHES):
        """Batches until every replica has ended or max_batches have run; the batch count of each replica."""
        nb = 0
        while nb != max_batches:
            _, ended = self.tune_batch()
            nb += 1
            if all(ended):
                break
        return [self.info(r)["batches"] for r in range(self._n)]

    def sample(self, iters):
        check(self._fn("sample")(self._h, int(iters)))

    def _eta_rows(self, r):
        return self.L[0] + self.L[1]

    def results(self, r):
        F, K = self.F, self.K
        out = dict(gamma_mean=np.empty(F), logitp=np.empty(F), alpha=np.empty((2, F)), beta=np.empty((2, K, F)),
                   eta=np.empty((self._eta_rows(r), F)))
        check(self._fn("get_results")(self._h, int(r), *(_ptr(out[k]) for k in ("gamma_mean", "logitp", "alpha", "beta", "eta"))))
        return out

    def info(self, r):
        flags, nc, nb, ended = (C.c_int32 * 3)(), (C.c_uint32 * 2)(), C.c_uint32(), C.c_int32()
        check(self._fn("info")(self._h, int(r), flags, nc, C.byref(nb), C.byref(ended)))
        return dict(Mnil=bool(flags[0]), Pnil=(bool(flags[1]), bool(flags[2])), n_classes=(nc[0], nc[1]), batches=nb.value,
                    ended=bool(ended.value))

    def device_bytes(self):
        b = C.c_uint64()
        check(self._fn("device_bytes")(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DiffPoly(_DiffReplicas):
    """J alternatives against one model 0 on one handle (the mmg_diff_poly_* entries): y, e, M and P0 are held once and every launch
    covers all comparisons.  Comparison j's chain is bit for bit that of `Diff(y, e, M, P0, P1s[j], [classes0, classes1s[j]])` driven
    the same way; in tuning, a comparison whose untuned count reached 0 has ended and keeps its own batch count."""

    _prefix = "poly"

    def __init__(self, y, e, M, P0, classes0, P1s, classes1s, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, device=0):
        """y, e: (F, N); M (N, K); P0 (N, L0); classes0 (N,) the variance classes under model 0; P1s: J matrices (N, L1_j);
        classes1s: J vectors (N,) of classes under each alternative."""
        self._lib = _lib.load()
        self._h = None
        y = np.ascontiguousarray(y, np.float64)
        e = np.ascontiguousarray(e, np.float64)
        M = np.ascontiguousarray(M, np.float64)
        P0 = np.ascontiguousarray(P0, np.float64)
        C0 = np.ascontiguousarray(classes0, np.int32)
        P1s = [np.ascontiguousarray(P, np.float64) for P in P1s]
        C1 = np.ascontiguousarray(np.stack([np.asarray(c, np.int32) for c in classes1s]), np.int32) if len(classes1s) else np.zeros((0, 0), np.int32)
        F, N = y.shape
        J = len(P1s)
        if J < 1 or C1.shape != (J, N) or e.shape != (F, N) or M.shape[0] != N or P0.shape[0] != N or C0.shape != (N,) \
                or any(P.ndim != 2 or P.shape[0] != N for P in P1s):
            raise ValueError("inconsistent shapes")
        self.F, self.N, self.K, self.J = F, N, M.shape[1], J
        self.L0 = P0.shape[1]
        self.L1 = tuple(P.shape[1] for P in P1s)
        L1 = np.array(self.L1, np.uint32)
        P1 = np.ascontiguousarray(np.concatenate([P.ravel() for P in P1s]))
        self._create(J, device, F, N, _ptr(y), _ptr(e), self.K, _ptr(M), self.L0, _ptr(P0), _ptr(C0), J, _ptr(L1), _ptr(P1), _ptr(C1),
                     float(d), float(s), float(pdash), int(bool(fixalpha)), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def _eta_rows(self, j):
        return self.L0 + self.L1[j]


class DiffChains(_DiffReplicas):
    """C independent chains of one comparison on one handle (the mmg_diff_chains_* entries).  Chain c draws from the streams
    (seed, c, ...) and is bit for bit `Diff(..., seed=seed ^ (c << 32))` driven the same way; each chain tunes on its own and keeps
    its batch count.  `sample_total` (a positive multiple of 16) is the whole sampling length: `sample` may be called in pieces that
    add up to it, and `pool` then forms the pooled estimates."""

    NB = 16

    _prefix = "chains"

    def __init__(self, y, e, M, P0, P1, classes, n_chains, sample_total, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, device=0):
        self._lib = _lib.load()
        self._h = None
        y, e, M, P, Cl = _design(self, y, e, M, P0, P1, classes)
        self.C, self.T = int(n_chains), int(sample_total)
        self._create(self.C, device, self.F, self.N, _ptr(y), _ptr(e), self.K, _ptr(M), self.L[0], _ptr(P[0]), self.L[1], _ptr(P[1]), _ptr(Cl),
                     float(d), float(s), float(pdash), int(bool(fixalpha)), int(seed) & 0xFFFFFFFFFFFFFFFF, self.C, self.T)

    def pool(self):
        check(self._lib.mmg_diff_chains_pool(self._h))

    def batch_sums(self, c):
        out = np.empty((self.NB, self.F))
        check(self._lib.mmg_diff_chains_get_batch_sums(self._h, int(c), _ptr(out)))
        return out

    def pooled(self):
        F, K, L = self.F, self.K, self.L
        out = dict(log_bf=np.empty(F), log_bf_sd=np.empty(F), log_bf_mcse=np.empty(F), chains_mixed=np.empty(F, np.uint32),
                   alpha=np.empty((2, F)), beta=np.empty((2, K, F)), eta=np.empty((L[0] + L[1], F)))
        check(self._lib.mmg_diff_chains_get_pooled(self._h, *(_ptr(out[k]) for k in ("log_bf", "log_bf_sd", "log_bf_mcse", "chains_mixed",
                                                                                      "alpha", "beta", "eta"))))
        return out


class DiffPerm(_DiffReplicas):
    """The data and B shuffled copies of it on one handle (the mmg_diff_perm_* entries): R = n_perm + 1 replicas, 1 <= n_perm <= 31.
    Replica 0 is the data as given; replica b >= 1 is the data with every feature's samples shuffled on the device, the shuffle
    `mmdiff -permute` applies with the seed seed ^ (b << 32).  Replica b is bit for bit `Diff(y_b, e_b, ..., seed=seed ^ (b << 32))`
    driven the same way; each replica tunes on its own and keeps its batch count.  After sampling, `qvalues` gives the log Bayes
    factors of every replica and the q-values of replica 0 against the pooled replicas 1 .. B."""

    _prefix = "perm"

    def __init__(self, y, e, M, P0, P1, classes, n_perm, d=1.4, s=2.0, pdash=0.5, fixalpha=False, seed=1234, device=0):
        self._lib = _lib.load()
        self._h = None
        y, e, M, P, Cl = _design(self, y, e, M, P0, P1, classes)
        self.B = int(n_perm)
        self.R = self.B + 1
        self._create(self.R, device, self.F, self.N, _ptr(y), _ptr(e), self.K, _ptr(M), self.L[0], _ptr(P[0]), self.L[1], _ptr(P[1]), _ptr(Cl),
                     float(d), float(s), float(pdash), int(bool(fixalpha)), int(seed) & 0xFFFFFFFFFFFFFFFF, self.B & 0xFFFFFFFF)

    def qvalues(self):
        """After sampling: `stat` (R, F) the log Bayes factor of every replica and feature, and of replica 0 against the pooled
        replicas 1 .. B `null_ge` (F,) the null statistics not below the feature's own and `q` (F,) the q-values."""
        out = dict(stat=np.empty((self.R, self.F)), null_ge=np.empty(self.F, np.uint64), q=np.empty(self.F))
        check(self._lib.mmg_diff_perm_qvalues(self._h))
        check(self._lib.mmg_diff_perm_get_qvalues(self._h, _ptr(out["stat"]), _ptr(out["null_ge"]), _ptr(out["q"])))
        return out


class DiffLrt:
    """The per-feature likelihood-ratio test of `Diff`'s two models (the mmg_diff_lrt_* entries): both fitted by maximum likelihood,
    without priors, on the device; no sampler and no stream.  The constructor computes everything and the handle keeps the results
    on the host.  tests/mmdiff_lrt_ref.py restates it."""

    def __init__(self, y, e, M, P0, P1, classes, fixalpha=False, max_iters=0, device=0):
        """y, e, M, P0, P1, classes as for `Diff`; max_iters: the cap on scoring iterations per model (0: the default, 200)."""
        self._lib = _lib.load()
        self._h = None
        y, e, M, P, Cl = _design(self, y, e, M, P0, P1, classes)
        h = C.c_void_p()
        check(self._lib.mmg_diff_lrt_create(device, self.F, self.N, _ptr(y), _ptr(e), self.K, _ptr(M), self.L[0], _ptr(P[0]), self.L[1], _ptr(P[1]),
                                            _ptr(Cl), int(bool(fixalpha)), int(max_iters), C.byref(h)))
        self._h = h

    def info(self):
        flags, nc, p = (C.c_int32 * 3)(), (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
        check(self._lib.mmg_diff_lrt_info(self._h, flags, nc, p))
        return dict(Mnil=bool(flags[0]), Pnil=(bool(flags[1]), bool(flags[2])), n_classes=(nc[0], nc[1]), n_cols=(p[0], p[1]))

    def results(self):
        """dict: loglik (2, F), stat, p_value, q_value (F,), df, theta0 (p0, F), theta1 (p1, F) in the column order
        [alpha | beta | eta] of the terms the model has, sigmasq0 (classes0, F), sigmasq1, iters and status (2, F)."""
        F, i = self.F, self.info()
        out = dict(loglik=np.empty((2, F)), stat=np.empty(F), p_value=np.empty(F), q_value=np.empty(F), theta0=np.empty((i["n_cols"][0], F)),
                   theta1=np.empty((i["n_cols"][1], F)), sigmasq0=np.empty((i["n_classes"][0], F)), sigmasq1=np.empty((i["n_classes"][1], F)),
                   iters=np.empty((2, F), np.uint32), status=np.empty((2, F), np.uint32))
        df = C.c_int32()
        check(self._lib.mmg_diff_lrt_get(self._h, _ptr(out["loglik"]), _ptr(out["stat"]), _ptr(out["p_value"]), _ptr(out["q_value"]), C.byref(df),
                                         *(_ptr(out[k]) for k in ("theta0", "theta1", "sigmasq0", "sigmasq1", "iters", "status"))))
        out["df"] = df.value
        out["n_cols"], out["n_classes"] = i["n_cols"], i["n_classes"]
        return out

    def device_bytes(self):
        b = C.c_uint64()
        check(self._lib.mmg_diff_lrt_device_bytes(self._h, C.byref(b)))
        return b.value

    def close(self):
        if self._h:
            self._lib.mmg_diff_lrt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DiffLrtPerm(DiffLrt):
    """`DiffLrt` with a permutation null (the mmg_diff_lrt_perm_* entries): the test on the data and on n_perm copies of it whose
    samples are shuffled per feature as replica b of `DiffPerm` shuffles them, one device lane per (copy, feature).  The constructor
    computes everything and the handle keeps the results on the host.  tests/mmdiff_lrt_perm_ref.py restates it."""

    def __init__(self, y, e, M, P0, P1, classes, n_perm, fixalpha=False, max_iters=0, seed=1234, slab_copies=0, device=0):
        """y, e, M, P0, P1, classes, fixalpha, max_iters as for `DiffLrt`; n_perm: the copies B, 1 to 65535 with B x features at most
        2^31 - 1; seed: the shuffles' key; slab_copies: the copies fitted by one launch (0: as many as keep their data and
        workspace under 1 GiB) -- no result depends on it."""
        self._lib = _lib.load()
        self._h = self._perm = None
        y, e, M, P, Cl = _design(self, y, e, M, P0, P1, classes)
        F, N = self.F, self.N
        if not 0 <= int(n_perm) < 2 ** 32 or not 0 <= int(slab_copies) < 2 ** 32:
            raise ValueError("n_perm and slab_copies must fit 32 bits")
        self.B = int(n_perm)
        h = C.c_void_p()
        check(self._lib.mmg_diff_lrt_perm_create(device, F, N, _ptr(y), _ptr(e), self.K, _ptr(M), self.L[0], _ptr(P[0]), self.L[1], _ptr(P[1]),
                                                 _ptr(Cl), int(bool(fixalpha)), int(max_iters), self.B, int(seed) & (2 ** 64 - 1), int(slab_copies),
                                                 C.byref(h)))
        self._perm = h
        self._h = C.c_void_p(self._lib.mmg_diff_lrt_perm_observed(h))      # borrowed: DiffLrt's info() and results() read it

    def results(self):
        """What `DiffLrt.results()` returns for the data, and null_stat (B, F), null_status (B, F) uint8 = status0 | status1 << 4,
        perm_ge, perm_n (F,) uint64, perm_p, null_ge (uint64) and q_perm (F,)."""
        F, B = self.F, self.B
        out = DiffLrt.results(self)
        out.update(null_stat=np.empty((B, F)), null_status=np.empty((B, F), np.uint8), perm_ge=np.empty(F, np.uint64), perm_n=np.empty(F, np.uint64),
                   perm_p=np.empty(F), null_ge=np.empty(F, np.uint64), q_perm=np.empty(F))
        check(self._lib.mmg_diff_lrt_perm_get_null(self._perm, 0, B, _ptr(out["null_stat"]), _ptr(out["null_status"])))
        check(self._lib.mmg_diff_lrt_perm_get(self._perm, *(_ptr(out[k]) for k in ("perm_ge", "perm_n", "perm_p", "null_ge", "q_perm"))))
        return out

    def device_bytes(self):
        """The peak of the handle's own device memory during creation (the formula of include/mmgibbs.h)."""
        b = C.c_uint64()
        check(self._lib.mmg_diff_lrt_perm_device_bytes(self._perm, C.byref(b)))
        return b.value

    def close(self):
        if self._perm:
            self._lib.mmg_diff_lrt_perm_destroy(self._perm)
        self._perm = self._h = None


def qvalues(obs, null, device=0):
    """q-values of the observed statistics against the null statistics (any shapes, taken flat), on the device: (null_ge, q), per
    observed value the null values not below it and min over the observed t' <= it of min(1, V(t') m / (m0 R(t'))), with R and V the
    observed and null values >= t', m and m0 the observed and null values that are not NaN.  tests/qvalue_ref.py restates it."""
    lib = _lib.load()
    obs = np.ascontiguousarray(obs, np.float64).ravel()
    null = np.ascontiguousarray(null, np.float64).ravel()
    null_ge, q = np.empty(obs.size, np.uint64), np.empty(obs.size)
    check(lib.mmg_qvalues(device, obs.size, _ptr(obs), null.size, _ptr(null), _ptr(null_ge), _ptr(q)))
    return null_ge, q
