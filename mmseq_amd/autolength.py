"""Run length chosen by the data: a sampler is run to its planned end, judged by the convergence diagnostics across its chains, and
extended to twice the length (Sampler.extend: bit for bit the run that was planned that long) until the stopping rule holds or the
next doubling would pass max_iter.  The rule is the one of mmseq -gibbs_auto (csrc/host/auto_rule.hpp)."""
import math

import numpy as np

from .gibbs import SERIES_TRANSCRIPT, Convergence


def judge(rhat, ess_bulk, ess_tail, ess=400.0, rhat_bound=1.01, frac=0.99):
    """judged: transcripts whose three numbers are all non-NaN; passes: fmin(ess_bulk, ess_tail) >= ess and rhat <= rhat_bound;
    stop: passes >= ceil(frac * judged) in double, or nothing judged."""
    rhat, eb, et = (np.asarray(a, np.float64) for a in (rhat, ess_bulk, ess_tail))
    ok = ~(np.isnan(rhat) | np.isnan(eb) | np.isnan(et))
    e = np.fmin(eb[ok], et[ok])
    r = rhat[ok]
    judged = int(ok.sum())
    passes = int(((e >= ess) & (r <= rhat_bound)).sum())
    needed = int(math.ceil(frac * float(judged)))
    return dict(judged=judged, passes=passes, needed=needed, min_ess=float(e.min()) if judged else float("nan"),
                max_rhat=float(r.max()) if judged else float("nan"), stop=judged == 0 or passes >= needed)


def run_auto(sampler, max_iter, ess=400.0, rhat=1.01, frac=0.99):
    """Returns the stages: dicts of gibbs_iter, gibbs_ss, judged, passes, min_ess (the least fmin(ess_bulk, ess_tail)), max_rhat and
    decision -- 'extend', 'stop' (the rule holds) or 'max' (it does not, and twice the length would pass max_iter) -- and the per-transcript rhat, ess_bulk, ess_tail the decision was taken from."""
    if not (ess > 0.0 and rhat > 1.0 and 0.0 < frac <= 1.0):
        raise ValueError("ess > 0, rhat > 1 and 0 < frac <= 1")
    if max_iter < sampler.gibbs_iter:
        raise ValueError("max_iter is below the sampler's planned length")
    stages = []
    while True:
        sampler.run(sampler.gibbs_iter - sampler.iteration)
        conv = Convergence(sampler)
        try:
            d = conv.series(SERIES_TRANSCRIPT)
        finally:
            conv.close()
        v = judge(d["rhat"], d["ess_bulk"], d["ess_tail"], ess, rhat, frac)
        decision = "stop" if v["stop"] else ("extend" if 2 * sampler.gibbs_iter <= max_iter else "max")
        stages.append(dict(gibbs_iter=sampler.gibbs_iter, gibbs_ss=sampler.gibbs_iter // sampler.trace_len, judged=v["judged"], passes=v["passes"],
                           min_ess=v["min_ess"], max_rhat=v["max_rhat"], decision=decision, rhat=d["rhat"], ess_bulk=d["ess_bulk"],
                           ess_tail=d["ess_tail"]))
        if decision != "extend":
            return stages
        sampler.extend()
