"""The stopping rule of mmseq -gibbs_auto (mmseq_amd/csrc/host/auto_rule.hpp) restated in Python, for the tests.

judged = transcripts whose rhat, ess_bulk and ess_tail are all non-NaN; a judged transcript passes when fmin(ess_bulk, ess_tail) >= E
and rhat <= R; stop when passes >= ceil(f * judged) (product and ceiling in double) or when nothing is judged."""
import math


def judge(rhat, ess_bulk, ess_tail, ess=400.0, rhat_bound=1.01, frac=0.99):
    judged = passes = 0
    min_ess = max_rhat = float("nan")
    for r, eb, et in zip(rhat, ess_bulk, ess_tail):
        r, eb, et = float(r), float(eb), float(et)
        if r != r or eb != eb or et != et:
            continue
        e = min(eb, et)
        min_ess = e if judged == 0 else min(min_ess, e)
        max_rhat = r if judged == 0 else max(max_rhat, r)
        judged += 1
        if e >= ess and r <= rhat_bound:
            passes += 1
    needed = int(math.ceil(frac * float(judged)))
    return dict(judged=judged, passes=passes, needed=needed, min_ess=min_ess, max_rhat=max_rhat, stop=judged == 0 or passes >= needed)
