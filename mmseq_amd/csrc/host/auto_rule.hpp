// auto_rule.hpp -- the stopping rule of mmseq -gibbs_auto, plain host code.
// From the transcripts' rank-normalised split R-hat and bulk / tail ESS over all chains (mmg_convergence_*):
//   judged  = transcripts whose three numbers are all non-NaN
//   passes  = judged transcripts with fmin(ess_bulk, ess_tail) >= E and rhat <= R
//   stop    = passes >= ceil(f * judged), product and ceiling in double; also when nothing is judged
// tests/autolength_ref.py restates it; host/auto_rule_test.cpp runs it on a file.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace autolen {

struct Targets {
    double ess = 400.0;   // E > 0
    double rhat = 1.01;   // R > 1
    double frac = 0.99;   // f in (0, 1]
};

inline bool targets_valid(const Targets &t) { return t.ess > 0.0 && t.rhat > 1.0 && t.frac > 0.0 && t.frac <= 1.0; } // (NaN: false)

struct Verdict {
    uint64_t judged = 0, passes = 0, needed = 0;   // needed = ceil(f * judged)
    double min_ess = NAN, max_rhat = NAN;          // over the judged transcripts; NaN when nothing is judged
    bool stop = true;
};

inline Verdict judge(size_t n, const double *rhat, const double *ess_bulk, const double *ess_tail, const Targets &t)
{
    Verdict v;
    for (size_t i = 0; i < n; ++i) {
        if (std::isnan(rhat[i]) || std::isnan(ess_bulk[i]) || std::isnan(ess_tail[i])) continue;
        const double e = std::fmin(ess_bulk[i], ess_tail[i]);
        if (v.judged == 0) { v.min_ess = e; v.max_rhat = rhat[i]; }
        else { v.min_ess = std::fmin(v.min_ess, e); v.max_rhat = std::fmax(v.max_rhat, rhat[i]); }
        ++v.judged;
        if (e >= t.ess && rhat[i] <= t.rhat) ++v.passes;
    }
    v.needed = (uint64_t)std::ceil(t.frac * (double)v.judged);
    v.stop = v.judged == 0 || v.passes >= v.needed;
    return v;
}

} // namespace autolen
