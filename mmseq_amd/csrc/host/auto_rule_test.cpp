// auto_rule_test.cpp -- host/auto_rule.hpp on a file (tests/test_autolength_rule.py compares with tests/autolength_ref.py).
//   auto_rule_test E R F FILE    lines "rhat ess_bulk ess_tail" ("nan" allowed)
//   -> one line "judged passes needed min_ess max_rhat stop" (%.17g for the two doubles, stop 0 | 1)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "auto_rule.hpp"

int main(int argc, char **argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: auto_rule_test ESS RHAT FRAC FILE\n");
        return 2;
    }
    autolen::Targets t;
    t.ess = std::strtod(argv[1], nullptr);
    t.rhat = std::strtod(argv[2], nullptr);
    t.frac = std::strtod(argv[3], nullptr);
    if (!autolen::targets_valid(t)) { std::fprintf(stderr, "targets: ESS > 0, RHAT > 1, 0 < FRAC <= 1\n"); return 2; }
    FILE *f = std::fopen(argv[4], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[4]); return 1; }
    std::vector<double> r, eb, et;
    double a, b, c;
    while (std::fscanf(f, "%lf %lf %lf", &a, &b, &c) == 3) { r.push_back(a); eb.push_back(b); et.push_back(c); }
    std::fclose(f);
    const autolen::Verdict v = autolen::judge(r.size(), r.data(), eb.data(), et.data(), t);
    std::printf("%llu %llu %llu %.17g %.17g %d\n", (unsigned long long)v.judged, (unsigned long long)v.passes, (unsigned long long)v.needed, v.min_ess,
                v.max_rhat, v.stop ? 1 : 0);
    return 0;
}
