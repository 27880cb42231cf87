// lrt_stats_test.cpp -- host/lrt_stats.hpp on a file (tests/test_lrt_stats.py compares with scipy and a plain-loop BH).
//   lrt_stats_test p FILE    lines "df stat"  -> one p-value per line (%.17g)
//   lrt_stats_test q FILE    one p per line ("nan" allowed) -> one q-value per line (%.17g)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lrt_stats.hpp"

int main(int argc, char **argv)
{
    if (argc != 3 || (std::strcmp(argv[1], "p") && std::strcmp(argv[1], "q"))) {
        std::fprintf(stderr, "usage: lrt_stats_test p|q FILE\n");
        return 2;
    }
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    if (argv[1][0] == 'p') {
        int df;
        double stat;
        while (std::fscanf(f, "%d %lf", &df, &stat) == 2) std::printf("%.17g\n", lrt::chi2_sf((int32_t)df, stat));
    } else {
        std::vector<double> p;
        double v;
        while (std::fscanf(f, "%lf", &v) == 1) p.push_back(v);
        std::vector<double> q(p.size());
        lrt::bh_qvalues(p.size(), p.data(), q.data());
        for (double x : q) std::printf("%.17g\n", x);
    }
    std::fclose(f);
    return 0;
}
