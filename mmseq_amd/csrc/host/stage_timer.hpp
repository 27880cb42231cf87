// Stage timings on stderr when MMSEQ_TIMING is set (not part of the reference's output): shared by mmseq and mmcollapse
#pragma once
#include <omp.h>

#include <cstdio>
#include <cstdlib>

struct StageTimer {
    bool on = getenv("MMSEQ_TIMING") != nullptr;
    double t0 = omp_get_wtime(), last = t0;
    void mark(const char *what)
    {
        if (!on) return;
        const double now = omp_get_wtime();
        fprintf(stderr, "[timing] %-28s %8.3f s\n", what, now - last);
        last = now;
    }
    void total() { if (on) fprintf(stderr, "[timing] %-28s %8.3f s\n", "total", omp_get_wtime() - t0); }
};
