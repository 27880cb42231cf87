// cpu_quota.hpp -- the CPUs this process may actually use, shared by the host tools.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// A container's CFS quota (cgroup v2 cpu.max, v1 cpu.cfs_quota_us) in whole CPUs, rounded up; 0 without a quota.  It is invisible to
// OpenMP and to std::thread::hardware_concurrency(), which count the cores of the host: a pool sized by them is throttled to the quota's
// worth of time.
inline int cpu_quota()
{
    long long quota = -1, period = 100000;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64];
        if (std::fscanf(f, "%63s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
        std::fclose(f);
    } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        if (std::fscanf(g, "%lld", &quota) != 1) quota = -1;
        std::fclose(g);
        if (FILE *h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(h, "%lld", &period) != 1) period = 100000; std::fclose(h); }
    }
    if (quota <= 0 || period <= 0) return 0;
    return (int)std::max<long long>(1, (quota + period - 1) / period);
}
