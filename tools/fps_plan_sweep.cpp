// fps_plan_sweep.cpp — fps_plan() (sph3d_gcn_amd/csrc/fps_plan.hpp) over the grid of tests/test_fps_forms.py and the ends of the int
// range in every argument, as a host program of its own: built with the sanitizers it shows that the plan's arithmetic has no
// undefined behaviour there.  Prints the number of plans, how many chose each kernel, and a checksum of their fields.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fps_plan_sweep.cpp -o /tmp/fps_plan_sweep
//   /tmp/fps_plan_sweep
#include <initializer_list>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "../sph3d_gcn_amd/csrc/fps_plan.hpp"

using namespace sph3d;

static unsigned long long sum = 1469598103934665603ull, count = 0, kernels[5] = {}, bad[4] = {};

static int fail(int b, int n, int m, const char* what)
{
    printf("fps_plan(%d, %d, %d): %s\n", b, n, m, what);
    return 1;
}

static int one(int b, int n, int m)
{
    const FpsPlan p = fps_plan(b, n, m);
    long long f[sizeof(FpsPlan) / sizeof(long long)] = {};
    memcpy(f, &p, offsetof(FpsPlan, bad));
    for (long long v : f) sum = (sum ^ (unsigned long long)v) * 1099511628211ull;
    sum = (sum ^ (unsigned long long)p.bad) * 1099511628211ull;
    count++;
    bad[p.bad]++;
    if (p.bad) {
        for (long long v : f)
            if (v != 0) return fail(b, n, m, "a rejected call with a field set");
        return 0;
    }
    kernels[p.kernel]++;
    // what the launcher relies on: counts that fit a launch, offsets inside the workspace
    if (p.kernel != kFpsNone && !(p.grid >= 1 && p.grid <= 0x7fffffff && p.block >= 64 && p.block <= 1024 && p.block % 64 == 0))
        return fail(b, n, m, "launch dimensions");
    if (p.big_grid < 0 || p.big_grid > kFpsBigGrid || p.off_err != 0 || p.off_slots > p.off_temp || p.off_temp > p.workspace_bytes)
        return fail(b, n, m, "workspace layout");
    if (p.kernel == kFpsCoop && !(p.off_slots + 16 * (long long)b * p.G <= p.off_temp && p.grid >= (long long)b * p.G && (long long)b * p.G <= kFpsCoopMaxBlocks))
        return fail(b, n, m, "co-operative launch");
    if ((p.kernel == kFpsCoop || p.kernel == kFpsBig) && p.off_temp + 4 * p.big_grid * (long long)n != p.workspace_bytes)
        return fail(b, n, m, "running distances");
    return 0;
}

int main()
{
    const int Ns[] = {1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385, 24576, 24577,
                      28672, 28673, 65536, 131072, 262144, 262145};
    const int Bs[] = {0, 1, 2, 3, 8, 9, 16, 17, 18, 19, 32, 33, 64, 65, 128, 129, 0x7fffffff};
    const int Ms[] = {1, 2, 16384, 16385};
    int rc = 0;
    for (int b : Bs)
        for (int n : Ns)
            for (int m : Ms) rc |= one(b, n, m);
    // the ends of the int range, one argument at a time on three shapes and in every combination
    const int ends[] = {-0x7fffffff - 1, -1, 0, 1, 0x7ffffffe, 0x7fffffff};
    const int base[3][3] = {{2, 1000, 16}, {9, 40000, 48}, {65, 262144, 12}};
    for (const auto& s : base)
        for (int i = 0; i < 3; i++)
            for (int v : ends) {
                int d[3];
                memcpy(d, s, sizeof(d));
                d[i] = v;
                rc |= one(d[0], d[1], d[2]);
            }
    for (int b : ends)
        for (int n : ends)
            for (int m : ends) rc |= one(b, n, m);
    for (int b : ends)
        for (int n : {24576, 24577, 262143, 262144}) rc |= one(b, n, 0x7fffffff);
    printf("%llu plans (none %llu, plain %llu, pruned %llu, co-operative %llu, big %llu; rejected %llu), checksum %016llx\n", count,
           kernels[kFpsNone], kernels[kFpsPlain], kernels[kFpsPruned], kernels[kFpsCoop], kernels[kFpsBig], bad[1] + bad[2] + bad[3], sum);
    return rc;
}
