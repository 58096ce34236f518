// nn_plan_sweep.cpp — nn_plan() (sph3d_gcn_amd/csrc/nn_plan.hpp) over the grid of tests/test_nn_forms.py, the ends of the int range
// and the radii no search should meet, as a host program of its own: built with the sanitizers it shows that the plan's
// arithmetic has no undefined behaviour there.  Prints the number of plans and a checksum of their fields.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/nn_plan_sweep.cpp -o /tmp/nn_plan_sweep
//   /tmp/nn_plan_sweep
#include <initializer_list>
#include <limits>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "../sph3d_gcn_amd/csrc/nn_plan.hpp"

using namespace sph3d;

static unsigned long long sum = 1469598103934665603ull, count = 0;

static void one(int B, int N, int M, int K, float radius)
{
    for (int fixed = 0; fixed < 2; fixed++)
        for (int fuse = 0; fuse < 2; fuse++)
            for (int memory = kNnMemNone; memory <= kNnMemLibrary; memory++) {
                const NnPlan p = nn_plan(fixed, B, N, M, K, radius, fuse != 0, memory);
                long long f[sizeof(NnPlan) / sizeof(long long)] = {};
                memcpy(f, &p, offsetof(NnPlan, bad));
                for (long long v : f) sum = (sum ^ (unsigned long long)v) * 1099511628211ull;
                sum = (sum ^ (unsigned long long)p.bad) * 1099511628211ull;
                count++;
            }
}

int main()
{
    const int Ns[] = {1, 128, 700, 1023, 1024, 1025, 2048, 4096, 12288, 12289, 65536, 65537};
    const int Ms[] = {0, 1, 63, 64, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 5119, 5120, 5121, 65536, 65537};
    const int Bs[] = {0, 1, 2, 3, 16, 32, 33, 64, 65, 131064, 131065};
    const int Ks[] = {1, 160, 161, 256, 257, 320, 321, 640, 641};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float radii[] = {0.02f, 0.03f, 0.11f, 0.5f, 0.1f, 0.0f, -0.0f, -1.0f, std::numeric_limits<float>::denorm_min(),
                           std::numeric_limits<float>::min(), std::numeric_limits<float>::max(), inf, -inf, nan};
    for (int B : Bs)
        for (int N : Ns)
            for (int M : Ms)
                for (int K : Ks)
                    for (float r : radii) one(B, N, M, K, r);
    // the ends of the int range, one dimension at a time and all at once
    const int ends[] = {-0x7fffffff - 1, -1, 0, 1, 0x7fffffff};
    const int base[4][4] = {{3, 128, 128, 16}, {16, 8192, 8192, 64}, {40, 2048, 2048, 8}, {1, 65536, 65536, 256}};       // B, N, M, K
    for (float r : radii) {
        for (const auto& b : base)
            for (int i = 0; i < 4; i++)
                for (int v : ends) {
                    int d[4];
                    memcpy(d, b, sizeof(d));
                    d[i] = v;
                    one(d[0], d[1], d[2], d[3], r);
                }
        for (int v : ends) one(v, v, v, v, r);
        // ... and the largest batches the grid's shape test lets through
        for (int B : {0x7fffffff, 0x7fffffe0, 1 << 30})
            for (int N : {1024, 65536})
                for (int M : {64, 1024, 65536, 0x7fffffff}) one(B, N, M, 0x7fffffff, r), one(B, N, M, 1, r);
    }
    printf("%llu plans, checksum %016llx\n", count, sum);
    return 0;
}
