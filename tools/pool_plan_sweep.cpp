// pool_plan_sweep.cpp — pool_plan() (sph3d_gcn_amd/csrc/pool_plan.hpp) for every op over the grid of tests/test_pool_forms.py, the
// ends of the int range in every argument included, as a host program of its own: built with the sanitizers it shows that the
// plan's arithmetic has no undefined behaviour there.  Checks the invariants the test checks, prints the number of plans, how many
// took each kernel, how many were refused and why, and a checksum of their fields.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/pool_plan_sweep.cpp -o /tmp/pool_plan_sweep
//   /tmp/pool_plan_sweep
#include <initializer_list>
#include <limits>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "../sph3d_gcn_amd/csrc/pool_plan.hpp"

using namespace sph3d;

static unsigned long long sum = 1469598103934665603ull, count = 0, kernels[10] = {}, bad[7] = {};

static int fail(int op, int B, int Nin, int Mout, int C, int K, int F, const char* what)
{
    printf("pool_plan(%d, %d, %d, %d, %d, %d, %d): %s\n", op, B, Nin, Mout, C, K, F, what);
    return 1;
}

static int one(int op, int B, int Nin, int Mout, int C, int K, int F)
{
    const PoolPlan p = pool_plan(op, B, Nin, Mout, C, K, F);
    long long f[sizeof(PoolPlan) / sizeof(long long)] = {};
    memcpy(f, &p, offsetof(PoolPlan, bad));
    for (long long v : f) sum = (sum ^ (unsigned long long)v) * 1099511628211ull;
    sum = (sum ^ (unsigned long long)p.bad) * 1099511628211ull;
    count++;
    bad[p.bad]++;
#define CHECK(cond, what) if (!(cond)) return fail(op, B, Nin, Mout, C, K, F, what)
    if (p.bad) {
        for (long long v : f) CHECK(v == 0, "a refused call with a field set");
        return 0;
    }
    kernels[p.kernel]++;
    const long long b = B, n = Nin, m = Mout, c = C;
    const bool fwd = op == kPoolOpFwd || op == kPoolOpNarrow;
    if (p.kernel == kPoolNone) {
        CHECK(B == 0 || (Mout == 0 && (fwd || op == kPoolOpMaxGrad)), "nothing is launched for an empty call, and only for one");
        for (size_t i = 0; i < offsetof(PoolPlan, bad) / sizeof(long long); i++)
            CHECK(f[i] == 0 || i == offsetof(PoolPlan, zero_bytes) / sizeof(long long), "an empty call with a field set");
        return 0;
    }
    const long long points = fwd ? m : n;
    CHECK(p.grid >= 1 && p.grid <= 0x7fffffff && p.grid_y >= 1 && p.grid_y <= 65535 && p.block == 256 && p.lds <= 64 * 1024, "a launch's shape");
    if (p.kernel == kPoolFwdHalf || p.kernel == kPoolFwd || p.kernel == kPoolBwdT || p.kernel == kPoolMaxBwdT || p.kernel == kPoolMaxBwdRows) {
        CHECK((p.ppwg == 4 || p.ppwg == 16) && p.parts * p.ppwg >= points && (p.parts - 1) * p.ppwg < points, "parts of a cloud");
        CHECK(p.grid == conv_xcd_grid(b, p.parts) && p.grid >= b * p.parts && p.grid % 8 == 0, "the parts of every cloud over the XCDs");
        CHECK(p.parts <= 0x7fffffff, "parts: an int in the kernels");
    }
    if (p.V) CHECK(p.V == (c % 4 == 0 ? 4 : 1) && (p.pairs || (p.passes * 64 * p.V >= c && (p.passes - 1) * 64 * p.V < c)), "channels per lane and passes");
    if (p.pairs) CHECK(p.V == 4 && c <= kPoolPairsMaxC && (p.kernel == kPoolFwdHalf || p.kernel == kPoolBwdTSplit), "the pairing body");
    if (p.kernel == kPoolBwdTSplit) CHECK(p.grid == b * n && p.grid <= kPoolSplitMaxSources && m >= 2 * n && p.lds == 4 * 64 * p.V * 4, "the split gather");
    if (p.kernel == kPoolBwdT) CHECK(b * n > kPoolSplitMaxSources || m < 2 * n, "the plain gather");
    if (p.kernel == kPoolMaxBwd)
        CHECK(p.grid == (p.blocks_wanted < p.blocks_cap ? p.blocks_wanted : p.blocks_cap) && p.grid_y == b && p.grid * b <= kPoolScatterWGs + b &&
                  p.zero_bytes > 0 && (p.zero_bytes == kConvHuge || (p.zero_bytes % c == 0 && p.zero_bytes / c == 4 * b * n)),
              "the scatter");
    if (p.kernel == kPoolNarrowFwd || p.kernel == kPoolNarrowBwdT)
        CHECK(c <= kPoolNarrowMaxC && p.grid <= kPoolNarrowMaxWGs && (p.grid == kPoolNarrowMaxWGs || (p.grid * p.ppwg >= b * points && (p.grid - 1) * p.ppwg < b * points)),
              "narrow rows");
    if (op == kPoolOpMaxGradRows) CHECK(n * F < 0x7fffffffLL, "segments of the offsets");
#undef CHECK
    return 0;
}

int main()
{
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    // (the lists of tests/test_pool_forms.py)
    const int Cs[] = {1, 3, 4, 16, 17, 124, 128, 129, 132, 256, 260, 516, 0, -4, imax, imin};
    const int Bs[] = {0, 1, 2, 3, 5, 64, 65535, 65536, imax - 7, imax - 6, imax, -1, imin};
    const int Ns[] = {1, 2, 15, 16, 17, 100, 32767, 32768, 65535, 65536, 65537, 262144, 262145, 1048576, 1048577, imax, 0, -1, imin};
    const int ends[] = {imin, -1, 0, 1, imax - 1, imax};
    int rc = 0;
    for (int op = kPoolOpFwd; op <= kPoolOpNarrowGradT; op++) {
        for (int B : Bs)
            for (int N : Ns)
                for (int C : Cs) {
                    rc |= one(op, B, N, 0, C, 1, 33);
                    for (int M : Ns) rc |= one(op, B, N, M, C, 1, 33);
                }
        // the boundaries on the row count: Mout against 2 Nin, M C against 256 * cap
        for (int C : Cs)
            for (int N : {1, 100, 21845, 32768, 65536, 65537}) {
                for (int B : {1, 2, 3, 64})
                    for (int d : {-1, 0, 1}) rc |= one(op, B, N, 2 * N + d, C, 1, 1);
                if (C > 0 && C <= 516)
                    for (int B : {1, 3, 64, 8192, 65535})
                        for (int d : {0, 1, 2}) rc |= one(op, B, N, (int)(256 * ((8192 + B - 1) / B) / C) + d, C, 1, 1);
            }
        // K and F, and every combination of the ends of the int range
        for (int K : ends)
            for (int F : ends) rc |= one(op, 3, 100, 300, 8, K, F);
        for (int F : {2, 32768, 46341, imax - 1})
            for (int N : {(1 << 30) - 1, 1 << 30, 65535, 65536, 46340, 46341, 1}) rc |= one(op, 1, N, 7, 8, 1, F);
        for (int B : ends)
            for (int N : ends)
                for (int M : ends)
                    for (int C : ends) rc |= one(op, B, N, M, C, imax, imax);
    }
    for (int op : {-1, 7, imax, imin}) rc |= one(op, 3, 100, 300, 8, 1, 1);
    printf("%llu plans; kernels:", count);
    for (unsigned long long k : kernels) printf(" %llu", k);
    printf("; refused:");
    for (int i = 1; i < 7; i++) printf(" %llu", bad[i]);
    printf("; checksum %016llx\n", sum);
    for (int i = 0; i < 10; i++) rc |= kernels[i] == 0;           // every kernel of the file was planned
    for (int i = 1; i < 7; i++) rc |= bad[i] == 0;                // and every refusal given
    return rc;
}
