// lovasz_plan_sweep.cpp — lovasz_large_plan() (sph3d_gcn_amd/csrc/lovasz_plan.hpp) over the grid of tests/test_lovasz_large.py and
// the ends of the int range in every argument, as a host program of its own: built with the sanitizers it shows that the plan's
// arithmetic has no undefined behaviour there.  Checks the invariants the test checks, prints the number of plans, how many were
// refused for each reason, and a checksum of their fields.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lovasz_plan_sweep.cpp -o /tmp/lovasz_plan_sweep
//   /tmp/lovasz_plan_sweep
#include <initializer_list>
#include <limits>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "../sph3d_gcn_amd/csrc/lovasz_plan.hpp"

using namespace sph3d;

static unsigned long long sum = 1469598103934665603ull, count = 0, empty = 0, bad[7] = {};

static int fail(int B, int N, int C, int t, int slab, const char* what)
{
    printf("lovasz_large_plan(%d, %d, %d, %d, %d): %s\n", B, N, C, t, slab, what);
    return 1;
}

static int one(int B, int N, int C, int t, int slab)
{
    const LovaszPlan p = lovasz_large_plan(B, N, C, t, slab);
    long long f[sizeof(LovaszPlan) / sizeof(long long)] = {};
    memcpy(f, &p, offsetof(LovaszPlan, bad));
    for (long long v : f) sum = (sum ^ (unsigned long long)v) * 1099511628211ull;
    sum = (sum ^ (unsigned long long)p.bad) * 1099511628211ull;
    count++;
    bad[p.bad]++;
#define CHECK(cond, what) if (!(cond)) return fail(B, N, C, t, slab, what)
    if (p.bad || B == 0) {
        for (long long v : f) CHECK(v == 0, "a rejected or empty call with a field set");
        empty += p.bad == 0;
        return 0;
    }
    const long long b = B, n = N, c = C;
    CHECK(p.tile == 1LL << p.tile_log2 && p.tile_log2 == (t ? t : kLovDefaultTileLog2), "run length");
    CHECK((p.runs - 1) * p.tile < n && n <= p.npad && p.npad == p.runs * p.tile && p.runs <= 1024, "runs cover the rows");
    CHECK((1LL << p.passes) >= p.runs && (p.passes == 0 || (1LL << (p.passes - 1)) < p.runs) && p.passes <= 10, "merge passes");
    CHECK(p.mtile == kLovMergeTile && p.mtile <= p.tile && p.mtiles * p.mtile == p.npad && p.mtiles <= 1024, "output tiles");
    CHECK(p.slab >= 1 && p.slab <= c && (p.slabs - 1) * p.slab < c && c <= p.slabs * p.slab, "slabs partition the classes");
    CHECK(slab == 0 || p.slab == slab, "a forced slab");
    CHECK(p.sort_lds == 8 * p.tile && p.sort_lds <= 160 * 1024 - 4096 && p.merge_lds == 8 * kLovMergeTile, "LDS of a launch");
    CHECK(p.probs_grid >= 1 && p.probs_grid <= 0x7fffffffLL && p.probs_grid * 256 >= b * n && (p.probs_grid - 1) * 256 < b * n, "probs launch");
    CHECK(p.count_grid * kLovCountRows >= n && (p.count_grid - 1) * kLovCountRows < n && p.grad_grid * 1024 >= n && (p.grad_grid - 1) * 1024 < n,
          "count and gradient launches");
    CHECK(p.runs <= 0x7fffffffLL && p.slab <= 65535 && b <= 65535, "grid (x, slab, B)");
    const long long keys = 8 * p.slab * b * p.npad, words = 4 * p.slab * b * p.mtiles;
    CHECK(p.key_bufs == (p.passes ? 2 : 1) && p.off_keys0 == 0 && p.off_keys1 == (p.passes ? keys : 0) && p.off_tilecnt == p.key_bufs * keys,
          "key buffers");
    CHECK(p.off_partial == p.off_tilecnt + words && p.off_count == p.off_partial + words && p.off_bad == p.off_count + 4 * b * c, "workspace layout");
    CHECK(p.workspace_bytes >= p.off_bad + 4 * b && p.workspace_bytes < p.off_bad + 4 * b + 256 && p.workspace_bytes % 256 == 0 &&
              p.workspace_bytes < (1LL << 62),
          "workspace size");
    CHECK(p.off_keys1 % 16 == 0 && p.off_tilecnt % 16 == 0 && p.off_partial % 4 == 0 && p.off_count % 4 == 0 && p.off_bad % 4 == 0, "alignment");
    CHECK(p.cap == kLovWsCap && (slab != 0 || p.workspace_bytes <= kLovWsCap || p.slab == 1), "the cap");
#undef CHECK
    return 0;
}

int main()
{
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    int rc = 0;
    // (the lists of tests/test_lovasz_large.py)
    for (int N : {1, 1023, 1024, 1025, 16384, 16385, 40000, 65536, 1 << 20})
        for (int C : {1, 2, 13, 21, 1024})
            for (int B : {0, 1, 4, 16})
                for (int t : {0, 10, 14})
                    for (int slab : {0, 1, 5}) rc |= one(B, N, C, t, slab);
    // every run length, the refusals, and every combination of the ends of the int range
    for (int t : {-1, 1, 9, 10, 11, 12, 13, 14, 15, imax, imin})
        for (int slab : {-1, 0, 1, 13, 14, imax, imin}) rc |= one(16, 65536, 13, t, slab);
    rc |= one(16, 65536, 21, 0, 0);
    rc |= one(65535, 16, 1024, 0, 0);
    rc |= one(65535, 1 << 20, 1, 10, 0);
    const int ends[] = {imin, -1, 0, 1, (1 << 20), (1 << 20) + 1, imax - 1, imax};
    for (int B : ends)
        for (int N : ends)
            for (int C : ends)
                for (int t : {0, 14, imax})
                    for (int slab : {0, 1, imax, imin}) rc |= one(B, N, C, t, slab);
    const LovaszPlan flag = lovasz_large_plan(16, 65536, 21, 0, 0);
    if (!(flag.slab == 7 && flag.slabs == 3 && flag.runs == 16 && flag.passes == 4 && flag.workspace_bytes <= kLovWsCap))
        rc |= fail(16, 65536, 21, 0, 0, "the case the cap is derived from: three slabs of seven classes");
    printf("%llu plans (empty %llu; refused: dims %llu, size %llu, N %llu, C %llu, tile %llu, slab %llu), checksum %016llx\n", count, empty,
           bad[kLovBadDims], bad[kLovBadSize], bad[kLovBigN], bad[kLovBigC], bad[kLovBadTile], bad[kLovBadSlab], sum);
    return rc;
}
