// knn_plan_sweep.cpp — knn_plan() (sph3d_gcn_amd/csrc/knn_plan.hpp) over the grid of tests/test_knn_forms.py, the ends of the int
// range in every argument included, as a host program of its own: built with the sanitizers it shows that the plan's arithmetic has
// no undefined behaviour there.  Checks the invariants the test checks, prints the number of plans, how many took each form, and a
// checksum of their fields.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/knn_plan_sweep.cpp -o /tmp/knn_plan_sweep
//   /tmp/knn_plan_sweep
#include <initializer_list>
#include <limits>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "../sph3d_gcn_amd/csrc/knn_plan.hpp"

using namespace sph3d;

static unsigned long long sum = 1469598103934665603ull, count = 0, forms[3] = {}, bad[7] = {};

static int fail(int B, int N, int M, int k, float radius, int mode, const char* what)
{
    printf("knn_plan(%d, %d, %d, %d, %g, %d): %s\n", B, N, M, k, radius, mode, what);
    return 1;
}

static int one(int B, int N, int M, int k, float radius, int mode)
{
    const KnnPlan p = knn_plan(B, N, M, k, radius, mode);
    long long f[sizeof(KnnPlan) / sizeof(long long)] = {};
    memcpy(f, &p, offsetof(KnnPlan, bad));
    for (long long v : f) sum = (sum ^ (unsigned long long)v) * 1099511628211ull;
    sum = (sum ^ (unsigned long long)p.bad) * 1099511628211ull;
    count++;
    bad[p.bad]++;
#define CHECK(cond, what) if (!(cond)) return fail(B, N, M, k, radius, mode, what)
    if (p.bad) {
        for (long long v : f) CHECK(v == 0, "a rejected call with a field set");
        return 0;
    }
    forms[p.form]++;
    const long long b = B, n = N, m = M;
    CHECK((p.form == kKnnNone) == (B == 0 || M == 0), "an empty call launches nothing, and only an empty call");
    CHECK((p.workspace_bytes > 0) == (p.form == kKnnGrid) && (p.fallback != 0) == (p.form == kKnnGrid), "workspace and fallback: the grid's");
    for (long long g : {p.scan_grid, p.search_grid, p.build_grid, p.setup_grid, p.prefix_grid}) CHECK(g >= 0 && g <= kKnnMaxGrid, "workgroups of a launch");
    CHECK(p.scan_lds <= 64 * 1024 && p.search_lds <= 64 * 1024 && p.block <= 1024 && p.build_block <= 1024 && p.prefix_block <= 1024, "LDS and threads of a launch");
    if (p.form == kKnnNone) {
        for (long long v : f) CHECK(v == 0, "an empty call with a field set");
        return 0;
    }
    CHECK(p.block == kKnnBlock && p.queries == kKnnQueries && p.groups * p.queries >= m && (p.groups - 1) * p.queries < m, "queries per cloud");
    CHECK(p.scan_grid >= 1 && (p.scan_grid == b * p.groups || p.scan_grid == kKnnMaxGrid), "scan launch");
    if (mode == kKnnModeScan) CHECK(p.form == kKnnScan, "a forced scan");
    if (mode == kKnnModeGrid) CHECK(p.form == kKnnGrid, "a forced grid");
    if (mode == kKnnModeAuto) CHECK((p.form == kKnnScan) == (n <= kKnnScanMax), "AUTO's threshold");
    if (p.form == kKnnScan) {
        CHECK(p.search_grid == 0 && p.build_grid == 0 && p.setup_grid == 0 && p.prefix_grid == 0 && p.cells == 0, "a scan launches one kernel");
        return 0;
    }
    CHECK(p.search_grid == p.scan_grid && p.build_grid >= 1 && p.setup_grid >= 1 && p.prefix_grid >= 1, "grid launches");
    CHECK(p.off_hdr == 0 && p.off_cells == b * p.hdr_stride && p.off_points == p.off_cells + b * p.cell_stride &&
              p.workspace_bytes == p.off_points + b * p.point_stride && p.point_stride == 16 * n,
          "workspace layout");
    CHECK(p.off_cells % 16 == 0 && p.off_points % 16 == 0 && p.cell_stride % 16 == 0 && p.workspace_bytes < (1LL << 62), "alignment and size");
    CHECK(p.cells >= kKnnMinCells && p.cells <= p.cell_cap && p.cell_cap == kKnnMaxCells && 4 * (p.cells + 1) <= p.cell_stride &&
              (2 * p.cells <= n || p.cells == kKnnMinCells),
          "cells of a cloud");
    CHECK(p.build_parts >= 1 && p.build_parts <= kKnnBuildParts && (p.build_parts - 1) * p.build_block < n, "build passes");
#undef CHECK
    return 0;
}

int main()
{
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    // (the lists of tests/test_knn_forms.py)
    const int Ks[] = {1, 2, 63, 64, 65, 0, -1, imax, imin};
    const int Ns[] = {1, 2, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 65536,
                      (1 << 22) - 1, 1 << 22, (1 << 22) + 2, imax, 0, -1, imin};
    const int Bs[] = {0, 1, 2, 255, 256, 257, 511, 512, 513, 1 << 14, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, imax, -1, imin};
    const int Ms[] = {0, 1, 3, 4, 5, 2048, 8192, (1 << 22) - 3, 1 << 22, (1 << 22) + 1, imax, -1, imin};
    const float Rs[] = {std::numeric_limits<float>::infinity(), 0.15f};
    int rc = 0;
    for (int B : Bs)
        for (int N : Ns)
            for (int M : Ms)
                for (int k : Ks)
                    for (float r : Rs)
                        for (int mode : {kKnnModeAuto, kKnnModeScan, kKnnModeGrid}) rc |= one(B, N, M, k, r, mode);
    // radii and modes the entry refuses, and every combination of the ends of the int range
    const float badR[] = {0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity()};
    for (float r : badR) rc |= one(2, 1500, 1500, 16, r, kKnnModeAuto);
    for (int mode : {-1, 3, imax, imin}) rc |= one(2, 1500, 1500, 16, 1.0f, mode);
    const int ends[] = {imin, -1, 0, 1, imax - 1, imax};
    for (int B : ends)
        for (int N : ends)
            for (int M : ends)
                for (int k : {1, 64})
                    for (int mode : {kKnnModeAuto, kKnnModeGrid}) rc |= one(B, N, M, k, 1.0f, mode);
    printf("%llu plans (none %llu, scan %llu, grid %llu; rejected %llu), checksum %016llx\n", count, forms[kKnnNone], forms[kKnnScan],
           forms[kKnnGrid], bad[1] + bad[2] + bad[3] + bad[4] + bad[5] + bad[6], sum);
    return rc;
}
