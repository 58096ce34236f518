// knn_plan.hpp — everything the host decides about an exact k-nearest-neighbour search (knn.hip), stated once: knn_plan().
// sph3d_build_nearest_neighbor launches what the plan says, sph3d_build_nearest_neighbor_workspace reads its size from it, and
// sph3d_build_nearest_neighbor_plan reports it field by field (tests/test_knn_forms.py holds that report to tests/_knn_forms.py,
// the launcher restated in Python).  Plain C++ in 64-bit integers: nothing of HIP is included, no global and no environment is
// read, so a host program can compile it alone (tools/knn_plan_sweep.cpp, built with the sanitizers).
#pragma once

namespace sph3d {

constexpr int kKnnMaxK = 64;                // the running list holds one candidate per lane of a wave
// a workgroup's waves, and the queries a wave carries through every tile.  Four per wave (one tile load and one LDS read serving
// four lists) measured SLOWER than one at every shape of tools/exp_knn.py (16 x 768 -> 2048, k = 3: 74.8 against 62.8 us; 16 x 128 ->
// 384: 26.4 against 15.9): the insertions, not the tile loads, bound the scan, and a wave's four lists are merged one after the other
constexpr int kKnnWaves = 4, kKnnPerWave = 1;
constexpr int kKnnQueries = kKnnWaves * kKnnPerWave;        // queries per workgroup
constexpr int kKnnBlock = 64 * kKnnWaves;
constexpr int kKnnTile = 1024;              // database points per LDS tile of the scan form (x, y, z planes: 12 KB)
// AUTO: clouds of at most this many points are scanned, larger ones go through the cell grid: the measured crossover
constexpr int kKnnScanMax = 2048;
constexpr long long kKnnMaxGrid = 1LL << 20;        // workgroups of a launch; every kernel strides over its work items
constexpr long long kKnnMaxElems = 1LL << 40;       // B N and B M: the byte counts formed from them stay far inside 64 bits
// the cell grid of a cloud: nn1grid.hpp's layout and constants (knn.hip asserts that these are its values)
constexpr int kKnnMinCells = 64, kKnnMaxCells = 1 << 21;
constexpr long long kKnnHdrBytes = 256;
constexpr int kKnnBuildBlock = 256, kKnnBuildParts = 64;    // the build's strided passes: at most 64 workgroups of 256 per cloud
constexpr int kKnnPrefixBlock = 1024;                       // the cell scan: one workgroup per cloud

enum { kKnnNone = 0, kKnnScan, kKnnGrid };                                  // KnnPlan::form
enum { kKnnModeAuto = 0, kKnnModeScan, kKnnModeGrid };                      // knn_plan's `mode`
enum { kKnnOk = 0, kKnnBadK, kKnnBigK, kKnnBadRadius, kKnnBadDims, kKnnBadSize, kKnnBadMode };     // KnnPlan::bad

struct KnnPlan {            // (the order of sph3d_build_nearest_neighbor_plan's output, up to `bad`)
    long long form;                     // kKnnNone: B == 0 or M == 0, nothing is launched
    long long queries;                  // queries per workgroup (a wave each)
    long long block;                    // threads per workgroup of the search kernels
    long long groups;                   // workgroups' worth of queries per cloud: ceil(M / queries)
    long long scan_grid, scan_lds;      // knn_scan_kernel: workgroups (0: not launched) and static LDS bytes
    long long search_grid, search_lds;  // knn_grid_kernel (grid form)
    long long fallback;                 // grid form: knn_scan_kernel is queued behind the search, gated per cloud on the device flag
    long long cells, cell_cap;          // grid form: cells a cloud's grid may have (about two points per cell), and the ceiling on it
    long long build_block, build_parts, build_grid;     // grid form: bounding box, count and fill passes (build_parts workgroups per cloud)
    long long setup_grid;               // grid form: header reset and grid shape, a thread per cloud
    long long prefix_block, prefix_grid;                // grid form: the scan of a cloud's cell counts, a workgroup per cloud
    long long workspace_bytes;          // device memory the call needs, the byte offsets into it and the strides per cloud:
    long long off_hdr, off_cells, off_points;           // headers [B], cell ends [B][cells + 1], sorted points [B][N] float4
    long long hdr_stride, cell_stride, point_stride;
    int bad;                            // (not reported)
};

static inline long long knn_cell_cap(long long n)            // nn1_cell_cap
{
    const long long c = n / 2;
    return c < kKnnMinCells ? kKnnMinCells : (c > kKnnMaxCells ? kKnnMaxCells : c);
}

// radius: +inf is "no radius" (R2 = inf admits every finite d2)
static inline KnnPlan knn_plan(int B_, int N_, int M_, int k_, float radius, int mode)
{
    KnnPlan p = {};
    const long long B = B_, N = N_, M = M_, k = k_;          // (every product below: in 64 bits)
    if (!(k >= 1)) { p.bad = kKnnBadK; return p; }
    if (!(k <= kKnnMaxK)) { p.bad = kKnnBigK; return p; }
    if (!(radius > 0)) { p.bad = kKnnBadRadius; return p; }
    if (!(B >= 0 && N >= 1 && M >= 0)) { p.bad = kKnnBadDims; return p; }
    if (!(B * N <= kKnnMaxElems && B * M <= kKnnMaxElems)) { p.bad = kKnnBadSize; return p; }
    if (!(mode == kKnnModeAuto || mode == kKnnModeScan || mode == kKnnModeGrid)) { p.bad = kKnnBadMode; return p; }
    if (B == 0 || M == 0) return p;
    auto cap = [](long long v) { return v < kKnnMaxGrid ? v : kKnnMaxGrid; };
    p.queries = kKnnQueries;
    p.block = kKnnBlock;
    p.groups = (M + kKnnQueries - 1) / kKnnQueries;
    const long long items = B * p.groups;
    p.scan_lds = 12 * kKnnTile;
    const bool grid = mode == kKnnModeGrid || (mode == kKnnModeAuto && N > kKnnScanMax);
    if (!grid) {
        p.form = kKnnScan;
        p.scan_grid = cap(items);
        return p;
    }
    p.form = kKnnGrid;
    p.search_grid = p.scan_grid = cap(items);
    p.fallback = 1;
    p.cells = knn_cell_cap(N);
    p.cell_cap = kKnnMaxCells;
    p.build_block = kKnnBuildBlock;
    p.build_parts = (N + kKnnBuildBlock - 1) / kKnnBuildBlock;
    if (p.build_parts > kKnnBuildParts) p.build_parts = kKnnBuildParts;
    p.build_grid = cap(B * p.build_parts);
    p.setup_grid = cap((B + kKnnBuildBlock - 1) / kKnnBuildBlock);
    p.prefix_block = kKnnPrefixBlock;
    p.prefix_grid = cap(B);
    p.hdr_stride = kKnnHdrBytes;
    p.cell_stride = (4 * (p.cells + 1) + 255) & ~255LL;
    p.point_stride = 16 * N;
    p.off_hdr = 0;
    p.off_cells = p.off_hdr + B * p.hdr_stride;
    p.off_points = p.off_cells + B * p.cell_stride;
    p.workspace_bytes = p.off_points + B * p.point_stride;
    return p;
}

}  // namespace sph3d
