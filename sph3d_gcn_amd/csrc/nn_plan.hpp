// nn_plan.hpp — everything the host decides about a range search (nnquery.hip, nngrid.hip), stated once: nn_plan().  The seven
// search entry points launch what the plan says, sph3d_build_sphere_neighbor_workspace reads it, and
// sph3d_build_sphere_neighbor_plan reports it field by field (tests/test_nn_forms.py holds that report to tests/_nn_forms.py, the
// launchers restated in Python as they stood before the choice was gathered here).  Plain C++ in 64-bit integers: nothing of HIP
// is included, no global and no environment is read, so a host program can compile it alone (tools/nn_plan_sweep.cpp, built with
// the sanitizers).
#pragma once
#include "conv_plan.hpp"        // conv_xcd_grid: common.hpp's xcd_grid in 64 bits

namespace sph3d {

constexpr int kNnRefGrid = 32, kNnRefBlock = 1024;      // common.hpp's kRefGrid, kRefBlock (nngrid.hip asserts it)
constexpr long long kNnLds = 160 * 1024;                // LDS a workgroup can ask for

// ---- the chain kernel (nnquery_sphere_kernel)
constexpr int kWavesPerWG = 16;
constexpr int kMaxChunk = 12288;         // points per LDS chunk (3 * 12288 * 4 B = 144 KB)
constexpr int kThrTable = 64;            // positions of the radius sequence with a precomputed threshold
constexpr long long kHitsLds = 40 * 1024;        // deferred hit lists [wave][CPW][K] up to this many bytes; beyond, hits are written from inside the scan

// ---- the cell grid (nngrid_build_kernel, nngrid_qorder_kernel, nngrid_search_kernel)
constexpr int kGridMaxCells = 8192;      // LDS histogram of the build kernels (32 KB: they must fit beside the step's other kernels)
constexpr int kGridMaxK = 256;           // sorted hit lists of a wave's four queries: 4 * K * 2 B
constexpr int kGridMaxPos = 8;           // chain positions the grid may take (r_k <= kGridReach * r_0 bounds it further)
constexpr int kGridReach = 3;            // ... in units of r_0 = cells a query looks in every direction: (2 * 3 + 1)^2 = 49 columns
constexpr int kMaxPositions = 64;        // positions of a chain at M <= 65536 queries
// worth it from ~4 M point pairs per cloud (below, the chain kernel's scan of the whole cloud from LDS is as fast as the grid's
// build + search: 2048 x 512 measured 60 vs 68 us)
constexpr long long kGridMinPairs = 1LL << 22;
// ---- the early-stopping scan (nndense_kernel) and the small clouds it takes alone (nnsmall_prepare_kernel in front)
constexpr int kDenseQ = 4;               // queries per wave: they share every trip's points
// Small clouds: beyond 32 clouds (two clouds per reference block) the chain kernel keeps the call — and so do batches of one or two
// clouds: there its launch holds two CUs at most, so a step has nothing to win back from it, and the suite pins those batches to
// "no workspace, no launch counted" (test_abi, test_gpu_nngrid)
constexpr int kSmallMinClouds = 3;

// ---- the search's device memory: [0] the flag, [64] GridRadii, [1024] one GridHdr per cloud, then (grid) cell starts, the cloud
// in cell order as float4, the query orders.  nngrid.hip asserts the two struct sizes
constexpr long long kNnRadiiOffset = 64, kNnHdrOffset = 1024, kNnHdrBytes = 32, kNnRadiiBytes = 8 * kMaxPositions;

enum { kNnFrontNone = 0, kNnFrontGrid = 1, kNnFrontSmall = 2 };      // NnPlan::front
enum { kNnMemNone = 0, kNnMemCaller = 1, kNnMemLibrary = 2 };        // nn_plan's `memory`
enum { kNnOk = 0, kNnBadRadius, kNnBadSample, kNnBadDims };           // NnPlan::bad: why the entry point answers SPH3D_EINVAL

struct NnPlan {             // (the order of sph3d_build_sphere_neighbor_plan's output, up to `bad`)
    // The front: launches that compute every row of the call unless they raise the device flag; 0 where there is none
    long long front;
    long long npos;                     // grid: chain positions the grid takes (`fixed`: 1, and it takes every query)
    long long nq, nslices, parts, W;    // grid: queries per cloud in the visiting order, their slices of 1024, waves of four, bitmap words
    long long build_lds, search_lds;    // grid: dynamic LDS of nngrid_build_kernel / nngrid_qorder_kernel, of nngrid_search_kernel
    long long build_grid, order_grid, search_grid;          // grid: workgroups B, B nslices, xcd_grid(B, parts)
    long long j0;                       // the first query of a cloud the early-stopping scan takes (grid: M when it takes none; small: 0)
    long long dparts, dense_lds, dense_grid;                // nndense_kernel (0 when j0 == M)
    long long prepare_block;            // small: threads of nnsmall_prepare_kernel's one workgroup
    long long workspace_bytes;          // the front's device memory and the byte offsets into it
    long long off_flag, off_radii, off_hdr, off_cells, off_points, off_order;
    // The chain kernel behind the front (alone: without one): nnquery_sphere_kernel<CPW, MULTI, DEFER, fused>
    long long CPW, MULTI, DEFER;
    long long chunkN, groups, chain_grid, chain_lds;        // chain_grid == 0: nothing is launched (B == 0 or M == 0)
    long long grid_done;                // chain positions the front has done unless its flag is up: 0 or 1 << 20 (all)
    long long fused;                    // the output passes compute bins and segment counts; 0: sph3d_build_sphere_graph* runs the separate kernels
    long long clear_counts;             // segments of F counters the gated clearing covers in front of the chain kernel (B N + 1), 0: not launched
    int bad;                            // (not reported)
};

static inline NnPlan nn_plan(int fixed, int B_, int N_, int M_, int K_, float radius, bool fuse_wanted, int memory)
{
    NnPlan p = {};
    const long long B = B_, N = N_, M = M_, K = K_;          // (every product below: in 64 bits)
    if (!(radius > 0)) { p.bad = kNnBadRadius; return p; }                      // tf_nnquery.cpp:60
    if (!(K > 0)) { p.bad = kNnBadSample; return p; }                           // :63
    if (!(B >= 0 && N > 0 && M >= 0)) { p.bad = kNnBadDims; return p; }
    if (B == 0 || M == 0) return p;
    auto ceil_div = [](long long a, long long b) { return (a + b - 1) / b; };
    auto hits_bytes = [](long long cpw, long long k) { const long long b = 4 * kWavesPerWG * cpw * k; return b <= kHitsLds ? b : 0; };
    // whole trips of 128 points next to the hit lists and the threshold table
    auto max_chunk = [](long long hb) { const long long c = (kNnLds - kThrTable * 4 - hb) / 12 & ~127LL; return c < kMaxChunk ? c : kMaxChunk; };
    const long long nb = B < kNnRefGrid ? B : kNnRefGrid, nt = M < kNnRefBlock ? M : kNnRefBlock;
    const long long slices = ceil_div(M, kNnRefBlock), have = ceil_div(B, kNnRefGrid) * slices;        // chain positions in use

    // ---- the chain kernel: CPW chains per wave while that leaves 256 waves; a cloud that does not fit LDS beside the hit lists
    // goes chunk by chunk, one chain per wave
    const long long chains = nb * nt;
    p.CPW = chains >= 256 * kWavesPerWG * 4 ? 4 : (chains >= 256 * kWavesPerWG * 2 ? 2 : 1);
    p.MULTI = N > max_chunk(hits_bytes(p.CPW, K));
    if (p.MULTI) p.CPW = 1;
    const long long hb = hits_bytes(p.CPW, K);
    p.DEFER = hb != 0;
    p.chunkN = p.MULTI ? max_chunk(hb) : N;
    p.groups = ceil_div(nt, kWavesPerWG * p.CPW);
    p.chain_grid = nb * p.groups;
    p.chain_lds = 12 * ((p.chunkN + 127) & ~127LL) + hb + kThrTable * 4;
    p.fused = fuse_wanted && p.DEFER;          // the bins come from the deferred output pass

    // ---- the front.  The grid: 16-bit indices in its sorted hit lists; with more than 32 clouds (two clouds per reference block:
    // its chains go on from one to the next) every thread must visit the same number of queries per cloud, so that a query's
    // position is a function of (cloud, j) alone.  Where it declines, clouds of at most 1024 points through its early-stopping
    // scan alone.  (At N = 1024 both can hold: the grid.)
    const bool k_ok = K <= kGridMaxK, m_ok = M <= (long long)kMaxPositions * kNnRefBlock;
    const bool grid = N >= 1024 && N <= 65536 && M >= 64 && m_ok && N * M >= kGridMinPairs && k_ok &&
                      (fixed || B <= kNnRefGrid || (!(M >= kNnRefBlock && M % kNnRefBlock != 0) && have <= kMaxPositions));
    const bool small = B >= kSmallMinClouds && B <= kNnRefGrid && N <= 1024 && m_ok && k_ok;
    if (memory == kNnMemNone || !(grid || small)) return p;
    const long long hdr_end = (kNnHdrOffset + kNnHdrBytes * B + 15) & ~15LL;
    p.off_radii = kNnRadiiOffset;
    p.off_hdr = kNnHdrOffset;
    p.dense_lds = 4 * 4 * kDenseQ * K;
    if (grid) {
        p.front = kNnFrontGrid;
        // chain positions whose radius stays <= 3 r_0 go through the grid; the later ones find nn_sample hits early in an ascending
        // scan (nndense_kernel)
        p.npos = 1;
        if (!fixed) {
            float rk = radius;
            while (p.npos < kGridMaxPos) {
                rk = (float)((double)rk + 0.05);          // tf_nnquery_gpu.cu:59
                if (!(rk <= kGridReach * radius)) break;
                p.npos++;
            }
            if (p.npos > have) p.npos = have;
        }
        p.nq = fixed ? M : (M < p.npos * kNnRefBlock ? M : p.npos * kNnRefBlock);
        p.nslices = ceil_div(p.nq, kNnRefBlock);
        p.parts = ceil_div(p.nq, 4);
        p.W = (ceil_div(N, 32) + 15) & ~15LL;
        p.build_lds = 4 * kGridMaxCells;
        p.search_lds = 4 * p.W * 4 + 4 * 64 * 8 + 4 * K * 2;          // bitmaps, column bounds, sorted hits of four queries
        p.build_grid = B;
        p.order_grid = B * p.nslices;
        p.search_grid = conv_xcd_grid(B, p.parts);
        // the first query any cloud leaves to the scan (the clouds of the last block round start at the highest positions): the
        // kernel skips the part of a cloud that its grid share covers
        p.j0 = M;
        if (!fixed) {
            long long sl = p.npos - (B - 1) / kNnRefGrid * slices;
            sl = sl < 0 ? 0 : (sl > slices ? slices : sl);
            p.j0 = sl * kNnRefBlock < M ? sl * kNnRefBlock : M;
        }
        p.off_cells = hdr_end;
        p.off_points = p.off_cells + ((4 * B * (kGridMaxCells + 1) + 15) & ~15LL);
        p.off_order = p.off_points + 16 * B * N;
        p.workspace_bytes = p.off_order + 4 * B * M;
    } else {
        p.front = kNnFrontSmall;
        p.prepare_block = 64 * (B < 16 ? B : 16);
        p.workspace_bytes = hdr_end;
    }
    if (p.j0 < M) {
        p.dparts = ceil_div(M - p.j0, 4 * kDenseQ);
        p.dense_grid = conv_xcd_grid(B, p.dparts);
    } else {
        p.dense_lds = 0;
    }
    p.grid_done = 1 << 20;
    p.clear_counts = p.fused ? B * N + 1 : 0;
    // a launch's workgroups are an int: a batch past that (from 131 072 clouds) is the chain kernel's
    if (p.order_grid > 0x7fffffff || p.search_grid > 0x7fffffff || p.dense_grid > 0x7fffffff) return nn_plan(fixed, B_, N_, M_, K_, radius, fuse_wanted, kNnMemNone);
    return p;
}

}  // namespace sph3d
