// pool_plan.hpp — everything the host decides about a launch of pooling, un-pooling and their gradients (pool3d.hip), stated
// once: pool_plan().  Every entry point of pool3d.hip launches what the plan says, and sph3d_pool3d_plan reports it field by
// field (tests/test_pool_forms.py holds that report to tests/_pool_forms.py, the launchers restated in Python as they stood
// before the choice was gathered here).  Plain C++ in 64-bit integers: nothing of HIP is included, no global and no environment
// is read, so a host program can compile it alone (tools/pool_plan_sweep.cpp, built with the sanitizers).
#pragma once
#include "conv_plan.hpp"        // conv_xcd_grid: common.hpp's xcd_grid in 64 bits; conv_mul

namespace sph3d {

constexpr int kPoolBlock = 256;             // four waves, in every kernel of the file
// Output (forward) or source (gradient) points per workgroup of the wave-per-point gathers: these kernels have no per-workgroup
// prologue, so the small levels (a few thousand points) take ONE point per wave — four per wave left them with 2-8 waves per
// SIMD walking 4 x ~50 dependent gathers each (tools/exp_calls.py: max pooling 36 -> 17 us at 16 x 128 points of 512 channels,
// 80 -> 64 us at level 0); launches of >= 65536 points keep four per wave (mean interpolation at level 0: 80 vs 82 us).
constexpr int kPtsPerWG = 16, kPtsPerWGSmall = 4;
constexpr long long kPoolManyPoints = 65536;
constexpr int kPoolPairsMaxC = 128;         // a row of at most 32 lanes x 16 bytes: the halves of a wave take alternate rows
// the split gather (one workgroup per source): few sources, each with (Mout / Nin) x more in-edges than a target has neighbours
constexpr long long kPoolSplitMaxSources = 65536;
// the scatter: a thread per element up to about 8192 workgroups in all, grid-stride beyond; the clouds are the grid's y
constexpr long long kPoolScatterWGs = 8192, kPoolScatterMaxB = 65535;
// narrow rows: 16 lanes own a row of at most 16 channels (forward: 16 rows per workgroup; gradient: a wave per source)
constexpr int kPoolNarrowMaxC = 16, kPoolNarrowRows = 16, kPoolNarrowSources = 4;
constexpr long long kPoolNarrowMaxWGs = 65536;

// op: the entry point (include/sph3d.h: SPH3D_POOL_*)
enum { kPoolOpFwd = 0, kPoolOpSumGradT, kPoolOpMaxGrad, kPoolOpMaxGradT, kPoolOpMaxGradRows, kPoolOpNarrow, kPoolOpNarrowGradT };
// PoolPlan::kernel.  none: nothing is launched and every other field but zero_bytes is 0
enum { kPoolNone = 0, kPoolFwdHalf, kPoolFwd, kPoolBwdT, kPoolBwdTSplit, kPoolMaxBwd, kPoolMaxBwdT, kPoolMaxBwdRows, kPoolNarrowFwd,
       kPoolNarrowBwdT };
// PoolPlan::bad.  wide: SPH3D_EUNSUPPORTED, the others SPH3D_EINVAL
enum { kPoolOk = 0, kPoolBadOp, kPoolBadDims, kPoolBadSegments, kPoolBadBatch, kPoolWide, kPoolBadGrid };

struct PoolPlan {           // (the order of sph3d_pool3d_plan's output, up to `bad`)
    long long kernel;
    long long V;                        // channels per lane of the instantiation, 4 or 1; 0: the kernel has no such parameter
    long long pairs;                    // the halves of a wave take alternate rows (gather_fwd_half; the split gather at V == 4, C <= 128)
    long long passes;                   // channel passes of a wave over a row
    long long ppwg;                     // points (rows, sources) per workgroup
    long long parts;                    // workgroups' worth of work per cloud (the scatter: grid.x; narrow: 0, the rows are not cut by cloud)
    long long grid, grid_y;             // workgroups: grid.x and grid.y
    long long block;
    long long lds;                      // static LDS bytes
    long long zero_bytes;               // the scatter: bytes of grad_input cleared in front of the launch
    long long blocks_wanted, blocks_cap;        // the scatter: workgroups per cloud its elements ask for, and the ceiling on grid.x
    int bad;                            // (not reported)
};

static inline long long pool_ppwg(long long points) { return points >= kPoolManyPoints ? kPtsPerWG : kPtsPerWGSmall; }

// Nin: points gathered FROM (forward) or gradients written TO; Mout: rows of the neighbour graph.  K: forward ops; F: kPoolOpMaxGradRows
static inline PoolPlan pool_plan(int op, int B_, int Nin_, int Mout_, int C_, int K_, int F_)
{
    PoolPlan p = {};
    const long long B = B_, Nin = Nin_, Mout = Mout_, C = C_, K = K_, F = F_;        // (every product below: in 64 bits)
    auto ceil_div = [](long long a, long long b) { return (a + b - 1) / b; };
    if (!(op >= kPoolOpFwd && op <= kPoolOpNarrowGradT)) { p.bad = kPoolBadOp; return p; }
    const bool fwd = op == kPoolOpFwd || op == kPoolOpNarrow;
    if (!(B >= 0 && Nin > 0 && Mout >= 0 && C > 0 && (!fwd || K > 0) && (op != kPoolOpMaxGradRows || F > 0))) { p.bad = kPoolBadDims; return p; }
    if (op == kPoolOpMaxGradRows && !(Nin * F < 0x7fffffffLL)) { p.bad = kPoolBadSegments; return p; }
    const bool narrow = op == kPoolOpNarrow || op == kPoolOpNarrowGradT;
    if (narrow && C > kPoolNarrowMaxC) { p.bad = kPoolWide; return p; }
    if (B == 0 || (fwd && Mout == 0)) return p;
    const long long V = C % 4 == 0 ? 4 : 1;
    p.block = kPoolBlock;
    p.grid_y = 1;
    switch (op) {
    case kPoolOpFwd:
        p.kernel = V == 4 && C <= kPoolPairsMaxC ? kPoolFwdHalf : kPoolFwd;
        p.V = V;
        p.pairs = p.kernel == kPoolFwdHalf;
        p.passes = p.pairs ? 1 : ceil_div(C, 64 * V);
        p.ppwg = pool_ppwg(B * Mout);
        p.parts = ceil_div(Mout, p.ppwg);
        p.grid = conv_xcd_grid(B, p.parts);
        break;
    case kPoolOpSumGradT:
        p.V = V;
        p.passes = ceil_div(C, 64 * V);
        if (B * Nin <= kPoolSplitMaxSources && Mout >= 2 * Nin) {
            p.kernel = kPoolBwdTSplit;
            p.pairs = V == 4 && C <= kPoolPairsMaxC;
            p.ppwg = 1;
            p.parts = Nin;
            p.grid = B * Nin;
            p.lds = 4 * 64 * V * 4;             // part[4][64 * V] floats
        } else {
            p.kernel = kPoolBwdT;
            p.ppwg = kPtsPerWG;
            p.parts = ceil_div(Nin, p.ppwg);
            p.grid = conv_xcd_grid(B, p.parts);
        }
        break;
    case kPoolOpMaxGrad:
        p.zero_bytes = conv_mul(conv_mul(4 * B, Nin), C);
        if (Mout == 0) {                        // nothing to scatter: the cleared gradient is the answer
            const long long bytes = p.zero_bytes;
            p = {};
            p.zero_bytes = bytes;
            return p;
        }
        if (B > kPoolScatterMaxB) { p = {}; p.bad = kPoolBadBatch; return p; }
        p.kernel = kPoolMaxBwd;
        p.blocks_wanted = ceil_div(Mout * C, kPoolBlock);
        p.blocks_cap = ceil_div(kPoolScatterWGs, B) > 1 ? ceil_div(kPoolScatterWGs, B) : 1;
        p.parts = p.grid = p.blocks_wanted < p.blocks_cap ? p.blocks_wanted : p.blocks_cap;
        p.grid_y = B;
        break;
    case kPoolOpMaxGradT:
    case kPoolOpMaxGradRows:
        p.kernel = op == kPoolOpMaxGradT ? kPoolMaxBwdT : kPoolMaxBwdRows;
        p.V = V;
        p.passes = ceil_div(C, 64 * V);
        p.ppwg = pool_ppwg(B * Nin);
        p.parts = ceil_div(Nin, p.ppwg);
        p.grid = conv_xcd_grid(B, p.parts);
        break;
    case kPoolOpNarrow:
    case kPoolOpNarrowGradT: {
        const bool f = op == kPoolOpNarrow;
        p.kernel = f ? kPoolNarrowFwd : kPoolNarrowBwdT;
        p.passes = 1;
        p.ppwg = f ? kPoolNarrowRows : kPoolNarrowSources;
        const long long wgs = ceil_div(B * (f ? Mout : Nin), p.ppwg);
        p.grid = wgs < kPoolNarrowMaxWGs ? wgs : kPoolNarrowMaxWGs;         // (the kernels stride over their rows)
        break;
    }
    }
    if (p.grid > 0x7fffffff) { p = {}; p.bad = kPoolBadGrid; return p; }            // (a launch's workgroups: an int)
    return p;
}

}  // namespace sph3d
