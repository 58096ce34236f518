// conv_plan.hpp — everything the host decides about a launch of the depthwise convolution or its gradient (conv3d.hip), stated
// once: conv_plan().  Every entry point of conv3d.hip launches what the plan says, the workspace queries and the two-input
// predicate read it, and sph3d_depthwise_conv3d_plan reports it field by field (tests/test_conv_forms.py holds that report to
// tests/_conv_forms.py, the rules restated in Python).  Plain C++ in 64-bit integers: nothing of HIP is included, no global and
// no environment is read, so a host program can compile it alone (tools/conv_plan_sweep.cpp, built with the sanitizers).
#pragma once

namespace sph3d {

constexpr int kSlice = 256;              // output channels per wave pass (64 lanes x 4)
constexpr int kFwdPointsPerWG = 32;
constexpr int kMultiWaves = 4;                        // dwconv_fwd_multi: waves per workgroup (they share one LDS filter table)
constexpr int kMultiPoints = 8 * kMultiWaves;         // output points per workgroup
constexpr int kBwdTWaves = 4;
constexpr int kBwdTPointsPerWG = 64;     // measured: 256 -> 1.90 ms, 128 -> 1.15, 64 -> 0.90, 32 -> 0.91, 16 -> 1.22 (tail / balance vs per-block setup)
constexpr int kBwdFillWG = 128;          // workgroups per XCD that a small level is spread over (compact kernel: 4 fit a CU)
constexpr int kCompactBins = 17;         // accumulator rows of the compact variant
// hub sources (dwconv_bwd_t_vec<..., HUB>): clouds of at least 32 768 points (measured: at 16 384 the two extra launches cost more
// than the few hubs of that level give back, profiles/r06_ab_conv_hub.log), sources with more than 1024 in-edges; kHubWG
// workgroups per channel slice in the hub launch
constexpr int kHubGroup = 8;
constexpr int kHubWG = 1024;             // workgroups of the hub launch (a multiple of kHubGroup) = slabs reserved for it
static_assert(kHubWG % kHubGroup == 0, "hub workgroups come in groups of kHubGroup");
constexpr long long kConvLds = 160 * 1024;            // LDS a workgroup can ask for

// op: the entry point (include/sph3d.h: SPH3D_CONV_*)
enum { kConvFwd = 0, kConvFwdCat = 1, kConvGradT = 2, kConvGradTCat = 3 };
// ConvPlan::kernel.  none: nothing is launched (forward: B == 0 or M == 0; gradient: B == 0, grad_filter is zero-filled) and
// every other field but workspace_bytes is 0; refused: SPH3D_EUNSUPPORTED (a two-input shape that is not covered; deterministic
// mode and only dwconv_bwd_t_generic, which sums with float atomics, fits), every other field is 0
enum { kConvNone = 0, kConvFwdMulti, kConvFwdRow, kConvFwdGeneric, kConvBwdVec, kConvBwdOdd, kConvBwdGeneric, kConvRefused };
// ConvPlan::bad: why the entry point answers SPH3D_EINVAL
enum { kConvOk = 0, kConvBadDims, kConvBadLds, kConvBadMultiplier, kConvBadGrid };

// persistent-sweep table of dwconv_bwd_t_vec / dwconv_bwd_t_odd: `parts` position ranges per cloud so that (cloud, part) items
// divide evenly over the 8 XCDs, W workgroups per XCD and channel slice, slabs = 8 W partial tables, one per workgroup of a slice
struct ConvTable {
    long long parts, W, slabs;
};

struct ConvPlan {           // (the order of sph3d_depthwise_conv3d_plan's output, up to `bad`)
    long long kernel;
    long long R;                        // depth multiplier
    long long LPE;                      // fwd_multi: lanes per edge, 16 (C <= 64) or 32
    long long V;                        // bwd_vec: channels per lane, 4 or 2; bwd_odd: T, 1 .. 4
    long long MAXF;                     // bwd_vec, bwd_odd: accumulator rows of the instantiation, 33 or 65
    long long PARTS;                    // bwd_vec: 1 full waves, 2 half waves, 4 quarter waves take alternate edges; bwd_odd: 1
    long long nslices;                  // channel slices
    long long compact_launch;           // bwd_vec: the compact-table sweep is launched in front of the full one
    long long hub, hub_threshold;       // bwd_vec: hub launches, and the in-edge count above which a source is a hub
    ConvTable full, compact;            // bwd_vec: 3 and 4 workgroups per CU; bwd_odd: full alone
    long long reduce_slabs, reduce_slabs_compact;       // what reduce_filter_partials is told: slabs of the full / compact table's run
    long long lds, grid;                // dynamic LDS bytes and workgroups of the main launch
    long long hub_list_offset;          // bwd_vec: bytes from the workspace's start to the hub list [count, b * N + n ...]
    long long workspace_bytes;          // gradient: slabs of F x C r partial filter gradients (+ the hub list)
    int bad;                            // (not reported)
};

// a * b for a, b >= 0, held at 2^62: the two products below that dimensions an int can hold may carry past 64 bits
constexpr long long kConvHuge = 1LL << 62;
static inline long long conv_mul(long long a, long long b) { return b != 0 && a > kConvHuge / b ? kConvHuge : a * b; }

// common.hpp's xcd_grid in 64 bits: workgroups of a launch that deals `parts` parts of each of B clouds to the XCDs (xcd_decode)
static inline long long conv_xcd_grid(long long B, long long parts)
{
    const int ls = B >= 5 ? 0 : (B >= 3 ? 1 : (B == 2 ? 2 : 3));
    const long long s = 1LL << ls, cpr = 8 >> ls;
    return conv_mul(8 * ((B + cpr - 1) / cpr), (parts + s - 1) >> ls);
}

//   * large levels: ~64 sources per workgroup (per-workgroup cost: one F x CR partial table), at most wg_per_cu per CU;
//   * small levels (N = 128..768: the whole launch is a few hundred sources per XCD): the kernel is a chain of
//     dependent gathers per source, so the sources are spread over enough workgroups to put two on every CU
//     (down to 2 sources per wave) instead of leaving most CUs idle.
static inline ConvTable conv_table(long long B, long long N, long long nslices, int wg_per_cu)
{
    ConvTable t;
    long long g = B & 7;                   // gcd(B, 8)
    g = g == 0 ? 8 : (g & -g);
    t.parts = 8 / g;
    if (t.parts > N) t.parts = 1;
    const long long items_per_xcd = (B * t.parts + 7) / 8;
    const long long src = items_per_xcd * ((N + t.parts - 1) / t.parts);
    const long long w_work = (src + kBwdTPointsPerWG - 1) / kBwdTPointsPerWG;
    long long w_fill = (wg_per_cu >= 4 ? kBwdFillWG : 64) / nslices;
    if (w_fill < 1) w_fill = 1;
    const long long w_min = (src + 2 * kBwdTWaves - 1) / (2 * kBwdTWaves);
    long long w = w_fill < w_min ? w_fill : w_min;
    if (w < w_work) w = w_work;
    const long long cap = 32LL * wg_per_cu;
    t.W = w < 1 ? 1 : (w > cap ? cap : w);
    t.slabs = 8 * t.W;
    return t;
}

// B, N, M, F, r, K as the entry point takes them (K: an entry that has none passes 1), Ca + Cb channels (Cb = 0: one
// input); deterministic: the mode; active_given: the gradient's active_bins is not NULL; hub_min_n, hub_threshold: the hub hooks'
// values (gradients with the mode off)
static inline ConvPlan conv_plan(int op, int B_, int N_, int M_, int F_, int Ca_, int Cb_, int r_, int K, bool deterministic,
                                 bool active_given, int hub_min_n, int hub_threshold)
{
    ConvPlan p = {};
    const bool grad = op == kConvGradT || op == kConvGradTCat, cat = op == kConvFwdCat || op == kConvGradTCat;
    const long long B = B_, N = N_, M = M_, F = F_, Ca = Ca_, Cb = Cb_, r = r_;         // (every product below: in 64 bits)
    const long long C = Ca + Cb, wide = 1LL << 32;
    auto ceil_div = [](long long a, long long b) { return (a + b - 1) / b; };
    // ---- what every entry point requires: dimensions, and an F x min(C r, 256) filter table slice in LDS (dwconv_fwd_generic's
    // and dwconv_bwd_t_generic's table; no kernel of either direction asks for less)
    // (C r: an int, as every kernel holds it)
    if (!(B >= 0 && N > 0 && M >= 0 && F > 0 && C > 0 && r > 0 && K > 0 && C * r <= 0x7fffffff)) { p.bad = kConvBadDims; return p; }
    const long long CR = C * r, slice = CR < kSlice ? CR : kSlice;
    if (F * slice * 4 > kConvLds) { p.bad = kConvBadLds; return p; }
    // ---- the rules the kernels set.  32-bit offsets: dwconv_fwd_multi forms byte offsets into a cloud's input and packs the
    // neighbour id into 24 bits and the bin into 8; dwconv_fwd_row forms element offsets into the input; the vector gradients
    // form element offsets into a cloud's grad_output rows
    const bool r12 = r == 1 || r == 2, fwd_vec = r12 && C % 4 == 0;
    const bool in_bytes_32 = N <= (1 << 24) && F <= 254 && N * C + 256 < wide / 4;            // N C 4 + 1024 < 2^32
    const bool in_elems_32 = N * C + 256 < wide, gout_elems_32 = M * CR + 256 < wide;
    const int V = !r12 ? 0 : (F <= 33 && CR % 4 == 0) ? 4 : (F <= 65 && CR % 2 == 0) ? 2 : 0;      // vector gradient: channels per lane
    // two inputs: every 256-output slice reads one tensor, four channels per lane and more than 128 outputs (the full-wave form)
    if (cat && !(Ca > 0 && Cb > 0 && fwd_vec && C > 128 && (Ca * r) % kSlice == 0 && V == 4 && (grad ? gout_elems_32 : in_elems_32))) {
        p.kernel = kConvRefused;
        return p;
    }
    p.R = r;
    if (!grad) {
        // the first of multi, row, generic whose shape conditions hold and whose table (multi, row: + the zero row of the padding
        // slots) fits LDS; two inputs: the row kernel (F <= 33 there: it fits)
        const long long lpe = C <= 64 ? 16 : 32;
        const long long multi_lds = fwd_vec ? (F + 1) * 4 * lpe * r * 4 : 0, row_lds = (F + 1) * slice * 4;
        if (!cat && fwd_vec && in_bytes_32 && C <= 128 && multi_lds <= kConvLds) {
            p.kernel = kConvFwdMulti;
            p.LPE = lpe;
            p.nslices = 1;
            p.lds = multi_lds;
            p.grid = conv_xcd_grid(B, ceil_div(M, kMultiPoints));
        } else {
            const bool row = fwd_vec && in_elems_32 && row_lds <= kConvLds;
            p.kernel = row ? kConvFwdRow : kConvFwdGeneric;
            p.nslices = ceil_div(CR, kSlice);
            p.lds = row ? row_lds : F * slice * 4;
            p.grid = conv_xcd_grid(B, ceil_div(M, kFwdPointsPerWG) * p.nslices);
        }
    } else if (V && gout_elems_32) {
        p.kernel = kConvBwdVec;
        p.V = V;
        p.MAXF = V == 4 ? 33 : 65;
        // rows of at most 128 (64) outputs: two half (four quarter) waves take alternate edges; a narrower row leaves lanes of
        // each part idle, but fewer than the full-wave form would (the ModelNet plan's 36-, 64- and 68-channel layers)
        p.PARTS = V == 2 ? 1 : (CR <= 64 ? 4 : (CR <= 128 ? 2 : 1));
        p.nslices = ceil_div(CR, 64 * V);
        // the compact launch exists for the 4-channels-per-lane plans (at most 33 bins: one register of segment bounds)
        p.compact_launch = active_given && V == 4;
        // big clouds: hub sources are left out of the sweep and shared among the waves of the hub launch (see the kernel)
        // (deterministic mode: never — the hub list is appended with an atomic and the hub launch adds its grad_input sums with float
        // atomics; the sweep alone takes every source, its static partition and reduce_filter_partials sum in a fixed order)
        p.hub = V == 4 && !deterministic && N >= hub_min_n;
        p.hub_threshold = p.hub ? hub_threshold : 0;
        // A call runs the full table's launches, the compact table's, or both (the device chooses, see the kernel); both write
        // slabs 0 .., so the slab area holds the larger of the two tables and the hub launch's kHubWG slabs behind either, then
        // the hub list.  Nothing of the workspace depends on the per-call switches: sized once, it serves every call of the shape
        p.full = conv_table(B, N, p.nslices, 3);
        p.compact = conv_table(B, N, p.nslices, 4);
        const long long hub_slabs = p.hub ? kHubWG : 0;
        p.reduce_slabs = p.full.slabs + hub_slabs;
        p.reduce_slabs_compact = (p.compact_launch ? p.compact.slabs : 0) + hub_slabs;
        p.lds = F * (CR < 64 * V ? CR : 64 * V) * 4;
        p.grid = p.full.slabs * p.nslices;
        p.hub_list_offset = 4 * ((p.full.slabs > p.compact.slabs ? p.full.slabs : p.compact.slabs) + kHubWG) * F * CR;
        p.workspace_bytes = p.hub_list_offset + conv_mul(4, B * N + 4);
    } else if (deterministic) {
        // odd row widths (dwconv_bwd_t_odd: r = 1 and odd C — with r in {1, 2} every other row width is even and has a vector
        // plan): T channels per lane, as many as the row needs, at most 4 (F <= 33) or 2 (F <= 65); wider rows take several slices
        // of 64 T channels.  The sweep is the full table's; the workspace is its slabs alone.  Anything else would sum with atomics
        if (!(r == 1 && C % 2 == 1 && F <= 65 && gout_elems_32)) {
            p = {};
            p.kernel = B > 0 ? kConvRefused : kConvNone;          // (B == 0: the zero fill alone, as in every mode)
            return p;
        }
        const long long tmax = F <= 33 ? 4 : 2, need = ceil_div(C, 64);
        p.kernel = kConvBwdOdd;
        p.V = need < tmax ? need : tmax;
        p.MAXF = F <= 33 ? 33 : 65;
        p.PARTS = 1;
        p.nslices = ceil_div(C, 64 * p.V);
        p.full = conv_table(B, N, p.nslices, 3);
        p.reduce_slabs = p.full.slabs;
        p.lds = F * 64 * p.V * 4;                 // [F][64 T]: at most 33 x 256 or 65 x 128 floats
        p.grid = p.full.slabs * p.nslices;
        p.workspace_bytes = 4 * p.full.slabs * F * C;
    } else {
        // generic (odd channel counts, other multipliers, F > 65): LDS float atomics, slow but general
        if (r > 256) { p = {}; p.bad = B > 0 ? kConvBadMultiplier : kConvOk; return p; }
        long long sliceC = 256 / r;
        if (sliceC > C) sliceC = C;
        p.kernel = kConvBwdGeneric;
        p.nslices = ceil_div(C, sliceC);
        p.lds = F * sliceC * r * 4;
        p.grid = conv_xcd_grid(B, ceil_div(N, 64) * p.nslices);
    }
    if (p.grid > 0x7fffffff) { p = {}; p.bad = kConvBadGrid; return p; }           // (a launch's workgroups: an int)
    if (B == 0 || (!grad && M == 0)) {
        const long long bytes = p.workspace_bytes;
        p = {};
        p.workspace_bytes = bytes;
    }
    return p;
}

}  // namespace sph3d
