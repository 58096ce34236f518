// conv3d.hip — depthwise spherical convolution (forward + gradients) for gfx950.
//
// Replaces depthwise_conv3d_forward / depthwise_input_backward / depthwise_filter_backward
// (tf_ops/convolution/tf_conv3d_gpu.cu:7-101) and their launchers (:107-140).
//
// MI355X design:
//   * One WAVEFRONT per output point (the reference: one thread per output CHANNEL, every
//     channel-thread re-reading the neighbour/bin lists and doing K read-modify-writes on global
//     memory).  The point's neighbour ids and bin ids are fetched ONCE as two coalesced 256-B reads (lane k
//     holds slot k) and broadcast lane->scalar with v_readlane eight at a time, so eight gather addresses are
//     scalar, eight feature-row gathers (each one coalesced wave read, float2/float4 per lane) and eight LDS
//     filter reads are in flight before the first FMA.
//   * Lanes span output channels, 4 consecutive channels per lane: accumulate in registers, one
//     coalesced float4 store per point.  A "slice" is 256 output channels; wider layers loop slices.
//   * The filter table slice (F x 256 floats = 33 KB at F=33) lives in LDS, read as ds_read_b128.
//   * Backward fuses both gradients in ONE pass over the TRANSPOSED graph (graph.hip): grad_input is a
//     gather (registers, one store per element, no float atomics to memory), grad_filter accumulates in
//     per-lane REGISTER tables (one row per bin, compile-time indexed: the transposed graph is sorted by
//     (source, bin)), summed across waves / workgroups at the end.  The reference scattered grad_input with
//     one global atomicAdd per (point, neighbour, channel) and re-ran the whole gather ceil(F*C*r/12288)
//     times for grad_filter (tf_conv3d_gpu.cu:51, 126-139).
//   * Workgroups of one cloud are dealt to one XCD (xcd_decode) so the cloud's feature rows
//     (N*C*4 B, 4 MiB at N=8192,C=128) stay in that XCD's 4 MiB L2.
//   * Numerics: sum_k in*filt in fp32 FMA order k = 0..cnt-1, one division by cnt at the end (the
//     reference divides every term); agreement with the oracle is ~1e-7 relative, bound 1e-5.
//   * The host decides nothing here: which kernel, which instantiation, grid, LDS bytes, sweep tables, hub and compact launches
//     and the workspace are conv_plan.hpp's conv_plan(), one pure function for the four ops (forward and transposed gradient,
//     over one input or two).  The entry points at the end of this file launch what it says; sph3d_depthwise_conv3d_plan
//     reports it.
#include <stddef.h>
#include <string.h>
#include <type_traits>
#include "common.hpp"
#include "conv_plan.hpp"

namespace sph3d {

constexpr int kFwdSB = 4;              // dwconv_fwd_multi: wave loads (each EPL neighbour rows) issued together
constexpr int kBatch = 8;               // dwconv_fwd_row: neighbours whose gathers are issued together

// ------------------------------------------------------------------------------------------
// forward, vectorised: R = depth multiplier (1 or 2), C % 4 == 0.
// A lane owns FOUR INPUT channels (one 16-B gather per edge) and their 4R output channels; an edge therefore needs
// LPE = C/4 lanes (16 / 32 / 64 for C = 64 / 128 / >= 256) and one wave load instruction fetches EPL = 64/LPE
// different neighbour rows, lane group g taking the edges k = g (mod EPL) of the point.  Round-1 counters that
// forced this shape (C = 128, r = 2, one edge per load, float2 per lane): the CU's vector L1 was 83 % occupied
// (59 % processing + 24 % stalled on pending lines) — the L1 spends 16 cycles per wave load whether the lanes ask
// for 8 or 16 bytes and whether or not half of them repeat lane 0's address; the L2 and HBM were far from busy.
// The group partial sums are added across lane groups at the end (ds_swizzle-free: two ds_bpermute rounds at most).
// ------------------------------------------------------------------------------------------
template <int R, int LPE, int SB>
__global__ __launch_bounds__(64 * kMultiWaves) void dwconv_fwd_multi(
    int B, int N, int M, int F, int C, int K, int mblocks, int nslices,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ binIndex,
    const float* __restrict__ input, const float* __restrict__ filter, float* __restrict__ output)
{
    extern __shared__ __attribute__((aligned(16))) float lfilt[];   // [F + 1][R][SLI]: compile-time strides
    constexpr int EPL = 64 / LPE;               // edges per wave load
    constexpr int NO = 4 * R;                   // output channels per lane
    constexpr int SLI = 4 * LPE;                // input channels per slice
    constexpr int FSTB = SLI * R * 4;           // bytes per filter row in LDS
    const int CR = C * R;
    int b, part;
    xcd_decode((int)blockIdx.x, B, mblocks * nslices, b, part);
    if (b < 0) return;
    const int slice = part / mblocks;
    const int mb = part - slice * mblocks;
    const int ci0 = slice * SLI;                                     // first input channel of the slice
    const int SLi = (C - ci0) < SLI ? (C - ci0) : SLI;               // multiple of 4
    const int SLo = SLi * R;

    // stage the filter slice, de-interleaved so that the lanes' 16-B reads are contiguous (conflict-free ds_read_b128):
    // quad q of lane li (its output channels 4q..4q+3, i.e. slice columns li*4R + 4q + j) lives at [f][q][li*4 + j]
    for (int e = threadIdx.x * 4; e < F * SLo; e += blockDim.x * 4) {
        const int f = e / SLo;
        const int cl = e - f * SLo;                 // multiple of 4
        const int l4 = cl / (4 * R), q = (cl >> 2) % R;
        *reinterpret_cast<float4*>(&lfilt[f * (SLI * R) + q * SLI + l4 * 4]) =
            *reinterpret_cast<const float4*>(&filter[(size_t)f * CR + ci0 * R + cl]);
    }
    // row F: all zeros, the filter row of padding slots (see dwconv_fwd_row)
    for (int e = threadIdx.x; e < SLI * R; e += blockDim.x) lfilt[F * (SLI * R) + e] = 0.f;
    __syncthreads();

    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int g = lane / LPE;                   // edge group of this lane
    const int li = lane - g * LPE;
    const bool act = li * 4 < SLi;
    const int cic = act ? li * 4 : 0;           // clamped copy for branch-free loads
    const int m_begin = mb * kMultiPoints;
    const int m_end = (m_begin + kMultiPoints) < M ? (m_begin + kMultiPoints) : M;
    // Instruction diet (round 3; the kernel is bound by instruction ISSUE, ~4.4 SIMD cycles per wave instruction, not by
    // bytes: profiles/r03_pmc_sq_*): uniform row base + 32-bit per-lane byte offsets (no 64-bit vector adds), ONE cross-lane
    // hand-over per edge (neighbour id and bin id packed in a word: id in the low 24 bits, so v_mul_u32_u24 turns the word
    // into the row's byte offset without masking it), the second filter quad at an immediate LDS offset, one reciprocal per
    // point instead of a correctly rounded division per output.
    const char* inb = reinterpret_cast<const char*>(input + (size_t)b * N * C + ci0);
    const unsigned cicb = (unsigned)cic * 4u;
    const unsigned rowb = (unsigned)C * 4u;     // bytes per input row (< 2^24: launcher)
    const char* lfb = reinterpret_cast<const char*>(lfilt);

    for (int m = m_begin + wave; m < m_end; m += kMultiWaves) {
        const size_t row = (size_t)b * M + m;
        const int cnt = uniform(nnCount[row]);
        float acc[NO];
#pragma unroll
        for (int v = 0; v < NO; v++) acc[v] = 0.f;
        for (int kt = 0; kt < cnt; kt += 64) {
            // the row's neighbour ids and bin ids: ONE coalesced 256-B read each (lane k holds slot kt + k) ...
            const int myk = kt + lane;
            const int kn = (cnt - kt) < 64 ? (cnt - kt) : 64;
            const int mykc = myk < cnt ? myk : kt;                 // padding lanes: the chunk's first neighbour times the zero row
            const int idxv = nnIndex[row * K + mykc];
            int binv = binIndex[row * K + mykc];
            binv = binv < 0 ? 0 : (binv >= F ? F - 1 : binv);     // out-of-range bin ids: same clamp as the transposed graph
            binv = myk < cnt ? binv : F;
            const unsigned pk = ((unsigned)idxv & 0xffffffu) | ((unsigned)binv << 24);      // N <= 2^24, F <= 254: launcher; an id outside [0, 2^24) must not reach the bin field
            static_assert(64 % (SB * EPL) == 0, "batches must tile the 64-edge chunk (no index clamps)");
            // ... then consumed SB wave loads (SB*EPL edges) at a time: all their gathers are in flight before the
            // first FMA (the kernel is latency-bound otherwise)
            for (int k0 = 0; k0 < kn; k0 += SB * EPL) {
                float4 x[SB];
                unsigned fo[SB];
#pragma unroll
                for (int u = 0; u < SB; u++) {
                    // lane group g takes edge k0 + u*EPL + g.  Measured: ds_bpermute (0.145 ms at C = 64) beats EPL v_readlane
                    // broadcasts + per-lane selects (0.203 ms)
                    const int kq = k0 + u * EPL + g;               // <= 63: padding slots hold a real row and the zero filter row
                    const unsigned p = (unsigned)__shfl((int)pk, kq);
                    const unsigned off = __umul24(p, rowb) + cicb;                 // low 24 bits of p = neighbour id
                    fo[u] = __umul24(p >> 24, (unsigned)FSTB) + cicb;
                    x[u] = *reinterpret_cast<const float4*>(inb + off);
                }
#pragma unroll
                for (int u = 0; u < SB; u++) {
                    const float xs[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                    for (int q = 0; q < R; q++) {
                        const float4 w = *reinterpret_cast<const float4*>(lfb + fo[u] + q * (SLI * 4));
                        // outputs 4q..4q+3 of this lane belong to input channels (4q + j) / R
                        acc[4 * q + 0] = fmaf(xs[(4 * q + 0) / R], w.x, acc[4 * q + 0]);
                        acc[4 * q + 1] = fmaf(xs[(4 * q + 1) / R], w.y, acc[4 * q + 1]);
                        acc[4 * q + 2] = fmaf(xs[(4 * q + 2) / R], w.z, acc[4 * q + 2]);
                        acc[4 * q + 3] = fmaf(xs[(4 * q + 3) / R], w.w, acc[4 * q + 3]);
                    }
                }
            }
        }
        // add the partial sums of the EPL lane groups (lanes li, li + LPE, ...)
#pragma unroll
        for (int o = LPE; o < 64; o <<= 1)
#pragma unroll
            for (int v = 0; v < NO; v++) acc[v] += __shfl_xor(acc[v], o);
        if (act && g == 0) {
            // cnt == 0 only for rows the caller marked empty: output 0.  One reciprocal per point (1 ulp from the per-term
            // divisions of the reference; the bound on the op is 1e-5)
            const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;
            float* op = &output[row * CR + (size_t)(ci0 + li * 4) * R];
#pragma unroll
            for (int q = 0; q < R; q++) {
                float4 o;
                o.x = acc[4 * q + 0] * inv;
                o.y = acc[4 * q + 1] * inv;
                o.z = acc[4 * q + 2] * inv;
                o.w = acc[4 * q + 3] * inv;
                *reinterpret_cast<float4*>(&op[4 * q]) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// forward, one edge per wave load (C >= 128): R = depth multiplier (1 or 2), CR % 4 == 0
// ------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void dwconv_fwd_row(
    int B, int N, int M, int F, int C, int K, int mblocks, int nslices,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ binIndex,
    const float* __restrict__ input, const float* __restrict__ filter, float* __restrict__ output,
    const float* __restrict__ input2 = nullptr, int Ca = 0)
{
    extern __shared__ __attribute__((aligned(16))) float lfilt[];   // [F][SL]
    const int CR = C * R;
    int b, part;
    xcd_decode((int)blockIdx.x, B, mblocks * nslices, b, part);
    if (b < 0) return;
    const int slice = part / mblocks;
    const int mb = part - slice * mblocks;
    const int slice0 = slice * kSlice;
    const int SL = (CR - slice0) < kSlice ? (CR - slice0) : kSlice;   // multiple of 4

    // stage the filter slice: lfilt[f][cl] = filter[f*CR + slice0 + cl]
    for (int e = threadIdx.x * 4; e < F * SL; e += blockDim.x * 4) {
        const int f = e / SL;
        const int cl = e - f * SL;
        *reinterpret_cast<float4*>(&lfilt[e]) = *reinterpret_cast<const float4*>(&filter[(size_t)f * CR + slice0 + cl]);
    }
    // row F: all zeros — the filter row of padding slots (batches of eight run past the neighbour count without clamps or
    // conditional FMAs: a padding slot multiplies the row's FIRST neighbour by exactly 0)
    for (int e = threadIdx.x; e < SL; e += blockDim.x) lfilt[F * SL + e] = 0.f;
    __syncthreads();

    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int cl0 = lane * 4;
    const bool act = cl0 < SL;
    const int cin0 = (slice0 + cl0) / R;      // first input channel of this lane
    const int clc = act ? cl0 : 0;            // clamped copies for branch-free loads
    const int cinc = act ? cin0 : slice0 / R;
    const int m_begin = mb * kFwdPointsPerWG;
    const int m_end = (m_begin + kFwdPointsPerWG) < M ? (m_begin + kFwdPointsPerWG) : M;
    // input2 != nullptr: the input is the channel concatenation [input (Ca channels) | input2 (C - Ca)] of two tensors that were
    // never concatenated (sph3d_depthwise_conv3d_cat: a decoder level's un-pooled features and the encoder's skip features).
    // The launcher guarantees that a 256-output slice lies inside ONE of them, so the choice is per workgroup: a base
    // pointer, a row stride and a channel shift.
    const bool second = input2 != nullptr && (slice0 / R) >= Ca;
    const int Cs = input2 == nullptr ? C : (second ? C - Ca : Ca);       // row stride of the source tensor
    const int cshift = second ? Ca : 0;
    const float* inb = (second ? input2 : input) + (size_t)b * N * Cs - cshift;

    // (measured in round 1 and dropped: visiting the output points in Morton order: no gain, the rows come from L2 either way,
    // profiles/)
    for (int m = m_begin + wave; m < m_end; m += 4) {
        const size_t row = (size_t)b * M + m;
        const int cnt = uniform(nnCount[row]);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int kt = 0; kt < cnt; kt += 64) {
            // the row's neighbour ids and bin ids: ONE coalesced 256-B read each (lane k holds slot kt + k) ...
            const int myk = kt + lane;
            const int kn = (cnt - kt) < 64 ? (cnt - kt) : 64;
            const int mykc = myk < cnt ? myk : kt;                 // padding lanes: the chunk's first neighbour (a real one) ...
            const int idxv = nnIndex[row * K + mykc];
            int binv = binIndex[row * K + mykc];
            binv = binv < 0 ? 0 : (binv >= F ? F - 1 : binv);     // out-of-range bin ids: same clamp as the transposed graph
            binv = myk < cnt ? binv : F;                           // ... times the zero row
            // element offsets of the input row and of the filter row, once per 64 edges (N * C < 2^32: checked by the launcher)
            const unsigned noff = (unsigned)idxv * (unsigned)Cs;
            const int foff = binv * (SL >> 2);                     // in float4 units: keeps the LDS read a 16-byte aligned ds_read_b128
            // ... then consumed eight at a time: 8 lane->scalar broadcasts, 8 independent row gathers and 8 filter
            // reads are in flight before the first FMA (the kernel is latency-bound otherwise).  kBatch divides 64, so
            // k8 + u <= 63: no clamp
            for (int k8 = 0; k8 < kn; k8 += kBatch) {
                unsigned n[kBatch];
                int f[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    n[u] = (unsigned)__builtin_amdgcn_readlane((int)noff, k8 + u);
                    f[u] = __builtin_amdgcn_readlane(foff, k8 + u);
                }
                float4 w[kBatch];
                float4 x[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    // no per-lane branch here: inactive lanes (slices narrower than 256) read lane 0's columns, so the
                    // eight loads stay in one basic block and are all in flight together
                    w[u] = reinterpret_cast<const float4*>(lfilt)[f[u] + (clc >> 2)];
                    const float* __restrict__ rp = inb + n[u];          // wave-uniform row address (scalar registers)
                    if (R == 2) {
                        const float2 t = *reinterpret_cast<const float2*>(&rp[(unsigned)cinc]);
                        x[u] = make_float4(t.x, t.x, t.y, t.y);
                    } else {
                        x[u] = *reinterpret_cast<const float4*>(&rp[(unsigned)cinc]);
                    }
                }
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    acc.x = fmaf(x[u].x, w[u].x, acc.x);
                    acc.y = fmaf(x[u].y, w[u].y, acc.y);
                    acc.z = fmaf(x[u].z, w[u].z, acc.z);
                    acc.w = fmaf(x[u].w, w[u].w, acc.w);
                }
            }
        }
        if (act) {
            // cnt == 0 only for rows the caller marked empty: output 0.  One reciprocal per point, not a correctly rounded
            // division per output (4 x ~11 instructions per lane and point on an issue-bound kernel)
            const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;
            float4 o;
            o.x = acc.x * inv;
            o.y = acc.y * inv;
            o.z = acc.z * inv;
            o.w = acc.w * inv;
            *reinterpret_cast<float4*>(&output[row * CR + slice0 + cl0]) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------
// forward, generic: any C, r (odd channel counts of the ModelNet plan: C = 35, 67, 131)
// lane owns output channels slice0 + lane + 64*t, t < 4
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dwconv_fwd_generic(
    int B, int N, int M, int F, int C, int r, int K, int mblocks, int nslices,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ binIndex,
    const float* __restrict__ input, const float* __restrict__ filter, float* __restrict__ output)
{
    extern __shared__ __attribute__((aligned(16))) float lfilt[];   // [F][SL]
    const int CR = C * r;
    int b, part;
    xcd_decode((int)blockIdx.x, B, mblocks * nslices, b, part);
    if (b < 0) return;
    const int slice = part / mblocks;
    const int mb = part - slice * mblocks;
    const int slice0 = slice * kSlice;
    const int SL = (CR - slice0) < kSlice ? (CR - slice0) : kSlice;

    for (int e = threadIdx.x; e < F * SL; e += blockDim.x) {
        const int f = e / SL;
        const int cl = e - f * SL;
        lfilt[e] = filter[(size_t)f * CR + slice0 + cl];
    }
    __syncthreads();

    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    int cl[4], cin[4];
    bool act[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        cl[t] = lane + 64 * t;
        act[t] = cl[t] < SL;
        cin[t] = act[t] ? (slice0 + cl[t]) / r : 0;
        if (!act[t]) cl[t] = 0;
    }
    const int m_begin = mb * kFwdPointsPerWG;
    const int m_end = (m_begin + kFwdPointsPerWG) < M ? (m_begin + kFwdPointsPerWG) : M;
    const float* inb = input + (size_t)b * N * C;

    for (int m = m_begin + wave; m < m_end; m += 4) {
        const size_t row = (size_t)b * M + m;
        const int cnt = uniform(nnCount[row]);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const int* __restrict__ irow = nnIndex + row * K;   // wave-uniform address -> scalar loads
        const int* __restrict__ brow = binIndex + row * K;
        {
#pragma unroll 4
            for (int kk = 0; kk < cnt; kk++) {
                const int n = irow[kk];
                int f = brow[kk];
                f = f < 0 ? 0 : (f >= F ? F - 1 : f);
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const float x = inb[(size_t)n * C + cin[t]];
                    const float w = lfilt[f * SL + cl[t]];
                    acc[t] = fmaf(x, w, acc[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (act[t]) output[row * CR + slice0 + cl[t]] = cnt > 0 ? acc[t] / (float)cnt : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------
// backward over the TRANSPOSED graph (graph.hip): one wave per source point n, NO float atomics in the loop.
// Per in-edge (m, scale) of segment (n, f): one coalesced gather of grad_out[b,m, V channels/lane]; per segment one
// LDS read of the filter row; with g = grad_out * scale (scale = 1/nn_count[m]):
//     grad_in[b,n,c]     += sum_rho g * filt[f,c,rho]     registers, stored once per element
//     grad_filt[f,c,rho] += g * in[b,n,c]                 REGISTERS: every lane keeps a private [MAXF][V]
//                                                         accumulator; the transposed graph is sorted by
//                                                         (n, bin), so the kernel walks the F segments of a
//                                                         source in a fully unrolled loop: acc[f] is a fixed
//                                                         register, the filter row is read once per segment
//                                                         ("gather / segment-sum").
// Round-1 measurement that forced this shape: the same loop with the table in LDS updated by ds_add_f32
// ran 12.4 ms at (B=16, N=8192, C=128, r=2); without those LDS float atomics 1.4 ms — ds_add_f32 retires
// roughly one LANE per 4 cycles on gfx950.  Global fp32 atomics (the reference's scheme) were 9.0 ms.
// At the end the 4 waves of a workgroup sum their accumulators through LDS with plain reads/writes (taking
// turns), and the workgroup writes ONE partial table to a workspace slab; reduce_filter_partials adds the slabs.
// V = channels per lane: 4 for F <= 33 (the [8,2,2] and [8,2,1] kernels), 2 for F <= 65 ([8,2,3] = 49 bins).
// Edges are consumed four at a time: four scalar key loads and four independent row gathers are issued before
// any is used (memory-level parallelism; the kernel is latency-bound at 2 waves/SIMD otherwise).
// ------------------------------------------------------------------------------------------

constexpr int kBwdNL2 = 3;     // wave loads per batch of the half-wave form (2 edges per load)
constexpr int kBwdNL4 = 2;     // ... of the quarter-wave form (4 edges per load)
// PARTS = 2 (CR <= 128, V == 4): a grad_out row is at most 32 lanes wide, so the two halves of the wave take ALTERNATE edges of
// a segment (one wave load = two rows) and keep separate partial sums, added across the halves once per source
// (grad_input) / once per launch (the filter accumulators).  PARTS = 4 (CR <= 64): four quarter waves, four rows per load
// (the ModelNet plan's 64-output layers: half of the lanes idle otherwise).
// COMPACT: the accumulator table has one row per ACTIVE bin of the graph (active_bins = [count, ascending list], written by
// sph3d_graph_transpose): with the reference's sqrt-distance quirk the inner radial shell is empty at small radii
// (SURVEY §0.5), so at S3DIS levels 0-2 only 17 of the 33 bins ever occur: 68 accumulator VGPRs instead of 132, four
// workgroups per CU instead of three, and a 17- instead of 33-iteration segment loop.  The host cannot know the count
// without a device->host sync, so BOTH variants are launched and each returns at once unless the count is in its range.
// HUB (round 6, clouds of 32 768 points and more): on one 65 536-point cloud the first-K rule gives a few hundred low-index sources
// thousands of in-edges each (p99 1235, maximum 11 146), and a source is one wave's sequential walk: the launch took as long as its
// biggest hub (1.4 ms at level 0 of the ScanNet-shape plan for 4.2 M edge slots; the 16 x 8192 batch with twice the edges: 0.42).
//   HUB = 1: this kernel, but a source with more than hubT in-edges is not walked: its grad_input row is zeroed and (slice 0)
//            its id appended to hubList = [count, b * N + n ...];
//   HUB = 2: the hub kernel, launched behind it on the same stream: hubW workgroups per slice; kHubGroup workgroups share a listed
//            source, their 4 x kHubGroup waves take every (4 kHubGroup)-th 64-edge chunk of it (the chunk loop clips segments to a
//            chunk anyway), add their grad_input partial sums with float atomics (order not fixed — as the order of a segment's
//            entries already is not) and keep the filter gradient in their accumulators like every other wave: slabs
//            slabBase .. slabBase + hubW - 1 of `partial`.
//   HUB = 0 (every other launch, the headline's among them): neither.
template <int R, int V, int MAXF, int PARTS, bool COMPACT, int HUB = 0>
__global__ __launch_bounds__(kBwdTWaves * 64, COMPACT ? 4 : 3) void dwconv_bwd_t_vec(
    int B, int N, int M, int F, int C, int W, int parts, int nslices,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const float* __restrict__ entScale,
    const int* __restrict__ order, const int* __restrict__ activeBins, int compactMax,
    const float* __restrict__ input, const float* __restrict__ filter, const float* __restrict__ gradOutput,
    float* __restrict__ gradInput, float* __restrict__ partial,
    const float* __restrict__ input2 = nullptr, float* __restrict__ gradInput2 = nullptr, int Ca = 0,
    int* __restrict__ hubList = nullptr, int hubT = 0, int slabBase = 0)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SLW = 64 * V;                 // slice width in output channels
    constexpr int VI = (V >= R) ? V / R : 1;    // input channels per lane
    const int CR = C * R;
    // which of the two launches does the work (wave-uniform, decided from device memory: no host sync)
    const int A = activeBins ? uniform(activeBins[0]) : F;
    if (COMPACT ? (A > MAXF) : (activeBins != nullptr && A <= compactMax)) return;
    // persistent workgroups: W per XCD and channel slice, all resident together (launch bounds: 3 or 4 per CU)
    // (HUB == 2: W workgroups per slice in all, numbered w = 0 .. W - 1; xcd is not used)
    const int xcd = HUB == 2 ? 0 : ((int)blockIdx.x & 7);
    const int q = HUB == 2 ? (int)blockIdx.x : ((int)blockIdx.x >> 3);
    const int slice = q / W;
    const int w = q - slice * W;
    const int slice0 = slice * SLW;
    const int SL = (CR - slice0) < SLW ? (CR - slice0) : SLW;     // multiple of V
    float* lfilt = lds;                                           // [F][SL]
    // input2 != nullptr: input / gradInput are the two halves [Ca | C - Ca] of a channel concatenation that was never made
    // (sph3d_depthwise_conv3d_grad_t_cat); a slice lies inside one of them (launcher), so the choice is per workgroup
    const bool second = input2 != nullptr && (slice0 / R) >= Ca;
    const int Cs = input2 == nullptr ? C : (second ? C - Ca : Ca);
    const float* __restrict__ xin = (second ? input2 : input) - (second ? Ca : 0);
    float* __restrict__ gin = (second ? gradInput2 : gradInput) - (second ? Ca : 0);

    for (int e = threadIdx.x * V; e < F * SL; e += blockDim.x * V) {
        const int f = e / SL;
        const int cl = e - f * SL;
#pragma unroll
        for (int v = 0; v < V; v++) lfilt[e + v] = filter[(size_t)f * CR + slice0 + cl + v];
    }
    __syncthreads();

    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int stride = W * kBwdTWaves;          // waves of this XCD that sweep a cloud side by side
    constexpr bool HALF = PARTS > 1;                              // the wave is split into PARTS groups of 64 / PARTS lanes
    constexpr int PL = 64 / PARTS;                                // lanes per group = row width / V
    const int half = HALF ? (lane / PL) : 0;                      // the lane's group
    const int cl0 = (HALF ? (lane % PL) : lane) * V;
    const bool act = cl0 < SL;
    const int cin0 = (slice0 + cl0) / R;
    // per-lane gradient-of-filter accumulators, one row per bin; every index below is a compile-time constant
    // (the bin loop is fully unrolled), so the table lives in VGPRs
    float acc[MAXF][V];
#pragma unroll
    for (int i = 0; i < MAXF; i++)
#pragma unroll
        for (int v = 0; v < V; v++) acc[i][v] = 0.f;

    // COMPACT: lane i holds the bin of accumulator row i (one load for the whole launch; the per-segment scalar load of
    // activeBins[1 + fi] was not hoisted by the compiler and put an s_load + lgkmcnt(0) in front of every segment)
    // (lanes >= A read entry 1, never past the A + 1 ints the list holds: the caller's tensor is F + 1 ints and F may be < MAXF)
    const int abv = COMPACT ? activeBins[1 + ((lane < MAXF && lane < A) ? lane : 0)] : 0;

    // Work items of this XCD: (cloud, part) pairs dealt round-robin; a part is a contiguous range of POSITIONS in the
    // processing order (source_order, or the point index).  Wave gw visits positions gw, gw + stride, ...; the
    // accumulators live across ALL items, so a workgroup writes one partial table for the whole launch.
    // (Measured round 2 and dropped: handing the positions out dynamically through one ticket counter per item.  The
    // static interleave leaves the busiest wave of an XCD with 1.4x the mean number of in-edges — the in-degree is
    // heavy-tailed: level 0 mean 48, sigma 45, max 537, tools/exp_bwd_balance.py — but with tickets of 4 or 8 positions
    // the level-0 kernels ran 0.66 / 0.55 ms against 0.53 / 0.35 ms, with or without waiting for the atomic at once.)
    // (Also dropped: the four waves of a workgroup taking the workgroup's positions from an LDS counter — the extra live
    // scalars of the flattened (item, position) loop pushed the kernel from 119 VGPRs to 128 + 232 B of scratch: 1.16 ms.)
    const int nhub = HUB == 2 ? uniform(hubList[0]) : 0;
    for (int item = HUB == 2 ? w / kHubGroup : xcd; HUB == 2 ? item < nhub : item < B * parts; item += HUB == 2 ? W / kHubGroup : 8) {
    const int hubSrc = HUB == 2 ? uniform(hubList[1 + item]) : 0;
    const int b = HUB == 2 ? hubSrc / N : item / parts;
    const int pi = HUB == 2 ? 0 : item - b * parts;
    // part pi = the positions pi, pi + parts, ... (parts > 1 only when B is not a multiple of 8).  Interleaved, not contiguous
    // ranges: on ONE 65 536-point cloud the first-K rule gives the low indices nearly all in-edges (median in-degree 4, p99
    // 1235, maximum 11 146), and a contiguous first eighth put them all on one XCD
    // wave-uniform base of this cloud's grad_out rows + the lane's column: row gathers are uniform base + uniform row
    // offset (an SGPR pair) + one loop-invariant 32-bit lane offset
    const float* __restrict__ gou = gradOutput + (size_t)b * M * CR + slice0;
    const unsigned cla = (unsigned)(act ? cl0 : 0);
    const int* __restrict__ offb = offsets + (size_t)b * ((size_t)N * F + 1);
    // The index chain of a source — position -> order[] -> n -> bounds row and [E0, E1) -> the first 64 keys -> gathers — is three
    // dependent round trips that move no payload, and everything in it is known before the source in front has begun.  So
    // (HUB < 2) it runs ahead of the walk: at the top of the body for position p the wave issues order[] for p + 3 steps, E0 / E1
    // for p + 2 steps (scalar loads: SGPRs only), and the bounds row and the first key chunk for p + 1 step (one VGPR each, two
    // for the bounds where MAXF >= 64); the walk of p hides them.  Which wave takes which source and the order of every sum are
    // untouched.  A position past the cloud's end stands for position N - 1, whose index data is in range and read for nothing.
    const int pstep = HUB == 2 ? 1 : parts * stride;
    const int pfirst = HUB == 2 ? 0 : pi + parts * (w * kBwdTWaves + wave);
    if (HUB != 2 && pfirst >= N) continue;
    auto src_at = [&](int q) {
        const int qc = q < N ? q : N - 1;
        return order ? uniform(order[(size_t)b * N + qc]) : qc;
    };
    // the source's F+1 segment bounds: ONE coalesced read (lane f holds bound f), consumed with v_readlane at
    // compile-time lanes — not 33 dependent scalar loads (measured: they dominated the sparse levels)
    // (here and below: a wave-uniform row pointer indexed with an unsigned lane offset — an SGPR pair + one 32-bit VGPR per load.
    // lane_offset() hides the offset from loop-invariant code motion, which otherwise adds it to the cloud's base pointer once
    // per item and keeps that 64-bit per-lane address in two VGPRs through the whole walk: there is no room for them)
    auto lane_offset = [](int i) {
        unsigned u = (unsigned)i;
        asm volatile("" : "+v"(u));
        return u;
    };
    auto bounds0 = [&](int nn) { return (offb + (size_t)nn * F)[lane_offset(lane <= F ? lane : F)]; };
    auto bounds1 = [&](int nn) { return (MAXF >= 64) ? (offb + (size_t)nn * F)[lane_offset((64 + lane) <= F ? (64 + lane) : F)] : 0; };
    // the first min(64, E1 - E0) keys of a source, lanes past them clamped to the first; a source without in-edges reads nothing
    auto keys0 = [&](int e0, int e1) {
        const int c = (e1 - e0) < 64 ? (e1 - e0) : 64;
        return e1 > e0 ? (entKey + e0)[(unsigned)(lane < c ? lane : 0)] : 0;
    };
    int n1 = 0, n2 = 0, n3 = 0, E0n = 0, E1n = 0, E0nn = 0, E1nn = 0, ovn0 = 0, ovn1 = 0, wkn = 0;
    if (HUB != 2) {
        n1 = src_at(pfirst);
        n2 = src_at(pfirst + pstep);
        n3 = src_at(pfirst + 2 * pstep);
        E0n = uniform(offb[(size_t)n1 * F]);
        E1n = uniform(offb[(size_t)n1 * F + F]);
        E0nn = uniform(offb[(size_t)n2 * F]);
        E1nn = uniform(offb[(size_t)n2 * F + F]);
        ovn0 = bounds0(n1);
        ovn1 = bounds1(n1);
        wkn = keys0(E0n, E1n);
    }
    for (int p = pfirst; HUB == 2 ? p < 1 : p < N; p += pstep) {
        int n, ov0, ov1, E0, E1, wkey0 = 0;
        if (HUB == 2) {
            n = hubSrc - b * N;
            ov0 = bounds0(n);
            ov1 = bounds1(n);
            E0 = __builtin_amdgcn_readlane(ov0, 0);
            E1 = uniform(offb[(size_t)n * F + F]);
        } else {
            // this source's index data arrived under the walk of the one before; the next ones' loads go out now
            n = n1, ov0 = ovn0, ov1 = ovn1, E0 = E0n, E1 = E1n, wkey0 = wkn;
            n1 = n2, n2 = n3, E0n = E0nn, E1n = E1nn;
            n3 = src_at(p + 3 * pstep);
            E0nn = uniform(offb[(size_t)n2 * F]);
            E1nn = uniform(offb[(size_t)n2 * F + F]);
            ovn0 = bounds0(n1);
            ovn1 = bounds1(n1);
            wkn = keys0(E0n, E1n);
        }
        float xi[VI], xv[V];
#pragma unroll
        for (int u = 0; u < VI; u++) xi[u] = (xin + ((size_t)b * N + n) * Cs)[lane_offset(act ? cin0 : slice0 / R) + u];
#pragma unroll
        for (int v = 0; v < V; v++) xv[v] = xi[(V >= R) ? v / R : 0];
        float gi[V];
#pragma unroll
        for (int v = 0; v < V; v++) gi[v] = 0.f;
        // The source's in-edges are one contiguous run [E0, E1) of the (source, bin)-sorted entry arrays.  Their keys
        // and scales are fetched 64 at a time with ONE coalesced vector load each (lane = edge) and handed to the
        // gathers with v_readlane.  Round 2 counters on the scalar version of this loop (s_load of key and scale per
        // edge, 64-bit scalar address arithmetic, clamps): 16.8 scalar-ALU + 2.7 scalar-memory instructions per edge =
        // half of the CU's one-per-cycle scalar issue for the whole kernel, and a dependent s_load -> gather round
        // trip per batch of four edges.
        // COMPACT: which accumulator rows have a non-empty segment at this source (about half of the 17 do not): one mask per
        // source instead of two v_readlane + clamps + compare per empty segment
        unsigned long long nonempty = ~0ull;
        if (COMPACT) {
            const int fl = lane < MAXF ? abv : 0;
            const int s0 = __builtin_amdgcn_ds_bpermute(fl << 2, ov0);
            const int s1 = __builtin_amdgcn_ds_bpermute((fl + 1) << 2, ov0);
            // (rows past the A-th folded in here: `fi < A` per row kept 17 hoisted wave masks alive through the whole walk)
            nonempty = __ballot(s1 > s0 && lane < A);
        }
        if (HUB == 1 && (E1 - E0) > hubT) {
            // a hub: left to the hub kernel (every slice's wave decides the same from the degree alone; the list holds each source once)
            if (slice == 0 && lane == 0) hubList[1 + atomicAdd(&hubList[0], 1)] = b * N + n;
            if (act && half == 0 && V >= R) {
                float* gp = &gin[((size_t)b * N + n) * Cs + cin0];
#pragma unroll
                for (int u = 0; u < VI; u++) gp[u] = 0.f;
            }
            continue;
        }
        const int cfirst = HUB == 2 ? E0 + 64 * ((w % kHubGroup) * kBwdTWaves + wave) : E0;
        const int cstep = HUB == 2 ? 64 * kHubGroup * kBwdTWaves : 64;
        // the chunk at cb: its edge count, row offsets and scales; the first chunk's keys came with the prefetch (HUB < 2), a later
        // chunk's are loaded at the foot of the loop
        int cb = cfirst, cn = 0;
        unsigned kel = 0u;
        float sv = 0.f;
        auto take_chunk = [&](bool prefetched) {
            cn = (E1 - cb) < 64 ? (E1 - cb) : 64;
            const int li = lane < cn ? lane : 0;
            // (entScale == NULL: packed entries, common.hpp: row and count in one word, 1 / count divided here: once per lane and chunk)
            const int wkey = prefetched ? wkey0 : (entKey + cb)[(unsigned)li];
            kel = (unsigned)tg_key(wkey, entScale == nullptr) * (unsigned)CR;     // row offset in floats (M * CR < 2^32, checked by the launcher)
            const float svl = entScale == nullptr ? tg_packed_scale(wkey) : (entScale + cb)[(unsigned)li];
            sv = lane < cn ? svl : 0.f;
        };
        if (cb < E1) take_chunk(HUB != 2);
        while (cb < E1) {
#pragma unroll
        for (int fi = 0; fi < MAXF; fi++) {
            // the mask exists for the compact table only (MAXF <= 64 there); the full table of the V = 2 plan has MAXF = 65 and a
            // shift by 64 would be undefined — and let the compiler drop bin 64 altogether
            if (COMPACT ? ((nonempty >> (fi & 63)) & 1ull) != 0ull : fi < F) {
                // COMPACT: row fi of the accumulators belongs to bin activeBins[1 + fi] (wave-uniform, F <= 63)
                const int f = COMPACT ? __builtin_amdgcn_readlane(abv, fi) : fi;
                const int a0 = COMPACT ? __builtin_amdgcn_readlane(ov0, f)
                                       : __builtin_amdgcn_readlane(fi < 64 ? ov0 : ov1, fi & 63);
                const int a1 = COMPACT ? __builtin_amdgcn_readlane(ov0, f + 1)
                                       : __builtin_amdgcn_readlane((fi + 1) < 64 ? ov0 : ov1, (fi + 1) & 63);
                // the part of the segment inside this chunk, as lane numbers
                const int e0 = (a0 > cb ? a0 : cb) - cb;
                const int e1 = (a1 < cb + cn ? a1 : cb + cn) - cb;
                if (e0 < e1) {                               // wave-uniform: most (n, bin) segments are empty or short
                    float sg[V];
#pragma unroll
                    for (int v = 0; v < V; v++) sg[v] = 0.f;
                    // the segment's filter row is read from LDS now, under the gathers, not after them
                    float wr[V];
                    {
                        const float* wrow = &lfilt[f * SL + (act ? cl0 : 0)];
#pragma unroll
                        for (int v = 0; v < V; v++) wr[v] = wrow[v];
                    }
                    if (HALF) {
                        // the two half-waves take alternate edges: lane-half h reads edge e + 2u + h of the chunk through
                        // ds_bpermute (lane number modulo 64, scales masked to the segment: see the full-wave branch)
                        constexpr int NL = PARTS == 2 ? kBwdNL2 : kBwdNL4;          // wave loads per batch = PARTS * NL edges
                        const float svh = ((unsigned)(lane - e0) < (unsigned)(e1 - e0)) ? sv : 0.f;
                        // (exact-count last batches, which pay in the full-wave branch, measured no gain here: 0.305 vs 0.319 ms)
                        // a batch that runs past lane 63 wraps (ds_bpermute takes the lane modulo 64) onto lanes 0.. of the chunk, which
                        // belong to the segment when it is (nearly) the whole chunk: impossible while the batch divides 64 (4 and 8
                        // edges), masked by the edge number in that one batch otherwise (6 edges: segments of 61+ in-edges)
#define SPH3D_BWD_HALF_BATCH(WRAPS)                                                                                  \
    {                                                                                                                \
        const int a4 = ((e + half) << 2);                                                                            \
        unsigned ko[NL];                                                                                             \
        float sc[NL];                                                                                                \
        _Pragma("unroll") for (int u = 0; u < NL; u++) {                                                             \
            ko[u] = (unsigned)__builtin_amdgcn_ds_bpermute(a4 + 4 * PARTS * u, (int)kel);                            \
            sc[u] = __int_as_float(__builtin_amdgcn_ds_bpermute(a4 + 4 * PARTS * u, __float_as_int(svh)));           \
            if (WRAPS) sc[u] = (e + half + PARTS * u) < 64 ? sc[u] : 0.f;                                            \
        }                                                                                                            \
        float g[NL][V];                                                                                              \
        _Pragma("unroll") for (int u = 0; u < NL; u++) {                                                             \
            const float4 t = *reinterpret_cast<const float4*>(&gou[ko[u] + cla]);                                    \
            g[u][0] = t.x; g[u][1 % V] = t.y; g[u][2 % V] = t.z; g[u][3 % V] = t.w;                                  \
        }                                                                                                            \
        _Pragma("unroll") for (int u = 0; u < NL; u++)                                                               \
            _Pragma("unroll") for (int v = 0; v < V; v++) sg[v] = fmaf(g[u][v], sc[u], sg[v]);                       \
    }
                        for (int e = e0; e < e1; e += PARTS * NL) {
                            if ((64 % (PARTS * NL)) != 0 && e + PARTS * NL > 64) SPH3D_BWD_HALF_BATCH(true)
                            else SPH3D_BWD_HALF_BATCH(false)
                        }
#undef SPH3D_BWD_HALF_BATCH
                    } else {
                    // scales of THIS segment's lanes, zero elsewhere.  The batches below read lanes e0 .. e1 - 1 only (four at a
                    // time, then the exact remainder), so no row outside the segment is gathered and the mask changes nothing
                    // here: unlike the half- and quarter-wave batches above, this branch never multiplies a foreign row by 0
                    // (a non-finite grad_out row reaches the segments it belongs to and no other: include/sph3d.h)
                    const float svm = ((unsigned)(lane - e0) < (unsigned)(e1 - e0)) ? sv : 0.f;
                    // four edges at a time (their row gathers are independent and issued together), then the segment's last one
                    // to three edges with exactly that many gathers: a padded last batch made a third of all gathers padding
                    // (8.5 M wave loads for 6.3 M edges at level 0), and these kernels pay 16 L1 cycles per wave load
#define SPH3D_BWD_BATCH(NB)                                                                                          \
    {                                                                                                                \
        float sc[NB];                                                                                                \
        float g[NB][V];                                                                                              \
        _Pragma("unroll") for (int u = 0; u < NB; u++) {                                                             \
            const unsigned ko = (unsigned)__builtin_amdgcn_readlane((int)kel, e + u);                                \
            sc[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(svm), e + u));                           \
            const float* __restrict__ rp = gou + ko;                /* wave-uniform row address */                   \
            /* branch-free (inactive lanes read lane 0's columns): the gathers stay in one basic block */            \
            if (V == 4) {                                                                                            \
                const float4 t = *reinterpret_cast<const float4*>(&rp[cla]);                                         \
                g[u][0] = t.x; g[u][1 % V] = t.y; g[u][2 % V] = t.z; g[u][3 % V] = t.w;                              \
            } else if (V == 2) {                                                                                     \
                const float2 t = *reinterpret_cast<const float2*>(&rp[cla]);                                         \
                g[u][0] = t.x; g[u][1 % V] = t.y;                                                                    \
            } else {                                                                                                 \
                g[u][0] = rp[cla];                                                                                   \
            }                                                                                                        \
        }                                                                                                            \
        _Pragma("unroll") for (int u = 0; u < NB; u++)                                                               \
            _Pragma("unroll") for (int v = 0; v < V; v++) sg[v] = fmaf(g[u][v], sc[u], sg[v]);                       \
    }
                    int e = e0;
                    for (; e + 4 <= e1; e += 4) SPH3D_BWD_BATCH(4)
                    const int rem = e1 - e;
                    if (rem == 3) SPH3D_BWD_BATCH(3)
                    else if (rem == 2) SPH3D_BWD_BATCH(2)
                    else if (rem == 1) SPH3D_BWD_BATCH(1)
#undef SPH3D_BWD_BATCH
                    }
#pragma unroll
                    for (int v = 0; v < V; v++) {
                        gi[v] = fmaf(sg[v], wr[v], gi[v]);
                        acc[fi][v] = fmaf(sg[v], xv[v], acc[fi][v]);
                    }
                }
            }
        }
        cb += cstep;
        if (cb < E1) take_chunk(false);
        }   // chunks of 64 in-edges
        if (HALF) {
#pragma unroll
            for (int v = 0; v < V; v++) {
                gi[v] += __shfl_xor(gi[v], 32);
                if (PARTS == 4) gi[v] += __shfl_xor(gi[v], 16);
            }
        }
        if (act && half == 0) {
            float* gp = &(gin + ((size_t)b * N + n) * Cs)[lane_offset(cin0)];
            if (V >= R) {
#pragma unroll
                for (int u = 0; u < VI; u++) {
                    float s = 0.f;
#pragma unroll
                    for (int rr = 0; rr < R; rr++) s += gi[u * R + rr];
                    if (HUB == 2) atomicAdd(&gp[u], s);          // the row was zeroed by the HUB == 1 launch in front of this one
                    else gp[u] = s;
                }
            }
        }
    }

    }   // items

    if (HALF) {
#pragma unroll
        for (int i = 0; i < MAXF; i++)
#pragma unroll
            for (int v = 0; v < V; v++) {
                acc[i][v] += __shfl_xor(acc[i][v], 32);
                if (PARTS == 4) acc[i][v] += __shfl_xor(acc[i][v], 16);
            }
    }
    // workgroup reduction of the per-wave accumulators: waves take turns on one [F][SL] LDS table
    __syncthreads();                 // everyone is done reading lfilt
    float* tab = lds;                // reuse: [F][SL]
    // COMPACT: only the rows of bins that occur are summed, written to the slab and read by reduce_filter_partials (which
    // writes zeros for the others): half of the slab traffic at S3DIS radii (17 of 33 bins)
    __shared__ unsigned long long activeMask;
    if (COMPACT) {
        if (threadIdx.x == 0) activeMask = 0ull;
        __syncthreads();
        if ((int)threadIdx.x < A) atomicOr(&activeMask, 1ull << activeBins[1 + threadIdx.x]);
        __syncthreads();
    }
    for (int w = 0; w < kBwdTWaves; w++) {
        if (wave == w && act && half == 0) {
#pragma unroll
            for (int i = 0; i < MAXF; i++) {
                if (i < (COMPACT ? A : F)) {
                    const int f = COMPACT ? uniform(activeBins[1 + i]) : i;
#pragma unroll
                    for (int v = 0; v < V; v++) {
                        float* p = &tab[f * SL + cl0 + v];
                        *p = (w == 0) ? acc[i][v] : (*p + acc[i][v]);
                    }
                }
            }
        }
        __syncthreads();
    }
    float* out = partial + (HUB == 2 ? (size_t)slabBase + w : (size_t)xcd * W + w) * ((size_t)F * CR);
    const unsigned long long am = COMPACT ? activeMask : ~0ull;
    for (int e = threadIdx.x; e < F * SL; e += blockDim.x) {
        const int f = e / SL;
        const int cl = e - f * SL;
        if (!COMPACT || ((am >> f) & 1ull)) out[(size_t)f * CR + slice0 + cl] = tab[e];
    }
}

// grad_filter[j] = sum over the B*nblocks partial tables, fixed order -> deterministic given the partials.
// 1024 threads = 32 outputs x 32 partial-lanes (a one-thread-per-output loop over ~1000 slabs is latency-bound; 8 lanes: 20-30 us).
__global__ __launch_bounds__(1024) void reduce_filter_partials(int nparts, int total, int CR, const float* __restrict__ partial,
                                                              float* __restrict__ gradFilter,
                                                              const int* __restrict__ activeBins, int compactMax, int npartsCompact)
{
    const bool compact = activeBins != nullptr && activeBins[0] <= compactMax;
    if (compact) nparts = npartsCompact;   // the compact launch wrote the slabs — only the rows of the bins that occur
    __shared__ float red[32][32];      // 32 outputs x 32 partial-lanes
    __shared__ unsigned long long activeMask;
    if (compact) {
        if (threadIdx.x == 0) activeMask = 0ull;
        __syncthreads();
        if ((int)threadIdx.x < activeBins[0]) atomicOr(&activeMask, 1ull << activeBins[1 + threadIdx.x]);
        __syncthreads();
    }
    const int cx = (int)threadIdx.x & 31, py = (int)threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + cx;
    float s = 0.f;
    if (j < total && (!compact || ((activeMask >> (j / CR)) & 1ull))) {
        // eight slabs per trip, loads issued together (one per trip = up to 32 dependent L2 round trips per launch)
        for (int p0 = py; p0 < nparts; p0 += 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int p = p0 + u * 32;
                v[u] = partial[(size_t)(p < nparts ? p : py) * total + j];
            }
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (p0 + u * 32 < nparts) s += v[u];
        }
    }
    red[py][cx] = s;
    __syncthreads();
    if (py == 0 && j < total) {
        for (int k = 1; k < 32; k++) s += red[k][cx];
        gradFilter[j] = s;
    }
}

// generic transposed backward (any C, r <= 256): lanes own INPUT channels c_base + lane + 64*t,
// a slice is SC = min(C - c_base, max(1, 256 / r)) input channels; LDS table [F][SC*r]
__global__ __launch_bounds__(256) void dwconv_bwd_t_generic(
    int B, int N, int M, int F, int C, int r, int nblocks, int nslices, int sliceC,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const float* __restrict__ entScale,
    const float* __restrict__ input, const float* __restrict__ filter, const float* __restrict__ gradOutput,
    float* __restrict__ gradInput, float* __restrict__ gradFilter)
{
    extern __shared__ __attribute__((aligned(16))) float gtab[];
    const int CR = C * r;
    int b, part;
    xcd_decode((int)blockIdx.x, B, nblocks * nslices, b, part);
    if (b < 0) return;
    const int slice = part / nblocks;
    const int nb = part - slice * nblocks;
    const int c_base = slice * sliceC;
    const int SC = (C - c_base) < sliceC ? (C - c_base) : sliceC;
    const int SW = SC * r;
    for (int e = threadIdx.x; e < F * SW; e += blockDim.x) gtab[e] = 0.f;
    __syncthreads();

    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int n_begin = nb * 64;
    const int n_end = (n_begin + 64) < N ? (n_begin + 64) : N;
    const int* __restrict__ offb = offsets + (size_t)b * ((size_t)N * F + 1);
    for (int n = n_begin + wave; n < n_end; n += 4) {
        const int* __restrict__ o = offb + (size_t)n * F;
        for (int t = 0; t < 4; t++) {
            const int cl = lane + 64 * t;
            if (cl >= SC) break;
            const int cin = c_base + cl;
            const float x = input[((size_t)b * N + n) * C + cin];
            float gi = 0.f;
            for (int f = 0; f < F; f++) {
                const int e0 = o[f], e1 = o[f + 1];
                if (e0 >= e1) continue;
                for (int rr = 0; rr < r; rr++) {
                    const int cout = cin * r + rr;
                    float sg = 0.f;
                    for (int e = e0; e < e1; e++)
                        sg = fmaf(gradOutput[((size_t)b * M + tg_key(entKey[e], entScale == nullptr)) * CR + cout],
                                  entScale == nullptr ? tg_packed_scale(entKey[e]) : entScale[e], sg);
                    gi = fmaf(sg, filter[(size_t)f * CR + cout], gi);
                    unsafeAtomicAdd(&gtab[f * SW + cl * r + rr], sg * x);     // one LDS atomic per (segment, channel)
                }
            }
            gradInput[((size_t)b * N + n) * C + cin] = gi;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < F * SW; e += blockDim.x) {
        const int f = e / SW;
        const int j = e - f * SW;
        const float g = gtab[e];
        if (g != 0.f) unsafeAtomicAdd(&gradFilter[(size_t)f * CR + c_base * r + j], g);
    }
}

// ------------------------------------------------------------------------------------------
// backward over the transposed graph for ODD row widths (r = 1, C odd: the ModelNet plan's C = 67 and 131), the fixed-order
// form deterministic mode runs where dwconv_bwd_t_generic would sum with float atomics.  The scheme is dwconv_bwd_t_vec's
// full-wave form — one wave per source, the F segments walked in entry order in a fully unrolled loop, four row gathers issued
// before the first is used and the segment's last one to three edges with exactly that many, grad_input in registers and stored
// once, grad_filter in a private [MAXF][T] register table, the four waves' tables added through LDS in turn order into one slab,
// reduce_filter_partials over the slabs — with another ownership of the channels: a row of C floats is only 4-byte aligned, so
// no lane can load two or four channels at once; lane l owns channels slice0 + l + 64 t, t < T (the generic kernels' ownership),
// and a row gather is T dword loads, each coalesced on any alignment, with the lanes past the row's end reading the slice's first
// column.  T <= 4 for F <= 33 and T <= 2 for F <= 65: at most 132 accumulator registers, as the V = 4 form.
// The partition is conv_table's static one (conv_plan.hpp; W workgroups per XCD and slice, (cloud, part) items dealt to the XCDs, positions of
// source_order interleaved over the waves): no work cursor, no hub launches, no atomics of any kind, so every slab is a function
// of the shape, the graph and the order alone.
// ------------------------------------------------------------------------------------------
template <int T, int MAXF>
__global__ __launch_bounds__(kBwdTWaves * 64, 3) void dwconv_bwd_t_odd(
    int B, int N, int M, int F, int C, int W, int parts, int nslices,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const float* __restrict__ entScale,
    const int* __restrict__ order,
    const float* __restrict__ input, const float* __restrict__ filter, const float* __restrict__ gradOutput,
    float* __restrict__ gradInput, float* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SLW = 64 * T;                 // slice width in channels
    const int xcd = (int)blockIdx.x & 7;
    const int q = (int)blockIdx.x >> 3;
    const int slice = q / W;
    const int w = q - slice * W;
    const int slice0 = slice * SLW;
    const int SL = (C - slice0) < SLW ? (C - slice0) : SLW;
    // [F][SLW], zeros past the slice's end: a compile-time row stride, so a lane reads row fi at ONE address + an immediate
    // (with the stride SL the compiler kept MAXF x T hoisted addresses in registers and spilled the accumulators)
    float* lfilt = lds;
    for (int e = threadIdx.x; e < F * SLW; e += blockDim.x) {
        const int f = e / SLW;
        const int cl = e - f * SLW;
        lfilt[e] = cl < SL ? filter[(size_t)f * C + slice0 + cl] : 0.f;
    }
    __syncthreads();

    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int stride = W * kBwdTWaves;
    bool act[T];
    unsigned cla[T];                            // the lane's columns inside the slice; past the row's end: column 0 (read, never stored)
#pragma unroll
    for (int t = 0; t < T; t++) {
        act[t] = lane + 64 * t < SL;
        cla[t] = act[t] ? (unsigned)(lane + 64 * t) : 0u;
    }
    float acc[MAXF][T];
#pragma unroll
    for (int i = 0; i < MAXF; i++)
#pragma unroll
        for (int t = 0; t < T; t++) acc[i][t] = 0.f;

    for (int item = xcd; item < B * parts; item += 8) {
    const int b = item / parts;
    const int pi = item - b * parts;
    const float* __restrict__ gou = gradOutput + (size_t)b * M * C + slice0;
    const int* __restrict__ offb = offsets + (size_t)b * ((size_t)N * F + 1);
    for (int p = pi + parts * (w * kBwdTWaves + wave); p < N; p += parts * stride) {
        const int n = order ? uniform(order[(size_t)b * N + p]) : p;
        // the source's F + 1 segment bounds: one coalesced read (two for 65 bins), consumed with v_readlane
        const int* __restrict__ o = offb + (size_t)n * F;
        const int ov0 = o[lane <= F ? lane : F];
        const int ov1 = (MAXF >= 64) ? o[(64 + lane) <= F ? (64 + lane) : F] : 0;
        const size_t xrow = ((size_t)b * N + n) * C + slice0;
        float xv[T], gi[T];
#pragma unroll
        for (int t = 0; t < T; t++) {
            xv[t] = input[xrow + cla[t]];
            gi[t] = 0.f;
        }
        const int E0 = __builtin_amdgcn_readlane(ov0, 0);
        const int E1 = uniform(o[F]);
        for (int cb = E0; cb < E1; cb += 64) {
        // keys and scales of 64 in-edges: one coalesced load each (lane = edge), handed to the gathers with v_readlane
        const int cn = (E1 - cb) < 64 ? (E1 - cb) : 64;
        const int li = lane < cn ? lane : 0;
        const int wkey = entKey[cb + li];
        const unsigned kel = (unsigned)tg_key(wkey, entScale == nullptr) * (unsigned)C;     // row offset in floats (M * C < 2^32: launcher)
        const float sv = entScale == nullptr ? tg_packed_scale(wkey) : entScale[cb + li];
#pragma unroll
        for (int fi = 0; fi < MAXF; fi++) {
            if (fi < F) {
                const int a0 = __builtin_amdgcn_readlane(fi < 64 ? ov0 : ov1, fi & 63);
                const int a1 = __builtin_amdgcn_readlane((fi + 1) < 64 ? ov0 : ov1, (fi + 1) & 63);
                // the part of the segment inside this chunk, as lane numbers
                const int e0 = (a0 > cb ? a0 : cb) - cb;
                const int e1 = (a1 < cb + cn ? a1 : cb + cn) - cb;
                if (e0 < e1) {                               // wave-uniform
                    float sg[T], wr[T];
#pragma unroll
                    for (int t = 0; t < T; t++) {
                        sg[t] = 0.f;
                        wr[t] = lfilt[fi * SLW + 64 * t + lane];     // read under the gathers, not after them
                    }
                    // lanes e0 .. e1 - 1 only: no row outside the segment is gathered, no foreign row is multiplied by 0
#define SPH3D_BWD_ODD_BATCH(NB)                                                                                      \
    {                                                                                                                \
        float sc[NB];                                                                                                \
        float g[NB][T];                                                                                              \
        _Pragma("unroll") for (int u = 0; u < NB; u++) {                                                             \
            const unsigned ko = (unsigned)__builtin_amdgcn_readlane((int)kel, e + u);                                \
            sc[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), e + u));                            \
            const float* __restrict__ rp = gou + ko;                /* wave-uniform row address */                   \
            _Pragma("unroll") for (int t = 0; t < T; t++) g[u][t] = rp[cla[t]];                                      \
        }                                                                                                            \
        _Pragma("unroll") for (int u = 0; u < NB; u++)                                                               \
            _Pragma("unroll") for (int t = 0; t < T; t++) sg[t] = fmaf(g[u][t], sc[u], sg[t]);                       \
    }
                    int e = e0;
                    for (; e + 4 <= e1; e += 4) SPH3D_BWD_ODD_BATCH(4)
                    const int rem = e1 - e;
                    if (rem == 3) SPH3D_BWD_ODD_BATCH(3)
                    else if (rem == 2) SPH3D_BWD_ODD_BATCH(2)
                    else if (rem == 1) SPH3D_BWD_ODD_BATCH(1)
#undef SPH3D_BWD_ODD_BATCH
#pragma unroll
                    for (int t = 0; t < T; t++) {
                        gi[t] = fmaf(sg[t], wr[t], gi[t]);
                        acc[fi][t] = fmaf(sg[t], xv[t], acc[fi][t]);
                    }
                }
            }
        }
        }   // chunks of 64 in-edges
        // stored once per element; a source without in-edges gets its zero row
#pragma unroll
        for (int t = 0; t < T; t++)
            if (act[t]) gradInput[xrow + cla[t]] = gi[t];
    }
    }   // items

    // workgroup reduction of the per-wave tables: the waves take turns, in wave order, on one [F][SLW] LDS table (the columns
    // past the slice's end hold what their idle lanes computed; they are not copied out)
    __syncthreads();                 // everyone is done reading lfilt
    float* tab = lds;
    for (int tw = 0; tw < kBwdTWaves; tw++) {
        if (wave == tw) {
#pragma unroll
            for (int i = 0; i < MAXF; i++) {
                if (i < F) {
#pragma unroll
                    for (int t = 0; t < T; t++) {
                        float* p = &tab[i * SLW + 64 * t + lane];
                        *p = (tw == 0) ? acc[i][t] : (*p + acc[i][t]);
                    }
                }
            }
        }
        __syncthreads();
    }
    float* out = partial + ((size_t)xcd * W + w) * ((size_t)F * C);
    for (int e = threadIdx.x; e < F * SL; e += blockDim.x) {
        const int f = e / SL;
        const int cl = e - f * SL;
        out[(size_t)f * C + slice0 + cl] = tab[f * SLW + cl];
    }
}

}  // namespace sph3d

using namespace sph3d;

// ---- the host side --------------------------------------------------------------------------------------------------------------
// Every entry point asks conv_plan.hpp for the plan of its call and launches what the plan says; the checks they share (the
// dimensions, the refusals, the workspace) are written once each.  The templates are chosen by switches on plan fields.
struct ConvShape {
    int op, B, N, M, F, Ca, Cb, r, K;       // K: the gradient entries have none and say 1
};

// Test hooks SPH3D_BWD_HUB_MIN_N / SPH3D_BWD_HUB_T: read per call
static int hub_min_n() { return test_hook("SPH3D_BWD_HUB_MIN_N", 32768); }
static int hub_threshold() { const int t = test_hook("SPH3D_BWD_HUB_T", 1024); return t < 1 ? 1 : t; }

static ConvPlan plan_of(const ConvShape& s, bool active_given, bool deterministic = deterministic_on())
{
    const bool grad = s.op == kConvGradT || s.op == kConvGradTCat;
    return conv_plan(s.op, s.B, s.N, s.M, s.F, s.Ca, s.Cb, s.r, s.K, deterministic, active_given, grad ? hub_min_n() : 0,
                     grad ? hub_threshold() : 0);
}

// the entry point's answer where the plan already is one: SPH3D_EINVAL, SPH3D_EUNSUPPORTED.  SPH3D_OK: launch (kernel none: nothing)
static int plan_status(const ConvPlan& p, const ConvShape& s)
{
    const bool grad = s.op == kConvGradT || s.op == kConvGradTCat, cat = s.op == kConvFwdCat || s.op == kConvGradTCat;
    const char* who = grad ? "DepthwiseConv3dGrad" : "DepthwiseConv3d";
    const long long C = (long long)s.Ca + s.Cb;
    SPH3D_REQUIRE(p.bad != kConvBadDims, "%s: bad dims B=%d N=%d M=%d F=%d C=%lld r=%d K=%d", who, s.B, s.N, s.M, s.F, C, s.r, s.K);
    SPH3D_REQUIRE(p.bad != kConvBadLds, "%s: filter table slice F=%d does not fit LDS", who, s.F);
    SPH3D_REQUIRE(p.bad != kConvBadMultiplier, "%s: depth multiplier %d > 256 unsupported", who, s.r);
    SPH3D_REQUIRE(p.bad != kConvBadGrid, "%s: B=%d N=%d M=%d C=%lld r=%d is more than 2^31 - 1 workgroups", who, s.B, s.N, s.M, C, s.r);
    if (p.kernel != kConvRefused) return SPH3D_OK;
    if (cat)
        set_error("%s (two inputs): Ca=%d Cb=%d r=%d not covered (Ca*r must be a multiple of 256)", who, s.Ca, s.Cb, s.r);
    else
        set_error("DepthwiseConv3dGrad: deterministic mode is on and F=%d C=%lld r=%d takes the generic kernel, which sums with float "
                  "atomics (shapes with r in {1, 2} and F <= 65 run the fixed-order kernels)", s.F, C, s.r);
    return SPH3D_EUNSUPPORTED;
}

static int workspace_status(const void* workspace, size_t have, size_t need)
{
    if (need == 0 || (workspace != nullptr && have >= need)) return SPH3D_OK;
    set_error("DepthwiseConv3dGrad: workspace %zu B < required %zu B", have, need);
    return SPH3D_EWORKSPACE;
}

// ---- forward: one input, or (input2) the channel concatenation [input (Ca) | input2 (Cb)] that is never materialised ----------
// (models/SPH3D_s3dis.py:100-104: tf.concat of the un-pooled features and the encoder's skip features feeds the next decoder
// level's separable convolution).  Channel slices of the row kernel are 256 outputs = 256 / r inputs wide; Ca * r must be a
// multiple of 256 so that every slice reads one tensor.  Other shapes: SPH3D_EUNSUPPORTED (concatenate and call the plain ops).
static int run_fwd(const ConvShape& s, const int* nn_index, const int* nn_count, const int* bin_index, const float* input,
                   const float* input2, const float* filter, float* output, sph3d_stream_t stream, const char* what)
{
    const ConvPlan p = plan_of(s, false);
    int rc = plan_status(p, s);
    if (rc || p.kernel == kConvNone) return rc;
    hipStream_t st = as_stream(stream);
    const int B = s.B, N = s.N, M = s.M, F = s.F, C = s.Ca + s.Cb, r = s.r, K = s.K, nslices = (int)p.nslices;
    static_assert(kMultiPoints == kFwdPointsPerWG, "one mblocks for the three kernels");
    const int mblocks = (int)((M + (long long)kFwdPointsPerWG - 1) / kFwdPointsPerWG);
    const dim3 grid((unsigned)p.grid);
    const size_t lds = (size_t)p.lds;
    if (p.kernel == kConvFwdMulti) {
        // 65..128 channels: 32 lanes per edge, TWO neighbour rows per wave load.  (Round 1 had measured this shape slower than one
        // row per load, 0.353 vs 0.297 ms at C = 128; with the zero-row padding and vector-side offsets of round 2 it is
        // 0.202 vs 0.240 ms = 16.6 % of the roofline, ahead of the LDS-tiled kernel and without a plan.  64 lanes per edge for
        // C >= 256 — one pass over the edges instead of one per 128-channel slice, but 70 KB of filter table per workgroup —
        // stays behind the row kernel: 0.069 vs 0.060 ms at 2048 x 256.)
        // narrow layers (C <= 64): 16 lanes per edge, four neighbour rows per wave load (measured at C = 64, r = 2:
        // 0.254 -> 0.145 ms; at C >= 128 the one-edge-per-load kernel below is faster: 0.297 vs 0.353 ms with two edges per load)
        auto kern = p.LPE == 32 ? (p.R == 2 ? dwconv_fwd_multi<2, 32, kFwdSB> : dwconv_fwd_multi<1, 32, kFwdSB>)
                                : (p.R == 2 ? dwconv_fwd_multi<2, 16, kFwdSB> : dwconv_fwd_multi<1, 16, kFwdSB>);
        rc = launch_lds(kern, grid, dim3(64 * kMultiWaves), lds, st, "conv3d", B, N, M, F, C, K, mblocks, nslices, nn_index, nn_count,
                        bin_index, input, filter, output);
    } else if (p.kernel == kConvFwdRow) {
        rc = launch_lds(p.R == 2 ? dwconv_fwd_row<2> : dwconv_fwd_row<1>, grid, dim3(256), lds, st, "conv3d", B, N, M, F, C, K, mblocks,
                        nslices, nn_index, nn_count, bin_index, input, filter, output, input2, s.op == kConvFwdCat ? s.Ca : 0);
    } else {
        rc = launch_lds(dwconv_fwd_generic, grid, dim3(256), lds, st, "conv3d", B, N, M, F, C, r, K, mblocks, nslices, nn_index, nn_count,
                        bin_index, input, filter, output);
    }
    if (rc) return rc;
    return check_launch(what);
}

extern "C" int sph3d_depthwise_conv3d(int B, int N, int M, int F, int C, int r, int K,
                                      const int* nn_index, const int* nn_count, const int* bin_index,
                                      const float* input, const float* filter, float* output,
                                      sph3d_stream_t stream)
{
    return run_fwd({kConvFwd, B, N, M, F, C, 0, r, K}, nn_index, nn_count, bin_index, input, nullptr, filter, output, stream,
                   "sph3d_depthwise_conv3d");
}

extern "C" int sph3d_depthwise_conv3d_cat(int B, int N, int M, int F, int Ca, int Cb, int r, int K, const int* nn_index,
                                          const int* nn_count, const int* bin_index, const float* input_a, const float* input_b,
                                          const float* filter, float* output, sph3d_stream_t stream)
{
    return run_fwd({kConvFwdCat, B, N, M, F, Ca, Cb, r, K}, nn_index, nn_count, bin_index, input_a, input_b, filter, output, stream,
                   "sph3d_depthwise_conv3d_cat");
}

extern "C" int sph3d_depthwise_conv3d_cat_supported(int F, int Ca, int Cb, int r)
{
    return plan_of({kConvFwdCat, 1, 1, 1, F, Ca, Cb, r, 1}, false).kernel == kConvFwdRow;       // (a shape question: one point)
}

// ---- gradient over the transposed graph: one input, or (input2, grad_input2) two ---------------------------------------------------
struct GradArgs {
    const int *offsets, *ent_key;
    const float* ent_scale;
    const int *order, *active_bins;
    const float *input, *input2, *filter, *grad_output;
    float *grad_input, *grad_input2, *grad_filter;
    void* workspace;
};

// the vector gradient's launches: the compact table's sweep (if the plan says so) and the full table's — the device chooses which
// of the two does the work, see the kernel —, each with its hub launch behind it when hubs apply.  ab: active_bins for the kernels
template <int R, int V, int MAXF, int PARTS>
static int launch_bwd_t_vec(const ConvPlan& p, const ConvShape& s, const GradArgs& a, const int* ab, hipStream_t st)
{
    const int C = s.Ca + s.Cb, nslices = (int)p.nslices, T = (int)p.hub_threshold;
    int* hub_list = nullptr;
    if (p.hub) {
        hub_list = reinterpret_cast<int*>((char*)a.workspace + p.hub_list_offset);
        int rc = check_hip(hipMemsetAsync(hub_list, 0, sizeof(int), st), "conv3d grad: hub list");
        if (rc) return rc;
    }
    // one launch: `wgs` workgroups per slice, W of them per XCD (the hub launch: W = wgs in all)
    auto launch = [&](auto kern, long long wgs, long long W, long long parts, long long slab_base) {
        return launch_lds(kern, dim3((unsigned)(wgs * nslices)), dim3(kBwdTWaves * 64), (size_t)p.lds, st, "conv3d", s.B, s.N, s.M, s.F, C,
                          (int)W, (int)parts, nslices, a.offsets, a.ent_key, a.ent_scale, a.order, ab, kCompactBins, a.input, a.filter,
                          a.grad_output, a.grad_input, (float*)a.workspace, a.input2, a.grad_input2, s.op == kConvGradTCat ? s.Ca : 0,
                          hub_list, T, (int)slab_base);
    };
    // one table's sweep over all sources and, when hubs apply, the hub launch behind it (HUB = 1, 2 exist for V == 4 only)
    auto sweep = [&](auto compact_table, const ConvTable& t) {
        constexpr bool CT = decltype(compact_table)::value;
        constexpr int MF = CT ? kCompactBins : MAXF;
        if constexpr (V == 4) {
            if (p.hub) {
                int rc = launch(dwconv_bwd_t_vec<R, V, MF, PARTS, CT, 1>, t.slabs, t.W, t.parts, 0);
                if (rc) return rc;
                return launch(dwconv_bwd_t_vec<R, V, MF, PARTS, CT, 2>, kHubWG, kHubWG, 1, t.slabs);
            }
        }
        return launch(dwconv_bwd_t_vec<R, V, MF, PARTS, CT, 0>, t.slabs, t.W, t.parts, 0);
    };
    if constexpr (V == 4) {
        if (p.compact_launch) {
            int rc = sweep(std::true_type{}, p.compact);
            if (rc) return rc;
        }
    }
    return sweep(std::false_type{}, p.full);
}

// the instantiation for the plan's depth multiplier, channels per lane (with them the row count) and wave parts
static int run_bwd_t_vec(const ConvPlan& p, const ConvShape& s, const GradArgs& a, const int* ab, hipStream_t st)
{
    using std::integral_constant;
    auto go = [&](auto R, auto V, auto PARTS) { return launch_bwd_t_vec<R(), V(), (V() == 4 ? 33 : 65), PARTS()>(p, s, a, ab, st); };
    auto with_r = [&](auto R) {
        if (p.V == 2) return go(R, integral_constant<int, 2>{}, integral_constant<int, 1>{});
        if (p.PARTS == 4) return go(R, integral_constant<int, 4>{}, integral_constant<int, 4>{});
        if (p.PARTS == 2) return go(R, integral_constant<int, 4>{}, integral_constant<int, 2>{});
        return go(R, integral_constant<int, 4>{}, integral_constant<int, 1>{});
    };
    return p.R == 2 ? with_r(integral_constant<int, 2>{}) : with_r(integral_constant<int, 1>{});
}

// the odd-width gradient (deterministic mode): the sweep of the instantiation for (T, rows)
static int run_bwd_t_odd(const ConvPlan& p, const ConvShape& s, const GradArgs& a, hipStream_t st)
{
    auto go = [&](auto kern) {
        return launch_lds(kern, dim3((unsigned)p.grid), dim3(kBwdTWaves * 64), (size_t)p.lds, st, "conv3d", s.B, s.N, s.M, s.F, s.Ca,
                          (int)p.full.W, (int)p.full.parts, (int)p.nslices, a.offsets, a.ent_key, a.ent_scale, a.order, a.input, a.filter,
                          a.grad_output, a.grad_input, (float*)a.workspace);
    };
    const int T = (int)p.V;
    if (p.MAXF == 33) return T == 1 ? go(dwconv_bwd_t_odd<1, 33>) : T == 2 ? go(dwconv_bwd_t_odd<2, 33>)
                           : T == 3 ? go(dwconv_bwd_t_odd<3, 33>) : go(dwconv_bwd_t_odd<4, 33>);
    return T == 1 ? go(dwconv_bwd_t_odd<1, 65>) : go(dwconv_bwd_t_odd<2, 65>);
}

static int run_grad_t(const ConvShape& s, const GradArgs& a, size_t workspace_bytes, sph3d_stream_t stream)
{
    const ConvPlan p = plan_of(s, a.active_bins != nullptr);
    int rc = plan_status(p, s);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const int C = s.Ca + s.Cb, CR = C * s.r, total = s.F * CR;
    // no cloud: grad_filter is all there is to write; the generic kernel adds into it with atomics
    if (p.kernel == kConvNone || p.kernel == kConvBwdGeneric) {
        rc = check_hip(hipMemsetAsync(a.grad_filter, 0, sizeof(float) * (size_t)total, st), "conv3d grad: memset");
        if (rc || p.kernel == kConvNone) return rc;
    }
    rc = workspace_status(a.workspace, workspace_bytes, (size_t)p.workspace_bytes);
    if (rc) return rc;
    const int* ab = p.compact_launch ? a.active_bins : nullptr;
    if (p.kernel == kConvBwdVec) {
        rc = run_bwd_t_vec(p, s, a, ab, st);
    } else if (p.kernel == kConvBwdOdd) {
        rc = run_bwd_t_odd(p, s, a, st);
    } else {
        const int sliceC = (int)(p.lds / ((long long)sizeof(float) * s.F * s.r));           // the table is [F][sliceC r] floats
        rc = launch_lds(dwconv_bwd_t_generic, dim3((unsigned)p.grid), dim3(256), (size_t)p.lds, st, "conv3d", s.B, s.N, s.M, s.F, C, s.r,
                        (int)((s.N + 63LL) / 64), (int)p.nslices, sliceC, a.offsets, a.ent_key, a.ent_scale, a.input, a.filter,
                        a.grad_output, a.grad_input, a.grad_filter);
    }
    if (rc) return rc;
    // the slabs' sum (after a compact run: that table's slab count, and only the rows of the bins that occur)
    if (p.reduce_slabs)
        hipLaunchKernelGGL(reduce_filter_partials, dim3((total + 31) / 32), dim3(1024), 0, st, (int)p.reduce_slabs, total, CR,
                           (const float*)a.workspace, a.grad_filter, ab, p.kernel == kConvBwdVec ? kCompactBins : 0,
                           (int)p.reduce_slabs_compact);
    return check_launch("sph3d_depthwise_conv3d_grad_t");
}

extern "C" int sph3d_depthwise_conv3d_grad_t(int B, int N, int M, int F, int C, int r,
                                             const int* offsets, const int* ent_key, const float* ent_scale,
                                             const int* source_order, const int* active_bins,
                                             const float* input, const float* filter, const float* grad_output,
                                             float* grad_input, float* grad_filter,
                                             void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    return run_grad_t({kConvGradT, B, N, M, F, C, 0, r, 1}, {offsets, ent_key, ent_scale, source_order, active_bins, input, nullptr, filter,
                      grad_output, grad_input, nullptr, grad_filter, workspace}, workspace_bytes, stream);
}

extern "C" int sph3d_depthwise_conv3d_grad_t_cat(int B, int N, int M, int F, int Ca, int Cb, int r, const int* offsets, const int* ent_key,
                                                 const float* ent_scale, const int* source_order, const int* active_bins,
                                                 const float* input_a, const float* input_b, const float* filter,
                                                 const float* grad_output, float* grad_a, float* grad_b, float* grad_filter,
                                                 void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    return run_grad_t({kConvGradTCat, B, N, M, F, Ca, Cb, r, 1}, {offsets, ent_key, ent_scale, source_order, active_bins, input_a, input_b,
                      filter, grad_output, grad_a, grad_b, grad_filter, workspace}, workspace_bytes, stream);
}

// bytes of the gradient's own workspace.  (M = 0: they do not depend on M — a call whose grad_output rows pass 32-bit offsets
// takes a kernel that needs none)
extern "C" size_t sph3d_depthwise_conv3d_grad_t_workspace(int B, int N, int F, int C, int r)
{
    return (size_t)plan_of({kConvGradT, B, N, 0, F, C, 0, r, 1}, false).workspace_bytes;
}
extern "C" size_t sph3d_depthwise_conv3d_grad_workspace(int B, int N, int M, int F, int C, int r, int K)
{
    return tg_layout(nullptr, B, N, M, K, F).bytes + sph3d_depthwise_conv3d_grad_t_workspace(B, N, F, C, r);
}

// the one-call gradient: the transposed graph, built in front of the caller's workspace, then sph3d_depthwise_conv3d_grad_t
extern "C" int sph3d_depthwise_conv3d_grad(int B, int N, int M, int F, int C, int r, int K,
                                           const int* nn_index, const int* nn_count, const int* bin_index,
                                           const float* input, const float* filter, const float* grad_output,
                                           float* grad_input, float* grad_filter,
                                           void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    const ConvShape with_k = {kConvGradT, B, N, M, F, C, 0, r, K}, s = {kConvGradT, B, N, M, F, C, 0, r, 1};
    int rc = plan_status(plan_of(with_k, true), with_k);           // (the dimensions, K among them, before they size the graph)
    if (rc) return rc;
    GradArgs a = {nullptr, nullptr, nullptr, nullptr, nullptr, input, nullptr, filter, grad_output, grad_input, nullptr, grad_filter, nullptr};
    if (B == 0) return run_grad_t(s, a, 0, stream);
    const TgLayout t = tg_layout(workspace, B, N, M, K, F);
    rc = workspace_status(workspace, workspace_bytes, sph3d_depthwise_conv3d_grad_workspace(B, N, M, F, C, r, K));
    if (rc) return rc;
    rc = sph3d_graph_transpose(B, N, M, K, F, nn_index, nn_count, bin_index, nullptr, t.offsets, t.key, t.scale, t.active,
                               t.scratch, t.scratch_bytes, stream);
    if (rc) return rc;
    a.offsets = t.offsets, a.ent_key = t.key, a.ent_scale = t.scale, a.active_bins = t.active, a.workspace = (char*)workspace + t.bytes;
    return run_grad_t(s, a, workspace_bytes - t.bytes, stream);
}

// ---- the plan, reported (include/sph3d.h) ---------------------------------------------------------------------------------------------
extern "C" int sph3d_depthwise_conv3d_plan(int op, int B, int N, int M, int F, int Ca, int Cb, int r, int K, int deterministic,
                                           int active_given, long long* out)
{
    const bool grad = op == kConvGradT || op == kConvGradTCat, cat = op == kConvFwdCat || op == kConvGradTCat;
    SPH3D_REQUIRE(out != nullptr && op >= kConvFwd && op <= kConvGradTCat && deterministic >= -1 && deterministic <= 1 &&
                      (active_given == 0 || active_given == 1) && (cat || Cb == 0),
                  "sph3d_depthwise_conv3d_plan: bad argument (op=%d deterministic=%d active_given=%d Cb=%d out=%p)", op, deterministic,
                  active_given, Cb, (void*)out);
    const ConvShape s = {op, B, N, M, F, Ca, Cb, r, grad ? 1 : K};
    const ConvPlan p = plan_of(s, active_given != 0, deterministic < 0 ? deterministic_on() : deterministic != 0);
    if (p.bad) return plan_status(p, s);
    static_assert(offsetof(ConvPlan, bad) == SPH3D_CONV_PLAN_FIELDS * sizeof(long long), "the plan starts with the documented fields, in their order");
    static_assert(kConvFwd == SPH3D_CONV_FWD && kConvFwdCat == SPH3D_CONV_FWD_CAT && kConvGradT == SPH3D_CONV_GRAD_T && kConvGradTCat == SPH3D_CONV_GRAD_T_CAT,
                  "the ops as the header numbers them");
    memcpy(out, &p, SPH3D_CONV_PLAN_FIELDS * sizeof(long long));
    return SPH3D_OK;
}
