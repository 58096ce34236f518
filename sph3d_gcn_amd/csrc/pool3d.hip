// pool3d.hip — graph max/avg pooling and mean/weighted un-pooling (forward + gradients), gfx950.
//
// Replaces max_pool3d_forward/backward, avg_pool3d_forward/backward (tf_ops/pooling/tf_pool3d_gpu.cu:5-90)
// and mean/weighted_interpolate_forward/backward (tf_ops/unpooling/tf_unpool3d_gpu.cu:5-84).
//
// All eight kernels are the same shape of work — "for every output point, walk its neighbour list and
// combine gathered feature rows" — so they share one skeleton: one wavefront per output point, the
// neighbour row read through the scalar cache (its address is wave-uniform), lanes spanning channels
// with float4 (or scalar when C % 4 != 0) coalesced row reads, accumulation in registers, one store.
// The reference used one thread per (point, channel) with a global read-modify-write per neighbour
// and a cudaDeviceSynchronize after every launch (tf_pool3d_gpu.cu:97,104,111,118).
// Un-pooling "mean" is avg-pooling with the roles of the point sets swapped, so it reuses that kernel.
// avg / mean / weighted gradients gather over the transposed graph (graph.hip).  The max-pool gradient (one element per output,
// data-dependent target) has three forms: a gather over the transposed pooling graph (maxpool_bwd_t), the same gather over the
// level's intra transpose through a row link (maxpool_bwd_rows) — both write every element once, in a fixed order — and the
// reference's scatter (maxpool_bwd), the one kernel of the file that adds with hardware fp32 atomics: it serves callers without
// a transposed graph and is refused in deterministic mode.
// Which kernel a call launches, and at which shape, is decided in pool_plan.hpp (pool_plan) and nowhere else.
#include <stddef.h>
#include <string.h>
#include "common.hpp"
#include "pool_plan.hpp"

namespace sph3d {

enum class Mode { Max, Avg, Weighted };

// V = 4: channels c0 + 4*lane + {0..3} per pass of 256 channels; V = 1: c0 + lane (64 per pass)
template <Mode MODE, int V>
__global__ __launch_bounds__(256) void gather_fwd(
    int B, int Nin, int Mout, int C, int K, int mblocks,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount,
    const float* __restrict__ input, const float* __restrict__ weight,
    float* __restrict__ output, int* __restrict__ maxIndex, int ppwg)
{
    int b, mb;
    xcd_decode((int)blockIdx.x, B, mblocks, b, mb);
    if (b < 0) return;
    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int m_begin = mb * ppwg;
    const int m_end = (m_begin + ppwg) < Mout ? (m_begin + ppwg) : Mout;
    const float* inb = input + (size_t)b * Nin * C;

    for (int m = m_begin + wave; m < m_end; m += 4) {
        const size_t row = (size_t)b * Mout + m;
        const int cnt = uniform(nnCount[row]);
        for (int c0 = 0; c0 < C; c0 += 64 * V) {
            const int c = c0 + lane * V;
            const bool act = c < C;
            const int cc = act ? c : 0;
            float acc[V];
            int arg[V];
#pragma unroll
            for (int v = 0; v < V; v++) { acc[v] = 0.f; arg[v] = 0; }
            // wave-uniform address -> scalar loads, eight consecutive ids per s_load_dwordx8.  (Round 2: the vector-load +
            // v_readlane scheme that helped the convolution gradient made the step 3.7 % SLOWER here: these loops have no
            // clamps or interleaved scale loads for it to remove, and a readlane per edge costs more than an eighth of a wide s_load.)
            const int* __restrict__ irow = nnIndex + row * K;
            const float* __restrict__ wrow = weight + row * K;
            {
#pragma unroll 8
                for (int kk = 0; kk < cnt; kk++) {
                    const int n = irow[kk];
                    float w = 1.f;
                    if (MODE == Mode::Weighted) w = wrow[kk];
                    {
                        float x[V];          // branch-free: inactive lanes read channel 0 (keeps the unrolled gathers in flight)
                        if (V == 4) {
                            const float4 t = *reinterpret_cast<const float4*>(&inb[(size_t)n * C + cc]);
                            x[0] = t.x; x[1 % V] = t.y; x[2 % V] = t.z; x[3 % V] = t.w;
                        } else {
                            x[0] = inb[(size_t)n * C + cc];
                        }
#pragma unroll
                        for (int v = 0; v < V; v++) {
                            if (MODE == Mode::Max) {
                                // first neighbour seeds, strict > replaces (tf_pool3d_gpu.cu:17-29)
                                if (kk == 0 || x[v] > acc[v]) { acc[v] = x[v]; arg[v] = n; }
                            } else if (MODE == Mode::Avg) {
                                acc[v] += x[v];
                            } else {
                                acc[v] = fmaf(x[v], w, acc[v]);     // tf_unpool3d_gpu.cu:59
                            }
                        }
                    }
                }
            }
            if (act) {
                const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;
#pragma unroll
                for (int v = 0; v < V; v++) {
                    float o = acc[v];
                    if (MODE == Mode::Avg) o = o * inv;
                    output[row * C + c + v] = o;
                    if (MODE == Mode::Max) maxIndex[row * C + c + v] = arg[v];
                }
            }
        }
    }
}

// C <= 128 (C % 4 == 0): a row is at most 32 lanes of 16 bytes, so the two halves of the wave take ALTERNATE neighbours (one
// wave load = two rows): these launches are bound by the L1's 16 cycles per wave load (3.1 M edges at the decoder's last
// level = 0.08 ms of L1 issue with one row per load, measured 0.128 ms), and with one row per load half the lanes repeat
// lane 0's address.  Max: each half keeps (value, id, slot) of its own neighbours — half 0 is seeded by neighbour 0 as in
// the reference (tf_pool3d_gpu.cu:17-29), half 1 starts from -inf — and the halves are merged with "larger value, then
// earlier slot", which is what the reference's sequential strict-> scan computes.
template <Mode MODE>
__global__ __launch_bounds__(256) void gather_fwd_half(
    int B, int Nin, int Mout, int C, int K, int mblocks,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount,
    const float* __restrict__ input, const float* __restrict__ weight,
    float* __restrict__ output, int* __restrict__ maxIndex, int ppwg)
{
    int b, mb;
    xcd_decode((int)blockIdx.x, B, mblocks, b, mb);
    if (b < 0) return;
    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int half = lane >> 5;
    const int c = (lane & 31) * 4;
    const bool act = c < C;
    const int m_begin = mb * ppwg;
    const int m_end = (m_begin + ppwg) < Mout ? (m_begin + ppwg) : Mout;
    const float* inb = input + (size_t)b * Nin * C + (act ? c : 0);

    for (int m = m_begin + wave; m < m_end; m += 4) {
        const size_t row = (size_t)b * Mout + m;
        const int cnt = uniform(nnCount[row]);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int arg[4] = {0, 0, 0, 0}, pos[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
        if (MODE == Mode::Max && half == 1) {
#pragma unroll
            for (int v = 0; v < 4; v++) acc[v] = -__builtin_inff();
        }
        const int* __restrict__ irow = nnIndex + row * K;
        const float* __restrict__ wrow = weight + row * K;
#pragma unroll 4
        for (int kk = 0; kk < cnt; kk += 2) {
            const bool two = (kk + 1) < cnt;                         // wave-uniform
            const int n0 = irow[kk], n1 = irow[two ? kk + 1 : kk];
            float w0 = 1.f, w1 = two ? 1.f : 0.f;                    // the odd tail: the same row again with weight 0 ...
            if (MODE == Mode::Weighted) { w0 = wrow[kk]; w1 = two ? wrow[kk + 1] : 0.f; }
            const int n = half ? n1 : n0;
            const float w = half ? w1 : w0;
            const int k = kk + half;
            const bool real = half == 0 || two;                      // ... or, for max, skipped
            const float4 t = *reinterpret_cast<const float4*>(&inb[(size_t)n * C]);
            const float x[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int v = 0; v < 4; v++) {
                if (MODE == Mode::Max) {
                    if (real && (k == 0 || x[v] > acc[v])) { acc[v] = x[v]; arg[v] = n; pos[v] = k; }
                } else {
                    acc[v] = fmaf(x[v], w, acc[v]);
                }
            }
        }
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const float ov = __shfl_xor(acc[v], 32);
            if (MODE == Mode::Max) {
                const int oa = __shfl_xor(arg[v], 32), op = __shfl_xor(pos[v], 32);
                // larger value wins, equal values: the earlier slot.  Half 0's seed (slot 0) is kept even when it is NaN,
                // like the reference's unconditional first assignment: nothing compares greater than NaN
                if (ov > acc[v] || (ov == acc[v] && op < pos[v])) { acc[v] = ov; arg[v] = oa; pos[v] = op; }
            } else {
                acc[v] += ov;
            }
        }
        if (act && half == 0) {
            float4 o;
            if (MODE == Mode::Avg) {
                const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;      // one reciprocal per point (see conv3d.hip)
                o = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
            } else {
                o = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
            *reinterpret_cast<float4*>(&output[row * C + c]) = o;
            if (MODE == Mode::Max) *reinterpret_cast<int4*>(&maxIndex[row * C + c]) = make_int4(arg[0], arg[1], arg[2], arg[3]);
        }
    }
}

// gradient of avg-pool / mean- and weighted-interpolate as a GATHER over the transposed graph (graph.hip):
//   gradInput[b, n, c] = sum over in-edges (m, scale) of gradOutput[b, m, c] * scale
// scale = 1/nn_count[m] (avg / mean) or weight[b,m,k] (weighted).  One wave per source point n, each
// gradInput element written exactly once: no atomics, no memset (the reference: atomicAdd per
// (point, neighbour, channel), tf_pool3d_gpu.cu:86, tf_unpool3d_gpu.cu:38,80).
// acc[0 .. V) += row[0 .. V) * sc
template <int V>
__device__ __forceinline__ void fma_row(float (&acc)[V], const float* __restrict__ row, float sc)
{
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(row);
        acc[0] = fmaf(t.x, sc, acc[0]);
        acc[1] = fmaf(t.y, sc, acc[1]);
        acc[2] = fmaf(t.z, sc, acc[2]);
        acc[3] = fmaf(t.w, sc, acc[3]);
    } else {
        acc[0] = fmaf(row[0], sc, acc[0]);
    }
}

template <int V>
__global__ __launch_bounds__(256) void gather_bwd_t(
    int B, int Nin, int Mout, int C, int nblocks,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const float* __restrict__ entScale,
    const float* __restrict__ gradOutput, float* __restrict__ gradInput)
{
    int b, nb;
    xcd_decode((int)blockIdx.x, B, nblocks, b, nb);
    if (b < 0) return;
    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int n_begin = nb * kPtsPerWG;
    const int n_end = (n_begin + kPtsPerWG) < Nin ? (n_begin + kPtsPerWG) : Nin;
    const float* gob = gradOutput + (size_t)b * Mout * C;
    const int* __restrict__ offb = offsets + (size_t)b * (Nin + 1);
    for (int n = n_begin + wave; n < n_end; n += 4) {
        const int e0 = offb[n], e1 = offb[n + 1];
        for (int c0 = 0; c0 < C; c0 += 64 * V) {
            const int c = c0 + lane * V;
            const bool act = c < C;
            const int cc = act ? c : 0;
            float acc[V];
#pragma unroll
            for (int v = 0; v < V; v++) acc[v] = 0.f;
#pragma unroll 8
            for (int e = e0; e < e1; e++) {
                const int wk = entKey[e];
                const int m = tg_key(wk, entScale == nullptr);          // (packed entries: common.hpp)
                const float sc = entScale == nullptr ? tg_packed_scale(wk) : entScale[e];
                fma_row<V>(acc, &gob[(size_t)m * C + cc], sc);          // branch-free: inactive lanes read channel 0
            }
            if (act) {
#pragma unroll
                for (int v = 0; v < V; v++) gradInput[((size_t)b * Nin + n) * C + c + v] = acc[v];
            }
        }
    }
}

// max-pool gradient: gradInput[b, maxIndex[b,m,c], c] += gradOutput[b,m,c]   (tf_pool3d_gpu.cu:38-50)
__global__ __launch_bounds__(256) void maxpool_bwd(
    int B, int N, int M, int C, const int* __restrict__ maxIndex,
    const float* __restrict__ gradOutput, float* __restrict__ gradInput)
{
    // grid.y = cloud: no 64-bit division per element; the channel is carried from iteration to iteration
    const int b = (int)blockIdx.y;
    const long long per_b = (long long)M * C;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int c = (int)(i0 % C);
    const int cstep = (int)(stride % C);
    const int* __restrict__ mi = maxIndex + (size_t)b * per_b;
    const float* __restrict__ go = gradOutput + (size_t)b * per_b;
    float* __restrict__ gi = gradInput + (size_t)b * N * C;
    for (long long e = i0; e < per_b; e += stride) {
        unsafeAtomicAdd(&gi[(size_t)mi[e] * C + c], go[e]);
        c += cstep;
        c = c >= C ? c - C : c;
    }
}

// max-pool gradient as a GATHER over the transposed pooling graph (round 3): source point n walks its in-edges m and takes
// gradOutput[b,m,c] where maxIndex[b,m,c] == n.  Every gradInput element is written exactly once: no memset, no float
// atomics (the scatter above: 4.2 M single-lane atomics at S3DIS level 0, 151 us; 47-83 us on the small levels), and the sum
// of the (few) terms of an element has a fixed order.  Rows m WITHOUT neighbours keep maxIndex 0 in the forward pass and the
// scatter adds their gradient to point 0; they have no edge here, so the wave of point 0 looks for them in nn_count.
// What both gathers do for source n of cloud b at channels c .. c + V: seed the sums, hand `walk` the function take(m) that adds
// row m's gradient where its arg-max is n, collect the rows without neighbours (n == 0), store.  mib, gob: the cloud's rows.
template <int V, class Walk>
__device__ __forceinline__ void maxpool_bwd_source(
    int b, int n, int c, int lane, int Nin, int Mout, int C, const int* mib, const float* gob, const int* __restrict__ nnCount,
    const float* __restrict__ addend, float* __restrict__ gradInput, Walk walk)
{
    const bool act = c < C;
    const int cc = act ? c : 0;
    // addend (optional, [B, Nin, C]): a second gradient of the same tensor — the pooled tensor's other consumer, the
    // encoder's skip connection — summed here instead of by a separate elementwise kernel over three tensors
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; v++) acc[v] = addend != nullptr ? addend[((size_t)b * Nin + n) * C + cc + v] : 0.f;
    auto take = [&](int m) {       // branch-free: inactive lanes read channel 0
        if constexpr (V == 4) {
            const int4 a = *reinterpret_cast<const int4*>(&mib[(size_t)m * C + cc]);
            const float4 g = *reinterpret_cast<const float4*>(&gob[(size_t)m * C + cc]);
            acc[0] += a.x == n ? g.x : 0.f;
            acc[1] += a.y == n ? g.y : 0.f;
            acc[2] += a.z == n ? g.z : 0.f;
            acc[3] += a.w == n ? g.w : 0.f;
        } else {
            acc[0] += mib[(size_t)m * C + cc] == n ? gob[(size_t)m * C + cc] : 0.f;
        }
    };
    walk(take);
    if (n == 0) {                  // rows without neighbours: maxIndex 0 (see maxpool_bwd_t); 64 rows per trip
        for (int m0 = 0; m0 < Mout; m0 += 64) {
            const int mm = m0 + lane;
            const int cnt = mm < Mout ? nnCount[(size_t)b * Mout + mm] : 1;
            unsigned long long empty = __ballot(cnt == 0);
            while (empty != 0ull) {
                const int bit = (int)__builtin_ctzll(empty);
                empty &= empty - 1ull;
                take(m0 + bit);
            }
        }
    }
    if (act) {
#pragma unroll
        for (int v = 0; v < V; v++) gradInput[((size_t)b * Nin + n) * C + c + v] = acc[v];
    }
}

template <int V>
__global__ __launch_bounds__(256) void maxpool_bwd_t(
    int B, int Nin, int Mout, int C, int nblocks, int ppwg,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const int* __restrict__ nnCount,
    const int* __restrict__ maxIndex, const float* __restrict__ gradOutput, const float* __restrict__ addend,
    float* __restrict__ gradInput)
{
    int b, nb;
    xcd_decode((int)blockIdx.x, B, nblocks, b, nb);
    if (b < 0) return;
    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int n_begin = nb * ppwg;
    const int n_end = (n_begin + ppwg) < Nin ? (n_begin + ppwg) : Nin;
    const float* gob = gradOutput + (size_t)b * Mout * C;
    const int* mib = maxIndex + (size_t)b * Mout * C;
    const int* __restrict__ offb = offsets + (size_t)b * (Nin + 1);
    for (int n = n_begin + wave; n < n_end; n += 4) {
        const int e0 = offb[n], e1 = offb[n + 1];
        for (int c0 = 0; c0 < C; c0 += 64 * V) {
            maxpool_bwd_source<V>(b, n, c0 + lane * V, lane, Nin, Mout, C, mib, gob, nnCount, addend, gradInput, [&](auto take) {
#pragma unroll 4
                // (an entry word may be packed with the row's count above bit 24: common.hpp; rows are < 2^24 whenever it is)
                for (int e = e0; e < e1; e++) take(Mout <= (1 << 24) ? (int)((unsigned)entKey[e] & kTgKeyMask) : entKey[e]);
            });
        }
    }
}

// The same gather WITHOUT a transposed pooling graph.  A level's pooling graph is the rows of its intra-level graph at the sampled
// points, so the in-edges of source n in the pooling graph are those in-edges (p -> n) of the INTRA graph whose row p was
// sampled: the wave walks n's entries of the intra graph's transposed graph (F segments per source, contiguous: graph.hip), 64 per
// trip, looks every p up in the pooling graph's row link (graph.hip: gather_rows_link_kernel) and takes the pooled rows that copy
// a sampled p — the same rows, hence the same row loads, as maxpool_bwd_t; about N / S times as many 4-byte entries.  The sampled
// entries of a trip are moved to the wave's first lanes so that the row loop is a counted one and keeps four rows in flight.
// Every intra row must list a point at most once (the caller's promise: rows of the ball query do).
template <int V>
__global__ __launch_bounds__(256) void maxpool_bwd_rows(
    int B, int Nin, int Mout, int C, int F, int nblocks, int ppwg,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const int* __restrict__ first, const int* __restrict__ next,
    const int* __restrict__ nnCount, const int* __restrict__ maxIndex, const float* __restrict__ gradOutput,
    const float* __restrict__ addend, float* __restrict__ gradInput)
{
    int b, nb;
    xcd_decode((int)blockIdx.x, B, nblocks, b, nb);
    if (b < 0) return;
    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const int n_begin = nb * ppwg;
    const int n_end = (n_begin + ppwg) < Nin ? (n_begin + ppwg) : Nin;
    const float* gob = gradOutput + (size_t)b * Mout * C;
    const int* mib = maxIndex + (size_t)b * Mout * C;
    const int* __restrict__ offb = offsets + (size_t)b * ((size_t)Nin * F + 1);
    const int* __restrict__ firstb = first + (size_t)b * Nin;
    const int* __restrict__ nextb = next + (size_t)b * Mout;
    for (int n = n_begin + wave; n < n_end; n += 4) {
        const int e0 = offb[(size_t)n * F], e1 = offb[(size_t)n * F + F];
        for (int c0 = 0; c0 < C; c0 += 64 * V) {
            maxpool_bwd_source<V>(b, n, c0 + lane * V, lane, Nin, Mout, C, mib, gob, nnCount, addend, gradInput, [&](auto take) {
                for (int ec = e0; ec < e1; ec += 64) {                     // wave-uniform trips
                    const int e = ec + lane;
                    int link = 0;
                    // (an entry word may be packed with the row's count above bit 24: common.hpp; rows are < 2^24 whenever it is)
                    if (e < e1) link = firstb[Nin <= (1 << 24) ? (int)((unsigned)entKey[e] & kTgKeyMask) : entKey[e]];
                    const unsigned long long hit = __ballot(link != 0);
                    if (hit == 0ull) continue;
                    const int hits = (int)__popcll(hit);
                    const int below = prefix_popc(hit);
                    // a permutation of the lanes: sampled entries first, in entry order
                    const int rows = __builtin_amdgcn_ds_permute((link != 0 ? below : hits + lane - below) << 2, link);
                    auto row = [&](int i) { return (int)((unsigned)__builtin_amdgcn_readlane(rows, i) & kRowLinkMask) - 1; };
                    int i = 0;
                    for (; i + 4 <= hits; i += 4) {        // (by hand: a loop with a cross-lane read is not unrolled with a remainder)
                        const int r0 = row(i), r1 = row(i + 1), r2 = row(i + 2), r3 = row(i + 3);
                        take(r0);
                        take(r1);
                        take(r2);
                        take(r3);
                    }
                    for (; i < hits; i++) take(row(i));
                    unsigned long long more = __ballot(link < 0);          // points that were sampled more than once: their chains
                    while (more != 0ull) {
                        const int bit = (int)__builtin_ctzll(more);
                        more &= more - 1ull;
                        int r = nextb[(int)((unsigned)__builtin_amdgcn_readlane(link, bit) & kRowLinkMask) - 1];
                        while (r != 0) {
                            take(r - 1);
                            r = nextb[r - 1];
                        }
                    }
                }
            });
        }
    }
}

// Few sources with many in-edges each (un-pooling: 2048 coarse points collect ~100 fine points each): one WORKGROUP per
// source, its four waves take every fourth in-edge and the partial sums meet in LDS.  One wave per source (gather_bwd_t)
// leaves such a launch with eight waves per SIMD in total and a 100-edge dependent chain per wave: 0.13 ms at the decoder's
// last level whatever the channel count.  (Two edges per wave load for C <= 128 was measured first: no gain — the launch is
// latency-, not load-bound.)
template <int V>
__global__ __launch_bounds__(256) void gather_bwd_t_split(
    int B, int Nin, int Mout, int C,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const float* __restrict__ entScale,
    const float* __restrict__ gradOutput, float* __restrict__ gradInput)
{
    __shared__ float part[4][64 * V];
    const long long src = (long long)blockIdx.x;
    const int b = (int)(src / Nin);
    const int n = (int)(src - (long long)b * Nin);
    const int wave = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    const float* gob = gradOutput + (size_t)b * Mout * C;
    const int* __restrict__ offb = offsets + (size_t)b * (Nin + 1);
    const int e0 = offb[n], e1 = offb[n + 1];
    for (int c0 = 0; c0 < C; c0 += 64 * V) {
        const int c = c0 + lane * V;
        const bool act = c < C;
        const int cc = act ? c : 0;
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; v++) acc[v] = 0.f;
        if (V == 4 && C <= 128) {
            // a row is at most 32 lanes wide: the two halves of the wave take alternate edges (one wave load = two rows; the
            // launch is bound by the L1's 16 cycles per wave load once there are enough waves)
            const int half = lane >> 5;
            const int ch = (lane & 31) * 4;
            const int cch = ch < C ? ch : 0;
#pragma unroll 4
            for (int e = e0 + 2 * wave; e < e1; e += 8) {
                const bool two = (e + 1) < e1;                           // wave-uniform
                const int w0 = entKey[e], w1 = entKey[two ? e + 1 : e];
                const bool pk = entScale == nullptr;
                const int m0 = tg_key(w0, pk), m1 = tg_key(w1, pk);
                const float s0 = pk ? tg_packed_scale(w0) : entScale[e], s1 = two ? (pk ? tg_packed_scale(w1) : entScale[e + 1]) : 0.f;
                const int m = half ? m1 : m0;
                const float sc = half ? s1 : s0;
                fma_row<V>(acc, &gob[(size_t)m * C + cch], sc);
            }
#pragma unroll
            for (int v = 0; v < V; v++) acc[v] += __shfl_xor(acc[v], 32);       // lanes 0..31 now hold channels 4*lane..
        } else
#pragma unroll 4
        for (int e = e0 + wave; e < e1; e += 4) {
            const int wk = entKey[e];
            const int m = tg_key(wk, entScale == nullptr);
            const float sc = entScale == nullptr ? tg_packed_scale(wk) : entScale[e];
            fma_row<V>(acc, &gob[(size_t)m * C + cc], sc);
        }
        if (c0 > 0) __syncthreads();              // the previous pass's sums have been read
#pragma unroll
        for (int v = 0; v < V; v++) part[wave][lane * V + v] = acc[v];
        __syncthreads();
        if (wave == 0 && act) {
#pragma unroll
            for (int v = 0; v < V; v++)           // fixed order: deterministic
                gradInput[((size_t)b * Nin + n) * C + c + v] =
                    ((part[0][lane * V + v] + part[1][lane * V + v]) + part[2][lane * V + v]) + part[3][lane * V + v];
        }
    }
}

// ---- narrow rows (C <= 16): interpolation of PROJECTED features -----------------------------------------------------------------
// The decoder's last un-pooling feeds only the logits layer, and both are linear: interp(x) W = interp(x W).  The projected rows
// have num_cls (13) floats, and a wave per row would idle 3/4 of its lanes: here 16 lanes own a row, four rows per wave.  The 16
// lanes of a row fetch 16 consecutive neighbour ids (weights / entries) with ONE coalesced load and hand them round by
// shuffle, so an edge costs one gather instruction, not two.
//   out[b, n, :] = base[b, n, :] + sum_k w_k z[b, idx[b, n, k], :]        w_k = 1 / cnt (mean) or weight[b, n, k]
// The neighbours are summed as gather_fwd_half sums them (even slots, odd slots, then the two sums; mean: one multiplication by
// 1 / cnt at the end), so that a projection that only selects channels gives that kernel's values bit for bit.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void narrow_interp_fwd(
    long long rows, int Nf, int Mc, int C, int K,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const float* __restrict__ z,
    const float* __restrict__ weight, const float* __restrict__ base, float* __restrict__ out)
{
    const int l16 = (int)threadIdx.x & 15;
    const bool act = l16 < C;
    const int cc = act ? l16 : 0;
    const long long stride = (long long)gridDim.x * 16;
    for (long long r = (long long)blockIdx.x * 16 + ((int)threadIdx.x >> 4); r < rows; r += stride) {
        const int b = (int)(r / Nf);
        const float* __restrict__ zb = z + (size_t)b * Mc * C + cc;
        int cnt = nnCount[r];
        cnt = cnt < K ? cnt : K;
        const int* __restrict__ irow = nnIndex + (size_t)r * K;
        float acc0 = 0.f, acc1 = 0.f;
        for (int k0 = 0; k0 < cnt; k0 += 16) {                     // (the 16 lanes of a row share cnt: they stay together)
            const bool mine = k0 + l16 < cnt;
            const int my_n = mine ? irow[k0 + l16] : 0;
            float my_w = 1.f;
            if (WEIGHTED) my_w = mine ? weight[(size_t)r * K + k0 + l16] : 0.f;
            const int kn = (cnt - k0) < 16 ? (cnt - k0) : 16;
#pragma unroll 4
            for (int j = 0; j < kn; j += 2) {
                const bool two = (j + 1) < kn;
                const int n0 = __shfl(my_n, j, 16), n1 = __shfl(my_n, two ? j + 1 : j, 16);
                float w0 = 1.f, w1 = two ? 1.f : 0.f;              // the odd tail: the same row again with weight 0, as gather_fwd_half
                if (WEIGHTED) { w0 = __shfl(my_w, j, 16); w1 = two ? __shfl(my_w, j + 1, 16) : 0.f; }
                const float x0 = zb[(size_t)n0 * C], x1 = zb[(size_t)n1 * C];
                acc0 = fmaf(x0, w0, acc0);
                acc1 = fmaf(x1, w1, acc1);
            }
        }
        if (act) {
            const float bv = base != nullptr ? base[(size_t)r * C + l16] : 0.f;
            float o = bv;                                          // rows without neighbours: base, bit for bit
            if (cnt > 0) {
                float s = acc0 + acc1;
                if (!WEIGHTED) s = s * (1.0f / (float)cnt);
                o = base != nullptr ? bv + s : s;
            }
            out[(size_t)r * C + l16] = o;
        }
    }
}

// its gradient with respect to z, a gather over the transposed graph like gather_bwd_t: one WAVE per source point; each of its four
// 16-lane groups takes 16 consecutive in-edges of every 64 (one coalesced load of the entries per 64 edges), two chains per
// group, and the four groups' sums meet by shuffle in a fixed order: no atomics, the same bits on every run.
__global__ __launch_bounds__(256) void narrow_interp_bwd_t(
    long long sources, int Nin, int Mout, int C,
    const int* __restrict__ offsets, const int* __restrict__ entKey, const float* __restrict__ entScale,
    const float* __restrict__ gradOutput, float* __restrict__ gradInput)
{
    const int lane = lane_id();
    const int l16 = lane & 15, grp = lane >> 4;
    const bool act = l16 < C;
    const int cc = act ? l16 : 0;
    const bool pk = entScale == nullptr;
    const long long stride = (long long)gridDim.x * 4;
    for (long long src = (long long)blockIdx.x * 4 + uniform((int)threadIdx.x >> 6); src < sources; src += stride) {
        const int b = (int)(src / Nin);
        const int n = (int)(src - (long long)b * Nin);
        const float* __restrict__ gob = gradOutput + (size_t)b * Mout * C + cc;
        const int* __restrict__ offb = offsets + (size_t)b * (Nin + 1);
        const int e0 = offb[n], e1 = offb[n + 1];                  // (entries of cloud b start at b * Mout * K: see graph.hip)
        float acc0 = 0.f, acc1 = 0.f;
        for (int ec = e0; ec < e1; ec += 64) {                     // wave-uniform trips
            const int e = ec + lane;
            const bool mine = e < e1;
            const int wk = mine ? entKey[e] : 0;
            const int my_m = tg_key(wk, pk);
            float my_s = 0.f;
            if (mine) my_s = pk ? tg_packed_scale(wk) : entScale[e];
            const int left = e1 - (ec + 16 * grp);                 // edges of this group in this trip
#pragma unroll
            for (int j = 0; j < 16; j += 2) {
                const int m0 = __shfl(my_m, j, 16), m1 = __shfl(my_m, j + 1, 16);
                const float s0 = __shfl(my_s, j, 16), s1 = __shfl(my_s, j + 1, 16);
                // (entries past the list have key 0 — a valid row — and scale 0, and are skipped)
                if (j < left) acc0 = fmaf(gob[(size_t)m0 * C], s0, acc0);
                if (j + 1 < left) acc1 = fmaf(gob[(size_t)m1 * C], s1, acc1);
            }
        }
        float s = acc0 + acc1;
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (act && grp == 0) gradInput[(size_t)src * C + l16] = s;
    }
}

// ---- the host side: every entry computes its plan (pool_plan.hpp), answers what the plan refuses, and launches what it says ----

// The status and message of a call the plan refuses: the entries and the plan query answer alike
static int pool_refusal(const PoolPlan& p, const char* who, int op, int B, int Nin, int Mout, int C, int K, int F)
{
    if (p.bad == kPoolBadDims) {
        if (op == kPoolOpFwd) set_error("%s: bad dims B=%d N=%d M=%d C=%d K=%d", who, B, Nin, Mout, C, K);
        else if (op == kPoolOpSumGradT) set_error("%s: bad dims B=%d N=%d M=%d C=%d", who, B, Nin, Mout, C);
        else if (op == kPoolOpMaxGradRows) set_error("MaxPool3dGrad: bad dims B=%d N=%d M=%d C=%d F=%d", B, Nin, Mout, C, F);
        else if (op == kPoolOpNarrow) set_error("interpolate_narrow: bad dims B=%d N=%d M=%d C=%d K=%d", B, Mout, Nin, C, K);
        else if (op == kPoolOpNarrowGradT) set_error("interpolate_narrow_grad_t: bad dims B=%d N=%d M=%d C=%d", B, Nin, Mout, C);
        else set_error("MaxPool3dGrad: bad dims B=%d N=%d M=%d C=%d", B, Nin, Mout, C);
        return SPH3D_EINVAL;
    }
    SPH3D_REQUIRE(p.bad != kPoolBadSegments, "MaxPool3dGrad: N=%d sources of F=%d segments exceed the offsets' index range", Nin, F);
    SPH3D_REQUIRE(p.bad != kPoolBadBatch, "MaxPool3dGrad: batch %d exceeds the grid's second dimension", B);
    if (p.bad == kPoolWide) {
        set_error("%s: rows of at most 16 channels (got C=%d)", op == kPoolOpNarrow ? "interpolate_narrow" : "interpolate_narrow_grad_t", C);
        return SPH3D_EUNSUPPORTED;
    }
    SPH3D_REQUIRE(p.bad != kPoolBadGrid, "%s: B=%d N=%d M=%d need more than 2^31 - 1 workgroups", who, B, Nin, Mout);
    return SPH3D_OK;
}

template <Mode MODE>
static int launch_fwd(const char* who, int B, int Nin, int Mout, int C, int K,
                      const int* nn_index, const int* nn_count, const float* input, const float* weight,
                      float* output, int* max_index, hipStream_t st)
{
    const PoolPlan p = pool_plan(kPoolOpFwd, B, Nin, Mout, C, K, 0);
    int rc = pool_refusal(p, who, kPoolOpFwd, B, Nin, Mout, C, K, 0);
    if (rc || p.kernel == kPoolNone) return rc;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3((unsigned)p.block), 0, st, B, Nin, Mout, C, K, (int)p.parts,
                           nn_index, nn_count, input, weight, output, max_index, (int)p.ppwg);
    };
    if (p.kernel == kPoolFwdHalf) go(gather_fwd_half<MODE>);
    else if (p.V == 4) go(gather_fwd<MODE, 4>);
    else go(gather_fwd<MODE, 1>);
    return check_launch(who);
}

static int launch_bwd_t(const char* who, int B, int Nin, int Mout, int C,
                        const int* offsets, const int* ent_key, const float* ent_scale,
                        const float* grad_output, float* grad_input, hipStream_t st)
{
    const PoolPlan p = pool_plan(kPoolOpSumGradT, B, Nin, Mout, C, 0, 0);
    int rc = pool_refusal(p, who, kPoolOpSumGradT, B, Nin, Mout, C, 0, 0);
    if (rc || p.kernel == kPoolNone) return rc;
    const dim3 grid((unsigned)p.grid), block((unsigned)p.block);
    if (p.kernel == kPoolBwdTSplit) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, B, Nin, Mout, C, offsets, ent_key, ent_scale, grad_output, grad_input);
        };
        if (p.V == 4) go(gather_bwd_t_split<4>);
        else go(gather_bwd_t_split<1>);
    } else {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, B, Nin, Mout, C, (int)p.parts, offsets, ent_key, ent_scale, grad_output,
                               grad_input);
        };
        if (p.V == 4) go(gather_bwd_t<4>);
        else go(gather_bwd_t<1>);
    }
    return check_launch(who);
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_pool3d_plan(int op, int B, int Nin, int Mout, int C, int K, int F, long long* out)
{
    const PoolPlan p = pool_plan(op, B, Nin, Mout, C, K, F);
    SPH3D_REQUIRE(p.bad != kPoolBadOp, "sph3d_pool3d_plan: op %d is none of SPH3D_POOL_FWD .. SPH3D_POOL_NARROW_GRAD_T", op);
    int rc = pool_refusal(p, "sph3d_pool3d_plan", op, B, Nin, Mout, C, K, F);
    if (rc) return rc;
    SPH3D_REQUIRE(out != nullptr, "sph3d_pool3d_plan: out is NULL");
    static_assert(offsetof(PoolPlan, bad) == SPH3D_POOL_PLAN_FIELDS * sizeof(long long), "the plan starts with the documented fields, in their order");
    static_assert(kPoolOpFwd == SPH3D_POOL_FWD && kPoolOpSumGradT == SPH3D_POOL_SUM_GRAD_T && kPoolOpMaxGrad == SPH3D_POOL_MAX_GRAD &&
                      kPoolOpMaxGradT == SPH3D_POOL_MAX_GRAD_T && kPoolOpMaxGradRows == SPH3D_POOL_MAX_GRAD_ROWS &&
                      kPoolOpNarrow == SPH3D_POOL_NARROW && kPoolOpNarrowGradT == SPH3D_POOL_NARROW_GRAD_T,
                  "the ops as the header numbers them");
    static_assert(kPoolNone == SPH3D_POOL_KERNEL_NONE && kPoolFwdHalf == SPH3D_POOL_KERNEL_FWD_HALF && kPoolFwd == SPH3D_POOL_KERNEL_FWD &&
                      kPoolBwdT == SPH3D_POOL_KERNEL_BWD_T && kPoolBwdTSplit == SPH3D_POOL_KERNEL_BWD_T_SPLIT &&
                      kPoolMaxBwd == SPH3D_POOL_KERNEL_MAX_BWD && kPoolMaxBwdT == SPH3D_POOL_KERNEL_MAX_BWD_T &&
                      kPoolMaxBwdRows == SPH3D_POOL_KERNEL_MAX_BWD_ROWS && kPoolNarrowFwd == SPH3D_POOL_KERNEL_NARROW_FWD &&
                      kPoolNarrowBwdT == SPH3D_POOL_KERNEL_NARROW_BWD_T,
                  "the kernels as the header numbers them");
    memcpy(out, &p, SPH3D_POOL_PLAN_FIELDS * sizeof(long long));
    return SPH3D_OK;
}

extern "C" int sph3d_max_pool3d(int B, int N, int M, int C, int K, const int* nn_index, const int* nn_count,
                                const float* input, float* output, int* max_index, sph3d_stream_t stream)
{
    return launch_fwd<Mode::Max>("sph3d_max_pool3d", B, N, M, C, K, nn_index, nn_count, input, nullptr, output,
                                 max_index, as_stream(stream));
}

extern "C" int sph3d_max_pool3d_grad(int B, int N, int M, int C, const int* max_index, const float* grad_output,
                                     float* grad_input, sph3d_stream_t stream)
{
    const PoolPlan p = pool_plan(kPoolOpMaxGrad, B, N, M, C, 0, 0);
    if (p.bad != kPoolBadDims && deterministic_on()) {
        set_error("MaxPool3dGrad: deterministic mode is on and the scatter form adds with float atomics; use sph3d_max_pool3d_grad_t "
                  "on the transposed pooling graph");
        return SPH3D_EUNSUPPORTED;
    }
    int rc = pool_refusal(p, "sph3d_max_pool3d_grad", kPoolOpMaxGrad, B, N, M, C, 0, 0);
    if (rc || p.zero_bytes == 0) return rc;
    hipStream_t st = as_stream(stream);
    rc = zero_async(grad_input, (size_t)p.zero_bytes, st, "sph3d_max_pool3d_grad");
    if (rc || p.kernel == kPoolNone) return rc;
    hipLaunchKernelGGL(maxpool_bwd, dim3((unsigned)p.grid, (unsigned)p.grid_y), dim3((unsigned)p.block), 0, st, B, N, M, C, max_index,
                       grad_output, grad_input);
    return check_launch("sph3d_max_pool3d_grad");
}

extern "C" int sph3d_max_pool3d_grad_t(int B, int N, int M, int C, const int* offsets, const int* ent_key, const int* nn_count,
                                       const int* max_index, const float* grad_output, const float* addend, float* grad_input,
                                       sph3d_stream_t stream)
{
    const PoolPlan p = pool_plan(kPoolOpMaxGradT, B, N, M, C, 0, 0);
    int rc = pool_refusal(p, "sph3d_max_pool3d_grad_t", kPoolOpMaxGradT, B, N, M, C, 0, 0);
    if (rc || p.kernel == kPoolNone) return rc;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3((unsigned)p.block), 0, as_stream(stream), B, N, M, C, (int)p.parts,
                           (int)p.ppwg, offsets, ent_key, nn_count, max_index, grad_output, addend, grad_input);
    };
    if (p.V == 4) go(maxpool_bwd_t<4>);
    else go(maxpool_bwd_t<1>);
    return check_launch("sph3d_max_pool3d_grad_t");
}

extern "C" int sph3d_max_pool3d_grad_rows(int B, int N, int M, int C, int F, const int* offsets, const int* ent_key, const int* first,
                                          const int* next, const int* nn_count, const int* max_index, const float* grad_output,
                                          const float* addend, float* grad_input, sph3d_stream_t stream)
{
    const PoolPlan p = pool_plan(kPoolOpMaxGradRows, B, N, M, C, 0, F);
    int rc = pool_refusal(p, "sph3d_max_pool3d_grad_rows", kPoolOpMaxGradRows, B, N, M, C, 0, F);
    if (rc || p.kernel == kPoolNone) return rc;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3((unsigned)p.block), 0, as_stream(stream), B, N, M, C, F, (int)p.parts,
                           (int)p.ppwg, offsets, ent_key, first, next, nn_count, max_index, grad_output, addend, grad_input);
    };
    if (p.V == 4) go(maxpool_bwd_rows<4>);
    else go(maxpool_bwd_rows<1>);
    return check_launch("sph3d_max_pool3d_grad_rows");
}

extern "C" int sph3d_avg_pool3d(int B, int N, int M, int C, int K, const int* nn_index, const int* nn_count,
                                const float* input, float* output, sph3d_stream_t stream)
{
    return launch_fwd<Mode::Avg>("sph3d_avg_pool3d", B, N, M, C, K, nn_index, nn_count, input, nullptr, output,
                                 nullptr, as_stream(stream));
}

// ---- gradients: transposed-graph entry point + the reference-surface wrappers that build the transpose ----

// grad_input[B,Nin,C] = gather over in-edges of grad_output[B,Mout,C] * scale
extern "C" int sph3d_scatter_grad_t(int B, int Nin, int Mout, int C, const int* offsets, const int* ent_key,
                                    const float* ent_scale, const float* grad_output, float* grad_input,
                                    sph3d_stream_t stream)
{
    return launch_bwd_t("sph3d_scatter_grad_t", B, Nin, Mout, C, offsets, ent_key, ent_scale, grad_output, grad_input,
                        as_stream(stream));
}

extern "C" size_t sph3d_scatter_grad_workspace(int B, int N, int M, int K) { return tg_layout(nullptr, B, N, M, K, 1).bytes; }

static int grad_via_transpose(const char* who, int B, int Nin, int Mout, int C, int K, const int* nn_index,
                              const int* nn_count, const float* weight, const float* grad_output, float* grad_input,
                              void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B >= 0 && Nin > 0 && Mout >= 0 && C > 0 && K > 0, "%s: bad dims B=%d N=%d M=%d C=%d K=%d", who, B,
                  Nin, Mout, C, K);
    if (B == 0) return SPH3D_OK;
    const TgLayout t = tg_layout(workspace, B, Nin, Mout, K, 1);          // one bin; the list of active bins is not asked for
    if (workspace == nullptr || workspace_bytes < t.bytes) {
        set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, t.bytes);
        return SPH3D_EWORKSPACE;
    }
    int rc = sph3d_graph_transpose(B, Nin, Mout, K, 1, nn_index, nn_count, nullptr, weight, t.offsets, t.key, t.scale, nullptr,
                                   t.scratch, t.scratch_bytes, stream);
    if (rc) return rc;
    return launch_bwd_t(who, B, Nin, Mout, C, t.offsets, t.key, t.scale, grad_output, grad_input, as_stream(stream));
}

extern "C" int sph3d_avg_pool3d_grad(int B, int N, int M, int C, int K, const int* nn_index, const int* nn_count,
                                     const float* grad_output, float* grad_input,
                                     void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    return grad_via_transpose("sph3d_avg_pool3d_grad", B, N, M, C, K, nn_index, nn_count, nullptr, grad_output,
                              grad_input, workspace, workspace_bytes, stream);
}

// un-pooling: the reference's N is the fine (output) count and M the coarse (input) count
extern "C" int sph3d_mean_interpolate(int B, int N, int M, int C, int K, const int* nn_index, const int* nn_count,
                                      const float* input, float* output, sph3d_stream_t stream)
{
    return launch_fwd<Mode::Avg>("sph3d_mean_interpolate", B, /*Nin=*/M, /*Mout=*/N, C, K, nn_index, nn_count, input,
                                 nullptr, output, nullptr, as_stream(stream));
}

extern "C" int sph3d_mean_interpolate_grad(int B, int N, int M, int C, int K, const int* nn_index,
                                           const int* nn_count, const float* grad_output, float* grad_input,
                                           void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    return grad_via_transpose("sph3d_mean_interpolate_grad", B, /*Nin=*/M, /*Mout=*/N, C, K, nn_index, nn_count, nullptr,
                              grad_output, grad_input, workspace, workspace_bytes, stream);
}

extern "C" int sph3d_weighted_interpolate(int B, int N, int M, int C, int K, const int* nn_index,
                                          const int* nn_count, const float* input, const float* weight,
                                          float* output, sph3d_stream_t stream)
{
    return launch_fwd<Mode::Weighted>("sph3d_weighted_interpolate", B, M, N, C, K, nn_index, nn_count, input, weight,
                                      output, nullptr, as_stream(stream));
}

// ---- interpolation of narrow (projected) rows ----
extern "C" int sph3d_interpolate_narrow_supported(int C) { return (C >= 1 && C <= kPoolNarrowMaxC) ? 1 : 0; }

extern "C" int sph3d_interpolate_narrow(int B, int N, int M, int C, int K, const int* nn_index, const int* nn_count,
                                        const float* input, const float* weight, const float* base, float* output,
                                        sph3d_stream_t stream)
{
    const PoolPlan p = pool_plan(kPoolOpNarrow, B, /*Nin=*/M, /*Mout=*/N, C, K, 0);
    int rc = pool_refusal(p, "sph3d_interpolate_narrow", kPoolOpNarrow, B, M, N, C, K, 0);
    if (rc || p.kernel == kPoolNone) return rc;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3((unsigned)p.block), 0, as_stream(stream), (long long)B * N, N, M, C, K,
                           nn_index, nn_count, input, weight, base, output);
    };
    if (weight != nullptr) go(narrow_interp_fwd<true>);
    else go(narrow_interp_fwd<false>);
    return check_launch("sph3d_interpolate_narrow");
}

extern "C" int sph3d_interpolate_narrow_grad_t(int B, int Nin, int Mout, int C, const int* offsets, const int* ent_key,
                                               const float* ent_scale, const float* grad_output, float* grad_input,
                                               sph3d_stream_t stream)
{
    const PoolPlan p = pool_plan(kPoolOpNarrowGradT, B, Nin, Mout, C, 0, 0);
    int rc = pool_refusal(p, "sph3d_interpolate_narrow_grad_t", kPoolOpNarrowGradT, B, Nin, Mout, C, 0, 0);
    if (rc || p.kernel == kPoolNone) return rc;
    hipLaunchKernelGGL(narrow_interp_bwd_t, dim3((unsigned)p.grid), dim3((unsigned)p.block), 0, as_stream(stream), (long long)B * Nin, Nin,
                       Mout, C, offsets, ent_key, ent_scale, grad_output, grad_input);
    return check_launch("sph3d_interpolate_narrow_grad_t");
}

extern "C" int sph3d_weighted_interpolate_grad(int B, int N, int M, int C, int K, const int* nn_index,
                                               const int* nn_count, const float* grad_output, const float* weight,
                                               float* grad_input, void* workspace, size_t workspace_bytes,
                                               sph3d_stream_t stream)
{
    return grad_via_transpose("sph3d_weighted_interpolate_grad", B, M, N, C, K, nn_index, nn_count, weight, grad_output,
                              grad_input, workspace, workspace_bytes, stream);
}

