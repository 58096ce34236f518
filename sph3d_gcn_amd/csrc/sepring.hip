// sepring.hip — the separable spherical convolution layer as ONE barrier-free kernel, training and inference, gfx950
// ("BN stats as a side reduction ... to remove the [B,M,C*r] intermediate" of utils/sph3gcn_util.py:134-161).
//
//     depthwise_conv3d (tf_conv3d_gpu.cu:7-29)  ->  tf.matmul with the pointwise weights  (+ biases)
//       training : raw product y, the depthwise tensor (the weight gradient's operand: written, never re-read in forward) and
//                  per-column partial sums of elu(y), elu(y)^2 in the layout sph3d_elu_bn_forward_partials consumes
//       inference: -> ELU -> per-channel affine (batch norm with the moving statistics), depthwise tensor never written
//
// Why a second formulation next to sepconv.hip: there the 16 waves of a CU meet at a barrier per 32-point tile, gather and
// product of a wave alternate inside the barrier interval, and the measured layer time is the SUM of the gather kernel and the
// product (298 us against 205 + 85 at level 0): a wave's gather takes 10 .. 64 neighbours, the barrier waits for the slowest.
// Here nothing waits for anything but its own data:
//   * the workgroup's points go through ONE claim counter in LDS; whichever wave is free claims the next point, gathers its
//     neighbour rows exactly like dwconv_fwd_multi (conv3d.hip) and writes the point's C*r depthwise outputs into a row of a
//     RING of 16-point row blocks in LDS (and, training, to HBM: 16 B per lane, one 1-KB row);
//   * a row block whose 16 rows are in (`filled` counter) is multiplied with the pointwise weights by the waves that own its
//     column blocks — W columns RESIDENT IN REGISTERS for the whole launch (v_mfma_f32_16x16x4_f32, four independent chains) —
//     whenever those waves come by: before claiming their next point, or while they wait for a ring slot;
//   * a ring slot is reused when all column-block owners have read it (`consumed` counter).
// So a wave in its 2048 cycles of MFMA shares a SIMD with three waves waiting for feature rows: the product hides in the
// gather's memory latency.  Forward progress: points are claimed in order, the oldest unfinished row block always has a free
// slot, and every waiting wave multiplies what is ready — no wave ever holds something another one needs.  LDS operations of
// one wave execute in order, so "row written, then counter raised" needs no fence, only a compiler barrier.
// Spins are bounded: a wave that polls ~2^22 times raises a device flag and the workgroup drains (results wrong, no hang);
// sph3d_separable_conv3d_ring_failures() reads the flag (tests).
#include "sepconv.hpp"

namespace sph3d {

constexpr int kSrSpinLimit = 1 << 22;

__device__ int g_sr_fail = 0;

__device__ __forceinline__ int sr_peek(const int* p)
{
    const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return uniform(v);
}

__device__ __forceinline__ void sr_raise(int* p, int lane)
{
    // everything this wave sent to the LDS before is processed before the increment (in-order LDS queue per wave)
    asm volatile("" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
}

// R = depth multiplier; LPE = lanes per edge in the gather (16: C <= 64, 32: C <= 128); KT = ceil(C*R / 16) k-groups;
// TRAIN: outputs as described above
template <int R, int LPE, int KT, bool TRAIN>
__global__ __launch_bounds__(1024) void sepconv_ring_kernel(
    int B, int N, int M, int F, int C, int K, int Cout, int act, int NB,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ binIndex,
    const float* __restrict__ input, const float* __restrict__ dwFilter, const float* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
    float* __restrict__ output, float* __restrict__ dwOut, float* __restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NO = 4 * R;
    constexpr int SLI = 4 * LPE;                 // input channels the gather layout covers
    constexpr int KP = KT * 16;                  // padded k extent (C*R rounded up to 16)
    constexpr int LDA = KP + 4;                  // ring row stride (floats): conflict-free ds_read_b128 across rows
    constexpr int RBF = kSrRows * LDA;           // floats per row block
    float* lfilt = lds;                                          // [F + 1][R][SLI]
    float* ring = lds + (size_t)(F + 1) * SLI * R;               // [NB][16][LDA]
    int* ctrl = reinterpret_cast<int*>(ring + (size_t)NB * RBF); // [0] claim counter, [1] abort, [2 .. 2+NB) filled, [2+NB .. 2+2NB) consumed
    int* filled = ctrl + 2;
    int* consumed = ctrl + 2 + NB;
    const int CR = C * R;
    const int tid = (int)threadIdx.x;
    const int wave = uniform(tid >> 6);
    const int lane = lane_id();

    sep_load_filter<R, SLI>(lfilt, dwFilter, F, CR, tid);
    // ring columns beyond C*R (k padding) stay zero for the whole launch
    for (int e = tid; e < NB * RBF; e += kSepWaves * 64) ring[e] = 0.f;
    for (int e = tid; e < 2 + 2 * NB; e += kSepWaves * 64) ctrl[e] = 0;

    // ---- this wave's column block of the product; its W columns in registers ----
    const int ncb = Cout >> 4;                                   // column blocks (<= 16)
    const int G = kSepWaves / ncb;                                // wave groups: group g multiplies the row blocks j = g (mod G)
    const int grp = wave / ncb, cb = wave - grp * ncb;
    const bool gemm_wave = grp < G;
    const int i16 = lane & 15, kq = lane >> 4;
    float wreg[KT][4];
    sep_load_w<KT>(wreg, W, CR, Cout, cb, i16, kq, gemm_wave);
    const int col = cb * 16 + i16;
    const float bv = (gemm_wave && bias != nullptr) ? bias[col] : 0.f;
    const float sc = (!TRAIN && gemm_wave && scale != nullptr) ? scale[col] : 1.f;
    const float sh = (!TRAIN && gemm_wave && shift != nullptr) ? shift[col] : 0.f;
    float sz = 0.f, sq = 0.f;                                    // TRAIN: this lane's share of sum elu(y), sum elu(y)^2 of column `col`
    __syncthreads();                                             // the only barrier of the kernel

    // ---- row blocks of this workgroup: a contiguous range of the row blocks of its XCD's clouds ----
    const int rpc = (M + kSrRows - 1) / kSrRows;                 // row blocks per cloud
    bool affine;
    int xcd, j_begin, j_end;
    sep_units(B, rpc, affine, xcd, j_begin, j_end);
    const int nrb = j_end - j_begin;
    const int npts = nrb * kSrRows;

    const int g = lane / LPE, li = lane - g * LPE;
    const bool actl = li * 4 < C;
    const int cic = actl ? li * 4 : 0;
    const unsigned cicb = (unsigned)cic * 4u, rowb = (unsigned)C * 4u;
    const char* lfb = reinterpret_cast<const char*>(lfilt);

    // ---- gather of one claimed point p (local index) into its ring row ----
    auto gather_point = [&](int p, int s) {
        const int j = j_begin + (p >> 4);
        const int cl = j / rpc, rbi = j - cl * rpc;
        const int b = affine ? xcd + 8 * cl : cl;
        const int m = rbi * kSrRows + (p & 15);
        const char* inb = reinterpret_cast<const char*>(input + (size_t)b * N * C);
        const size_t row = (size_t)b * M + (m < M ? m : 0);
        const SepSums<R> sums = sep_gather<R, LPE>(lane, g, inb, m < M, row, K, F, nnCount, nnIndex, binIndex, lfb, rowb, cicb, cicb);
        const int cnt = sums.cnt;
        float acc[NO];
        const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;            // rows past M / empty rows: zeros
#pragma unroll
        for (int v = 0; v < NO; v++) acc[v] = sums.v[v] * inv;
        if (actl && g == 0) {
            float* ap = ring + (size_t)s * RBF + (size_t)(p & 15) * LDA + li * 4 * R;
#pragma unroll
            for (int q = 0; q < R; q++)
                *reinterpret_cast<float4*>(ap + 4 * q) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        }
        sr_raise(&filled[s], lane);
        if (TRAIN && m < M && actl && g == 0) {
            // the depthwise tensor, for the weight gradient (after the ring row: the product does not wait for HBM stores)
            float* op = dwOut + row * CR + (size_t)li * 4 * R;
#pragma unroll
            for (int q = 0; q < R; q++)
                *reinterpret_cast<float4*>(op + 4 * q) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        }
    };

    // ---- product of local row block jl (ring slot s) with this wave's W columns ----
    auto product_block = [&](int jl, int s) {
        const SepChains c = sep_product<KT>(ring + (size_t)s * RBF + (size_t)i16 * LDA + 4 * kq, wreg);
        // the slot's rows are in registers / the matrix pipe: hand the slot back before the epilogue's HBM stores
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        sr_raise(&consumed[s], lane);
        const sep_f32x4 d = (c.d0 + c.d1) + (c.d2 + c.d3);
        const int j = j_begin + jl;
        const int cl = j / rpc, rbi = j - cl * rpc;
        const int b = affine ? xcd + 8 * cl : cl;
        // D layout of 16x16x4: lane holds rows 4*(lane/16) + r, r < 4, of column lane % 16
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
            const int m = rbi * kSrRows + 4 * kq + r4;
            if (m < M) {
                float y = d[r4] + bv;
                if (TRAIN) {
                    output[((size_t)b * M + m) * Cout + col] = y;
                    const float z = elu1(y);
                    sz += z;
                    sq = fmaf(z, z, sq);
                } else {
                    if (act == 1) y = elu1(y);
                    output[((size_t)b * M + m) * Cout + col] = fmaf(y, sc, sh);
                }
            }
        }
    };

    // ---- the loop: multiply what is ready, else claim and gather a point, else wait ----
    int my_j = gemm_wave ? grp : 0x7fffffff;       // next local row block this wave multiplies
    int my_s = gemm_wave ? grp % NB : 0, my_e = gemm_wave ? grp / NB : 0;       // its ring slot and epoch
    bool exhausted = npts == 0;
    int spins = 0;
    auto try_product = [&]() -> bool {
        if (my_j >= nrb) return false;
        if (sr_peek(&filled[my_s]) < kSrRows * (my_e + 1)) return false;
        product_block(my_j, my_s);
        my_j += G;
        my_s += G;
        while (my_s >= NB) { my_s -= NB; my_e++; }
        return true;
    };
    auto spin = [&]() -> bool {                     // -> true: give up (the launch is broken; drain)
        __builtin_amdgcn_s_sleep(1);
        if (++spins > kSrSpinLimit) {
            if (lane == 0) {
                atomicExch(&g_sr_fail, 1);
                __hip_atomic_store(&ctrl[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            return true;
        }
        return (spins & 1023) == 0 && sr_peek(&ctrl[1]) != 0;
    };
    for (;;) {
        if (try_product()) continue;
        if (!exhausted) {
            int p = 0;
            if (lane == 0) p = __hip_atomic_fetch_add(&ctrl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            p = uniform(p);
            if (p >= npts) {
                exhausted = true;
                continue;
            }
            const int jl = p >> 4;
            const int e = jl / NB, s = jl - e * NB;
            bool dead = false;
            while (sr_peek(&consumed[s]) < ncb * e) {          // the slot's previous row block has not been read by all its owners
                if (try_product()) continue;
                if (spin()) { dead = true; break; }
            }
            if (dead) break;
            gather_point(p, s);
            continue;
        }
        if (my_j >= nrb) break;
        if (spin()) break;
    }

    if (TRAIN && gemm_wave) {
        // partial statistics of this (workgroup, wave group): fold the four row quarters of a column, one store per column
        sz += __shfl_xor(sz, 16);
        sq += __shfl_xor(sq, 16);
        sz += __shfl_xor(sz, 32);
        sq += __shfl_xor(sq, 32);
        if (kq == 0) {
            float* sp = stats + ((size_t)blockIdx.x * G + grp) * 2 * Cout + col;
            sp[0] = sz;
            sp[Cout] = sq;
        }
    }
}

// the instantiation a plan names (sepconv.hpp: sep_launch)
SepRingKernel sepring_kernel(const SepPlan& p)
{
    return sep_with_triple(p, [&](auto R, auto L, auto KT) -> SepRingKernel {
        return p.train ? sepconv_ring_kernel<R(), L(), KT(), true> : sepconv_ring_kernel<R(), L(), KT(), false>;
    });
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_separable_conv3d_train_supported(int N, int F, int C, int r, int K, int Cout)
{
    return sep_plan(true, 0, N, 0, F, C, r, K, Cout).kernel != kSepNone;
}

extern "C" int sph3d_separable_conv3d_train_blocks(int Cout)
{
    return sep_plan(true, 0, 1, 0, 1, 4, 1, 1, Cout).stats_blocks;      // Cout alone decides: the plan of the narrowest layer
}

extern "C" int sph3d_separable_conv3d_train(int B, int N, int M, int F, int C, int r, int K, int Cout,
                                            const int* nn_index, const int* nn_count, const int* bin_index,
                                            const float* input, const float* depthwise_filter, const float* pointwise_weights,
                                            const float* bias, float* depthwise_output, float* y, float* partial,
                                            sph3d_stream_t stream)
{
    if (int rc = sep_check_dims("SeparableConv3dTrain", B, N, M, F, C, K, Cout)) return rc;
    const SepPlan p = sep_plan(true, B, N, M, F, C, r, K, Cout);
    if (p.kernel == kSepNone) {
        set_error("SeparableConv3dTrain: shape C=%d r=%d Cout=%d F=%d not covered (C %% 4 == 0, C <= 128, C*r <= 256, "
                  "Cout in {16, 32, 64, 128, 256}, r in {1, 2})", C, r, Cout, F);
        return SPH3D_EUNSUPPORTED;
    }
    SPH3D_REQUIRE(depthwise_output != nullptr && y != nullptr && partial != nullptr, "SeparableConv3dTrain: NULL output");
    return sep_launch(p, {B, N, M, F, C, K, Cout, 0, nn_index, nn_count, bin_index, input, depthwise_filter, pointwise_weights, bias, nullptr,
                          nullptr, y, depthwise_output, partial}, as_stream(stream));
}

extern "C" int sph3d_separable_conv3d_ring_failures(void)
{
    int v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_sr_fail), sizeof(int), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}
