// sepconv.hip — fused separable spherical convolution for inference, gfx950 (second half).
//
// One kernel for the whole layer of utils/sph3gcn_util.py:134-161 in inference mode:
//     depthwise_conv3d (tf_conv3d_gpu.cu:7-29)  ->  tf.matmul with the pointwise weights  ->  + biases  ->  ELU  ->
//     batch norm with the moving statistics (an affine map per output channel)
// The [B, M, C*r] depthwise tensor never leaves the CU: a persistent 16-wave workgroup per CU takes tiles of 32 output
// points; every wave gathers two of them exactly like dwconv_fwd_multi (conv3d.hip: 16 / 32 lanes per edge, packed id | bin
// hand-over, LDS filter table) and writes the 32 x C*r tile to LDS; then the 16 waves multiply the tile with the pointwise
// weights on the matrix cores — v_mfma_f32_16x16x4_f32, one 16 x 16 output block per wave, its 16 columns of W
// (C*r x 16 floats = 64 VGPRs at C*r = 256) RESIDENT IN REGISTERS for the whole launch — and apply the epilogue.
// In training the depthwise tensor is the weight gradient's operand and has to be written anyway, so this
// path is taken when no gradient is recorded.  Shapes outside C <= 128, C*r <= 256, Cout <= 128 — every deeper layer of the
// S3DIS / ShapeNet plans — run sepconv_general_kernel below (accumulators resident, W streamed per k slice).
//
// fp32 MFMA is exact fp32 FMA arithmetic; results differ from the separate kernels by summation order only (k-order of the product:
// sepconv.hpp, sep_load_w).  The launch choice of this file's two kernels and of sepring.hip's is sepconv.hpp's sep_plan; the one
// launcher and the host-only query are at the end of this file.
#include "sepconv.hpp"

namespace sph3d {

// R = depth multiplier; LPE = lanes per edge in the gather phase (16: C <= 64, 32: C <= 128); KT = ceil(C*R / 16) k-groups
template <int R, int LPE, int KT>
__global__ __launch_bounds__(1024) void sepconv_fused_kernel(
    int B, int N, int M, int F, int C, int K, int Cout, int act,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ binIndex,
    const float* __restrict__ input, const float* __restrict__ dwFilter, const float* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
    float* __restrict__ output)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SLI = 4 * LPE;                 // input channels the gather layout covers
    constexpr int KP = KT * 16;                  // padded k extent (C*R rounded up to 16)
    constexpr int LDA = KP + 4;                  // A-tile row stride (floats): conflict-free ds_read_b128 across rows
    float* lfilt = lds;                                          // [F + 1][R][SLI]
    float* atile = lds + (size_t)(F + 1) * SLI * R;              // [2][kScTile][LDA]: double buffered
    const int CR = C * R;
    const int tid = (int)threadIdx.x;
    const int wave = uniform(tid >> 6);
    const int lane = lane_id();

    sep_load_filter<R, SLI>(lfilt, dwFilter, F, CR, tid);
    // columns of the A tile beyond C*R (k padding) stay zero for the whole launch
    for (int e = tid; e < 2 * kScTile * LDA; e += kSepWaves * 64) atile[e] = 0.f;

    // ---- this wave's block of the product: rows rb*16.., columns cb*16..; its W columns in registers ----
    const int ncb = Cout >> 4;
    const int rb = wave / ncb, cb = wave - rb * ncb;
    const bool gemm_wave = rb < (kScTile / 16);
    const int i16 = lane & 15, kq = lane >> 4;
    float wreg[KT][4];
    sep_load_w<KT>(wreg, W, CR, Cout, cb, i16, kq, gemm_wave);
    const int col = cb * 16 + i16;
    const float bv = (gemm_wave && bias != nullptr) ? bias[col] : 0.f;
    const float sc = (gemm_wave && scale != nullptr) ? scale[col] : 1.f;
    const float sh = (gemm_wave && shift != nullptr) ? shift[col] : 0.f;
    __syncthreads();

    // ---- tiles of this workgroup: contiguous range of the tiles of its XCD's clouds ----
    const int tpc = (M + kScTile - 1) / kScTile;                  // tiles per cloud
    bool affine;
    int xcd, f_begin, f_end;
    sep_units(B, tpc, affine, xcd, f_begin, f_end);

    const int g = lane / LPE, li = lane - g * LPE;
    const bool actl = li * 4 < C;
    const int cic = actl ? li * 4 : 0;
    const unsigned cicb = (unsigned)cic * 4u, rowb = (unsigned)C * 4u;
    const char* lfb = reinterpret_cast<const char*>(lfilt);

    // ---- software pipeline over the tiles: in iteration `it` the workgroup gathers tile `it` into A buffer it & 1 and
    // multiplies tile it - 1 out of the other buffer; half of the waves of every SIMD (wave / 4 odd) run the product first
    // and the gather second, so that the matrix pipe (64 x 32-cycle MFMAs per wave and tile: the product alone is
    // MFMA-rate bound at the fp32 peak) and the gather's VALU / LDS / VMEM work overlap inside a SIMD.
    auto gather_tile = [&](int b, int m0, float* abuf) {
        const char* inb = reinterpret_cast<const char*>(input + (size_t)b * N * C);
#pragma unroll 1
        for (int h = 0; h < 2; h++) {                 // wave w takes points m0 + w and m0 + w + 16
            const int p = wave + kSepWaves * h;
            const int m = m0 + p;
            const size_t row = (size_t)b * M + m;
            const SepSums<R> sums = sep_gather<R, LPE>(lane, g, inb, m < M, row, K, F, nnCount, nnIndex, binIndex, lfb, rowb, cicb, cicb);
            const int cnt = sums.cnt;
            const float* acc = sums.v;
            if (actl && g == 0) {
                const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;        // rows past M / empty rows: zeros
                float* ap = abuf + (size_t)p * LDA + li * 4 * R;
#pragma unroll
                for (int q = 0; q < R; q++)
                    *reinterpret_cast<float4*>(ap + 4 * q) =
                        make_float4(acc[4 * q] * inv, acc[4 * q + 1] * inv, acc[4 * q + 2] * inv, acc[4 * q + 3] * inv);
            }
        }
    };
    auto product_tile = [&](int b, int m0, const float* abuf) {
        if (!gemm_wave) return;
        const SepChains c = sep_product<KT>(abuf + (size_t)(rb * 16 + i16) * LDA + 4 * kq, wreg);
        const sep_f32x4 d = (c.d0 + c.d1) + (c.d2 + c.d3);
        // D layout of 16x16x4: lane holds rows 4*(lane/16) + r, r < 4, of column lane % 16
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
            const int m = m0 + rb * 16 + 4 * kq + r4;
            if (m < M) {
                float y = d[r4] + bv;
                if (act == 1) y = elu1(y);
                output[((size_t)b * M + m) * Cout + col] = fmaf(y, sc, sh);
            }
        }
    };

    const bool product_first = ((wave >> 2) & 1) != 0;
    int cl = f_begin / tpc, tl = f_begin - cl * tpc;
    int pb = 0, pm0 = 0;
    for (int it = f_begin; it <= f_end; it++) {
        const int b = affine ? xcd + 8 * cl : cl;
        const int m0 = tl * kScTile;
        float* gbuf = atile + (size_t)(it & 1) * (kScTile * LDA);
        const float* mbuf = atile + (size_t)((it & 1) ^ 1) * (kScTile * LDA);
        const bool do_g = it < f_end, do_p = it > f_begin;
        if (product_first) {
            if (do_p) product_tile(pb, pm0, mbuf);
            if (do_g) gather_tile(b, m0, gbuf);
        } else {
            if (do_g) gather_tile(b, m0, gbuf);
            if (do_p) product_tile(pb, pm0, mbuf);
        }
        __syncthreads();
        pb = b;
        pm0 = m0;
        if (++tl == tpc) { tl = 0; cl++; }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// General shapes (round 4): any layer of the S3DIS / ShapeNet plans (C up to 1024 in slices of 128 input channels, Cout up to
// 512).  The pointwise weights no longer fit a wave's registers (C*r x Cout = up to 2048 x 512 floats), so the product is
// organised the other way round: the ACCUMULATORS stay resident — wave w owns the output column blocks cb = w, w + 16 of a
// tile of TP = 16 * RBK points (RBK x 2 blocks of 16 x 16: <= 32 VGPRs) across the whole k range — and the layer is walked
// slice by slice: filter slice -> LDS, the 16 waves gather the slice's depthwise outputs of the tile's points into the
// LDS A tile [TP][SLI*R] (same gather as above), then every wave multiplies the tile with ITS columns of the slice's
// k-rows of W, fetched from global memory / L2 as they are needed (a lane's four B values of a t are four 4-byte loads of
// 16 consecutive columns; each fragment feeds RBK row blocks).  Per tile W is read once (C*r*Cout*4 B from L2): the kernel
// trades the [B, M, C*r] depthwise tensor's HBM round trip (write + read) for L2 reads of W per tile.
// ------------------------------------------------------------------------------------------------------------------
template <int R, int LPE, int RBK>
__global__ __launch_bounds__(1024) void sepconv_general_kernel(
    int B, int N, int M, int F, int C, int K, int Cout, int act,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ binIndex,
    const float* __restrict__ input, const float* __restrict__ dwFilter, const float* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ scale, const float* __restrict__ shift,
    float* __restrict__ output)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SLI = 4 * LPE;                 // input channels per slice
    constexpr int KP = SLI * R;                  // k extent of a slice
    constexpr int KT = KP / 16;
    constexpr int LDA = KP + 4;
    constexpr int TP = 16 * RBK;                 // points per tile
    constexpr int PPW = (TP + kSepWaves - 1) / kSepWaves;      // points a wave gathers per tile and slice
    float* lfilt = lds;                                          // [F + 1][R][SLI]
    float* atile = lds + (size_t)(F + 1) * SLI * R;              // [TP][LDA]
    const int CR = C * R;
    const int tid = (int)threadIdx.x;
    const int wave = uniform(tid >> 6);
    const int lane = lane_id();
    const int nslices = (C + SLI - 1) / SLI;
    const int ncb = Cout >> 4;                                   // <= 32
    const int i16 = lane & 15, kq = lane >> 4;

    const int tpc = (M + TP - 1) / TP;                           // tiles per cloud
    bool affine;
    int xcd, f_begin, f_end;
    sep_units(B, tpc, affine, xcd, f_begin, f_end);

    const int g = lane / LPE, li = lane - g * LPE;
    const unsigned rowb = (unsigned)C * 4u;
    const char* lfb = reinterpret_cast<const char*>(lfilt);
    for (int e = tid; e < SLI * R; e += kSepWaves * 64) lfilt[F * (SLI * R) + e] = 0.f;      // zero filter row of padding slots

    int cl = f_begin / tpc, tl = f_begin - cl * tpc;
    for (int it = f_begin; it < f_end; it++) {
        const int b = affine ? xcd + 8 * cl : cl;
        const int m0 = tl * TP;
        sep_f32x4 d[2][RBK];
#pragma unroll
        for (int c2 = 0; c2 < 2; c2++)
#pragma unroll
            for (int rb = 0; rb < RBK; rb++) d[c2][rb] = sep_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < nslices; s++) {
            const int c0 = s * SLI;
            const int SLc = (C - c0) < SLI ? (C - c0) : SLI;             // channels of this slice (multiple of 4)
            __syncthreads();                                              // the previous slice's product is done with LDS
            // ---- filter slice -> LDS ----
            for (int e = tid * 4; e < F * SLc * R; e += kSepWaves * 64 * 4) {
                const int f = e / (SLc * R);
                const int cl4 = e - f * (SLc * R);
                const int l4 = cl4 / (4 * R), q = (cl4 >> 2) % R;
                *reinterpret_cast<float4*>(&lfilt[f * (SLI * R) + q * SLI + l4 * 4]) =
                    *reinterpret_cast<const float4*>(&dwFilter[(size_t)f * CR + (size_t)c0 * R + cl4]);
            }
            __syncthreads();
            // ---- gather: wave w takes points m0 + w + 16 h of the tile ----
            const bool actl = li * 4 < SLc;
            const unsigned cicb = (unsigned)(c0 + (actl ? li * 4 : 0)) * 4u;
            const unsigned ficb = (unsigned)(actl ? li * 4 : 0) * 4u;
            const char* inb = reinterpret_cast<const char*>(input + (size_t)b * N * C);
#pragma unroll 1
            for (int h = 0; h < PPW; h++) {
                const int p = wave + kSepWaves * h;
                if (p >= TP) break;
                const int m = m0 + p;
                const size_t row = (size_t)b * M + m;
                const SepSums<R> sums = sep_gather<R, LPE>(lane, g, inb, m < M, row, K, F, nnCount, nnIndex, binIndex, lfb, rowb, cicb, ficb);
                const int cnt = sums.cnt;
                const float* acc = sums.v;
                if (g == 0) {
                    // lanes beyond the slice's channels write zeros: k columns the product multiplies with W rows that do not exist
                    const float inv = (cnt > 0 && actl) ? 1.0f / (float)cnt : 0.f;
                    float* ap = atile + (size_t)p * LDA + li * 4 * R;
#pragma unroll
                    for (int q = 0; q < R; q++)
                        *reinterpret_cast<float4*>(ap + 4 * q) =
                            make_float4(acc[4 * q] * inv, acc[4 * q + 1] * inv, acc[4 * q + 2] * inv, acc[4 * q + 3] * inv);
                }
            }
            __syncthreads();
            // ---- product: this wave's column blocks x every row block of the tile, k rows of this slice ----
            const int kbase = c0 * R;                                    // first k row of the slice in W
#pragma unroll
            for (int c2 = 0; c2 < 2; c2++) {
                const int cb = wave + kSepWaves * c2;
                if (cb >= ncb) break;
                const float* wp = W + (size_t)kbase * Cout + cb * 16 + i16;
#pragma unroll 1
                for (int t = 0; t < KT; t++) {
                    float bw[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int k = 16 * t + 4 * kq + u;
                        bw[u] = k < SLc * R ? wp[(size_t)k * Cout] : 0.f;
                    }
                    sep_f32x4 a[RBK];
#pragma unroll
                    for (int rb = 0; rb < RBK; rb++)
                        a[rb] = *reinterpret_cast<const sep_f32x4*>(atile + (size_t)(rb * 16 + i16) * LDA + 16 * t + 4 * kq);
                    // (u outer, row blocks inner: consecutive MFMAs write different accumulators)
#pragma unroll
                    for (int u = 0; u < 4; u++)
#pragma unroll
                        for (int rb = 0; rb < RBK; rb++)
                            d[c2][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][u], bw[u], d[c2][rb], 0, 0, 0);
                }
            }
        }
        // ---- epilogue: bias -> ELU -> per-channel affine; D layout: lane holds rows 4*(lane/16) + r of column lane % 16 ----
#pragma unroll
        for (int c2 = 0; c2 < 2; c2++) {
            const int cb = wave + kSepWaves * c2;
            if (cb >= ncb) break;
            const int col = cb * 16 + i16;
            const float bv = bias != nullptr ? bias[col] : 0.f;
            const float sc = scale != nullptr ? scale[col] : 1.f;
            const float sh = shift != nullptr ? shift[col] : 0.f;
#pragma unroll
            for (int rb = 0; rb < RBK; rb++)
#pragma unroll
                for (int r4 = 0; r4 < 4; r4++) {
                    const int m = m0 + rb * 16 + 4 * kq + r4;
                    if (m < M) {
                        float y = d[c2][rb][r4] + bv;
                        if (act == 1) y = elu1(y);
                        output[((size_t)b * M + m) * Cout + col] = fmaf(y, sc, sh);
                    }
                }
        }
        if (++tl == tpc) { tl = 0; cl++; }
    }
}

// ---- the launcher: the kernel a plan names (sepconv.hpp: sep_plan).  Only the instantiations some plan reaches are compiled ---
typedef void (*SepTileKernel)(int, int, int, int, int, int, int, int, const int*, const int*, const int*, const float*, const float*,
                              const float*, const float*, const float*, const float*, float*);

static SepTileKernel sc_kernel(const SepPlan& p)
{
    if (p.kernel == kSepSmall)
        return sep_with_triple(p, [](auto R, auto L, auto KT) -> SepTileKernel { return sepconv_fused_kernel<R(), L(), KT()>; });
    // general: R in {1, 2} x LPE in {16, 32} x RBK in {1, 2, 4}
    auto with_rbk = [&](auto R, auto L) -> SepTileKernel {
        if (p.RBK == 4) return sepconv_general_kernel<R(), L(), 4>;
        if (p.RBK == 2) return sepconv_general_kernel<R(), L(), 2>;
        return p.RBK == 1 ? sepconv_general_kernel<R(), L(), 1> : nullptr;
    };
    using std::integral_constant;
    auto with_lpe = [&](auto R) -> SepTileKernel {
        if (p.LPE == 16) return with_rbk(R, integral_constant<int, 16>{});
        return p.LPE == 32 ? with_rbk(R, integral_constant<int, 32>{}) : nullptr;
    };
    if (p.R == 1) return with_lpe(integral_constant<int, 1>{});
    return p.R == 2 ? with_lpe(integral_constant<int, 2>{}) : nullptr;
}

int sep_launch(const SepPlan& p, const SepArgs& a, hipStream_t st)
{
    if (p.grid == 0) return SPH3D_OK;
    const bool ring = p.kernel == kSepRing;
    const char* who = ring ? "SeparableConv3dRing" : "SeparableConv3dFused";
    const SepRingKernel rk = ring ? sepring_kernel(p) : nullptr;
    const SepTileKernel tk = ring ? nullptr : sc_kernel(p);
    SPH3D_REQUIRE((rk != nullptr || tk != nullptr) && p.lds > 0 && (size_t)p.lds <= kSepLds,
                  "%s: no kernel for plan %d <%d,%d,%d|%d> with %d B of LDS", who, p.kernel, p.R, p.LPE, p.KT, p.RBK, p.lds);
    const int rc = ring ? launch_lds<48 * 1024>(rk, dim3(p.grid), dim3(1024), p.lds, st, who, a.B, a.N, a.M, a.F, a.C, a.K, a.Cout, a.act, p.NB,
                                                a.nn_index, a.nn_count, a.bin_index, a.input, a.dw_filter, a.W, a.bias, a.scale, a.shift,
                                                a.output, a.dw_out, a.stats)
                        : launch_lds<48 * 1024>(tk, dim3(p.grid), dim3(1024), p.lds, st, who, a.B, a.N, a.M, a.F, a.C, a.K, a.Cout, a.act,
                                                a.nn_index, a.nn_count, a.bin_index, a.input, a.dw_filter, a.W, a.bias, a.scale, a.shift,
                                                a.output);
    if (rc) return rc;
    return check_launch(ring ? "sph3d_separable_conv3d_ring"
                             : (p.kernel == kSepSmall ? "sph3d_separable_conv3d_fused" : "sph3d_separable_conv3d_fused (general)"));
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_separable_conv3d_plan(int train, int B, int N, int M, int F, int C, int r, int K, int Cout, int* out)
{
    SPH3D_REQUIRE((train | 1) == 1 && out != nullptr, "separable_conv3d_plan: train is 0 or 1, out is not NULL");
    if (int rc = sep_check_dims("separable_conv3d_plan", B, N, M, F, C, K, Cout)) return rc;
    const SepPlan p = sep_plan(train != 0, B, N, M, F, C, r, K, Cout);
    static_assert(offsetof(SepPlan, train) == SPH3D_SEP_PLAN_FIELDS * sizeof(int), "the plan starts with the documented fields, in their order");
    memcpy(out, &p, SPH3D_SEP_PLAN_FIELDS * sizeof(int));
    return SPH3D_OK;
}

extern "C" int sph3d_separable_conv3d_fused_supported(int N, int F, int C, int r, int K, int Cout)
{
    return sep_plan(false, 0, N, 0, F, C, r, K, Cout).kernel != kSepNone;
}

extern "C" int sph3d_separable_conv3d_fused(int B, int N, int M, int F, int C, int r, int K, int Cout, int act,
                                            const int* nn_index, const int* nn_count, const int* bin_index,
                                            const float* input, const float* depthwise_filter, const float* pointwise_weights,
                                            const float* bias, const float* scale, const float* shift, float* output,
                                            sph3d_stream_t stream)
{
    if (int rc = sep_check_dims("SeparableConv3dFused", B, N, M, F, C, K, Cout)) return rc;
    SPH3D_REQUIRE(act == 0 || act == 1, "SeparableConv3dFused: act must be 0 (none) or 1 (ELU), got %d", act);
    const SepPlan p = sep_plan(false, B, N, M, F, C, r, K, Cout);
    if (p.kernel == kSepNone) {
        set_error("SeparableConv3dFused: shape C=%d r=%d Cout=%d F=%d not covered (C %% 4 == 0 and C <= 128 or a multiple of 128; "
                  "Cout <= 512 in multiples of 16; r in {1, 2})", C, r, Cout, F);
        return SPH3D_EUNSUPPORTED;
    }
    // (B == 0 or M == 0: the plan's grid is 0, nothing is launched)
    return sep_launch(p, {B, N, M, F, C, K, Cout, act, nn_index, nn_count, bin_index, input, depthwise_filter, pointwise_weights, bias, scale,
                          shift, output, nullptr, nullptr}, as_stream(stream));
}
