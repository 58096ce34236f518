// condlogits.hip — the category-conditioned logits layer of the one-hot ShapeNet model (128 + 16 -> 50 parts over 65 536 points), gfx950.
//
// models/SPH3D_shapenet_onehot.py:105-119: the mlp2 output is concatenated with the mlp1 features, then with a [B, N, 16] tile of
// tf.one_hot(cls_label), and pointwise_conv3d (utils/sph3gcn_util.py:166-222) maps the 144 channels to the 50 part logits.  The
// one-hot block is no matrix operand: onehot(cat[b]) . W[K1+K2:, :] is ONE ROW of W per cloud.  So
//   forward   Y[b*P + p, :] = A1[b*P + p, :] W[0:K1] + A2[b*P + p, :] W[K1:K1+K2] + W[K1 + K2 + cat[b], :] (+ bias)
//   gradient  dT[c, :]      = sum over the clouds b with cat[b] == c, over p, of dY[b*P + p, :];   dbias = the sum over all rows
// and neither the tile, nor the [R, 144] concatenation, nor the 128-wide one in front of it is ever written.  A category outside
// [0, T) selects no row (tf.one_hot gives a zero row there).
// Forward: skinny.hip's scheme widened to NT = ceil(N / 16) <= 4 column tiles.  A wave owns 16 rows; lane (row i, k-quarter q)
// loads A[i][16t + 4q .. +3] as ONE 16-byte load per k-group t; v_mfma_f32_16x16x4_f32 (exact fp32 FMAs) multiplies it with the
// weights, which sit in registers for the whole launch (K/4 VGPRs per column tile); every column tile keeps independent
// accumulation chains.  The epilogue adds the cloud's category row, then the bias: output row ro belongs to cloud ro / P, and the
// four rows a lane holds may belong to different clouds.
// Gradient: two launches, fixed summation order, no floating-point atomics.  Stage 1: a workgroup sums the columns of one slice of
// one cloud's rows (256 / N rows per pass, read as they lie in memory) and writes one partial row; stage 2: one workgroup per
// category adds the sums of that category's clouds, b ascending, and one more workgroup adds all clouds' sums for dbias.
#include "common.hpp"

namespace sph3d {

typedef float cl_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kClMaxK = 128;             // K1 + K2
constexpr int kClKT = kClMaxK / 16;      // k-groups of 16
constexpr int kClMaxN = 64;              // four column tiles
constexpr int kClMaxT = 4096;            // categories (rows of W behind the two operand halves)

__device__ __forceinline__ cl_f32x4 cl_mfma(float a, float b, cl_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---- forward -----------------------------------------------------------------------------------------------------------------
// NT column tiles, NC accumulation chains per tile (k-slot u of the 16-byte load goes to chain u % NC)
template <int NT, int NC>
__global__ __launch_bounds__(256) void cond_nn_kernel(int R, int P, int K1, int K2, int N, int T, const float* __restrict__ A1,
                                                      const float* __restrict__ A2, const float* __restrict__ W,
                                                      const float* __restrict__ bias, const int* __restrict__ cat,
                                                      float* __restrict__ Y)
{
    const int lane = lane_id();
    const int i16 = lane & 15, kq = lane >> 4;
    const int kt1 = K1 >> 4, kt = (K1 + K2) >> 4;
    // W[16t + 4kq + u][16c + i16] for every k-group and column tile: resident for the launch (columns >= N are zero: padded
    // outputs, never stored)
    float wreg[NT][kClKT][4];
    float bv[NT];
#pragma unroll
    for (int c = 0; c < NT; c++) {
        const int col = 16 * c + i16;
#pragma unroll
        for (int t = 0; t < kClKT; t++)
#pragma unroll
            for (int u = 0; u < 4; u++) wreg[c][t][u] = (t < kt && col < N) ? W[(size_t)(16 * t + 4 * kq + u) * N + col] : 0.f;
        bv[c] = (bias != nullptr && col < N) ? bias[col] : 0.f;
    }
    const float* Wcat = W + (size_t)(K1 + K2) * N;                  // [T, N]: the category rows
    const int tiles = (R + 15) >> 4;
    const int wid = (int)blockIdx.x * 4 + uniform((int)threadIdx.x >> 6), nw = (int)gridDim.x * 4;
    for (int tile = wid; tile < tiles; tile += nw) {
        const int row = tile * 16 + i16;
        const int rowc = row < R ? row : R - 1;                     // ragged last tile: a valid row, its outputs are not stored
        const float* p1 = A1 + (size_t)rowc * K1 + 4 * kq;
        const float* p2 = A2 ? A2 + (size_t)rowc * K2 + 4 * kq : p1;
        cl_f32x4 a[kClKT];
#pragma unroll
        for (int t = 0; t < kClKT; t++) {
            if (t < kt) a[t] = *reinterpret_cast<const cl_f32x4*>(t < kt1 ? p1 + 16 * t : p2 + 16 * (t - kt1));   // wave-uniform selects
        }
        cl_f32x4 d[NT][NC];
#pragma unroll
        for (int c = 0; c < NT; c++)
#pragma unroll
            for (int h = 0; h < NC; h++) d[c][h] = cl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < kClKT; t++) {
            if (t < kt) {
#pragma unroll
                for (int c = 0; c < NT; c++) {
                    d[c][0 % NC] = cl_mfma(a[t].x, wreg[c][t][0], d[c][0 % NC]);
                    d[c][1 % NC] = cl_mfma(a[t].y, wreg[c][t][1], d[c][1 % NC]);
                    d[c][2 % NC] = cl_mfma(a[t].z, wreg[c][t][2], d[c][2 % NC]);
                    d[c][3 % NC] = cl_mfma(a[t].w, wreg[c][t][3], d[c][3 % NC]);
                }
            }
        }
        // D: lane holds rows 4*(lane/16) + r, r < 4, of column 16c + lane % 16.  Row ro is row `rem` of cloud `b`
        const int ro0 = tile * 16 + 4 * kq;
        int b = ro0 / P, rem = ro0 - b * P;
        int b_have = -1;
        float wc[NT];
#pragma unroll
        for (int c = 0; c < NT; c++) wc[c] = 0.f;
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
            const int ro = ro0 + r4;
            if (ro < R) {                                            // (so b < B)
                if (b != b_have) {
                    b_have = b;
                    const int cb = cat[b];
                    const bool in = cb >= 0 && cb < T;               // the range before the address
#pragma unroll
                    for (int c = 0; c < NT; c++) {
                        const int col = 16 * c + i16;
                        wc[c] = (in && col < N) ? Wcat[(size_t)cb * N + col] : 0.f;
                    }
                }
#pragma unroll
                for (int c = 0; c < NT; c++) {
                    const int col = 16 * c + i16;
                    float s;
                    if (NC == 4) s = (d[c][0][r4] + d[c][1 % NC][r4]) + (d[c][2 % NC][r4] + d[c][3 % NC][r4]);
                    else if (NC == 2) s = d[c][0][r4] + d[c][1 % NC][r4];
                    else s = d[c][0][r4];
                    if (col < N) Y[(size_t)ro * N + col] = (s + wc[c]) + bv[c];
                }
            }
            if (++rem == P) {
                rem = 0;
                ++b;
            }
        }
    }
}

// ---- gradient of the category rows and the bias ------------------------------------------------------------------------------
// stage 1: workgroup (slice s, cloud b) -> partial[(b * S + s) * N + col] = sum of dY[b*P + r][col] over the slice's rows r, in
// the order: thread (row lane j, col) adds rows j, j + rpp, j + 2 rpp, ... (rpp = 256 / N rows per pass: a pass reads rpp * N
// contiguous floats; eight passes' loads are issued together), then the row lanes are added j ascending
__global__ __launch_bounds__(256) void cond_grad_partial_kernel(int P, int N, int S, int rows_per_slice, const float* __restrict__ dY,
                                                                float* __restrict__ partial)
{
    __shared__ float red[256];
    const int s = (int)blockIdx.x, b = (int)blockIdx.y;
    const int rpp = 256 / N;
    const int tid = (int)threadIdx.x;
    const int j = tid / N, col = tid - j * N;
    const int r_begin = s * rows_per_slice;
    const int r_end = (r_begin + rows_per_slice) < P ? (r_begin + rows_per_slice) : P;
    float acc = 0.f;
    if (j < rpp) {
        const float* p = dY + ((size_t)b * P) * N + col;
        for (int r = r_begin + j; r < r_end; r += 8 * rpp) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int rr = r + u * rpp;
                v[u] = rr < r_end ? p[(size_t)rr * N] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) acc += v[u];
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < N) {
        float sum = red[tid];
        for (int k = 1; k < rpp; k++) sum += red[k * N + tid];
        partial[((size_t)b * S + s) * N + tid] = sum;
    }
}

// stage 2: workgroup c < T -> dT[c][:] = the sums of the clouds with cat[b] == c, b ascending — exactly 0 for a category no cloud
// has (an out-of-range category matches no c) —; workgroup c == T -> dbias[:] = the sums of all clouds, b ascending.  A cloud's
// sum: its S partials, s ascending.  G = 1024 / N clouds at a time: thread (g, col) forms the sum of cloud b0 + g (0 if the cloud
// does not count), then thread (0, col) adds the G sums in order.
__global__ __launch_bounds__(1024) void cond_grad_finish_kernel(int B, int N, int T, int S, const float* __restrict__ partial,
                                                                const int* __restrict__ cat, float* __restrict__ dT,
                                                                float* __restrict__ dbias)
{
    __shared__ float red[1024];
    const int c = (int)blockIdx.x;
    const int G = 1024 / N;
    const int tid = (int)threadIdx.x;
    const int g = tid / N, col = tid - g * N;
    float sum = 0.f;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int b = b0 + g;
        float v = 0.f;
        if (g < G && b < B && (c == T || cat[b] == c)) {
            const float* p = partial + ((size_t)b * S) * N + col;
            for (int s = 0; s < S; s += 8) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; u++) x[u] = s + u < S ? p[(size_t)(s + u) * N] : 0.f;
#pragma unroll
                for (int u = 0; u < 8; u++) v += x[u];
            }
        }
        red[tid] = v;
        __syncthreads();
        if (tid < N) {
            const int n = (B - b0) < G ? (B - b0) : G;
            for (int k = 0; k < n; k++) sum += red[k * N + tid];
        }
        __syncthreads();
    }
    if (tid < N) {
        if (c < T) dT[(size_t)c * N + tid] = sum;
        else dbias[tid] = sum;
    }
}

// B * P rows, rounded up to whole 16-row tiles, fit an int
static bool cl_dims_ok(int B, int P) { return B > 0 && P > 0 && (long long)B * (long long)P <= 0x7fffffffll - 15; }

static bool cl_ok(int B, int P, int K1, int K2, int N, int T)
{
    return cl_dims_ok(B, P) && N >= 1 && N <= kClMaxN && K1 >= 16 && K1 % 16 == 0 && K2 >= 0 && K2 % 16 == 0 &&
           K1 + K2 <= kClMaxK && T >= 1 && T <= kClMaxT;
}

static bool cl_grad_ok(int B, int P, int N, int T) { return cl_dims_ok(B, P) && B <= 65535 && N >= 1 && N <= kClMaxN && T >= 1 && T <= kClMaxT; }

// slices of a cloud's rows in stage 1: at least 64 rows each, about 512 workgroups in all
static void cl_slices(int B, int P, int& S, int& rows_per_slice)
{
    int want = (512 + B - 1) / B;
    const int most = (P + 63) / 64;
    if (want > most) want = most;
    if (want < 1) want = 1;
    rows_per_slice = (P + want - 1) / want;
    S = (P + rows_per_slice - 1) / rows_per_slice;
}

template <int NT, int NC>
static void cl_launch(int wgs, hipStream_t st, int R, int P, int K1, int K2, int N, int T, const float* A1, const float* A2,
                      const float* W, const float* bias, const int* cat, float* Y)
{
    hipLaunchKernelGGL((cond_nn_kernel<NT, NC>), dim3(wgs), dim3(256), 0, st, R, P, K1, K2, N, T, A1, A2, W, bias, cat, Y);
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_pointwise_gemm_cond_supported(int B, int P, int K1, int K2, int N, int T) { return cl_ok(B, P, K1, K2, N, T) ? 1 : 0; }

extern "C" int sph3d_pointwise_gemm_cond(int B, int P, int K1, int K2, int N, int T, const float* A1, const float* A2, const float* W,
                                         const float* bias, const int* cat, float* Y, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && P > 0 && K1 > 0 && K2 >= 0 && N > 0 && T > 0,
                  "pointwise_gemm_cond: B, P, K1, N, T > 0 and K2 >= 0 required (got B=%d P=%d K1=%d K2=%d N=%d T=%d)", B, P, K1, K2, N, T);
    SPH3D_REQUIRE(cl_dims_ok(B, P), "pointwise_gemm_cond: B * P = %lld rows do not fit an int", (long long)B * (long long)P);
    if (!cl_ok(B, P, K1, K2, N, T)) {
        set_error("pointwise_gemm_cond: needs N <= %d, K1 and K2 multiples of 16, K1 + K2 <= %d, T <= %d (got K1=%d K2=%d N=%d T=%d)",
                  kClMaxN, kClMaxK, kClMaxT, K1, K2, N, T);
        return SPH3D_EUNSUPPORTED;
    }
    SPH3D_REQUIRE(A1 != nullptr && W != nullptr && cat != nullptr && Y != nullptr && (K2 == 0 || A2 != nullptr),
                  "pointwise_gemm_cond: A1, W, cat and Y (and A2 with K2 > 0) must not be NULL");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(A1) & 15) == 0 && (reinterpret_cast<size_t>(A2) & 15) == 0,
                  "pointwise_gemm_cond: operands must be 16-byte aligned");
    const int R = B * P;
    const int tiles = (R + 15) / 16;
    int wgs = (tiles + 7) / 8;                         // two tiles per wave
    if (wgs > 2048) wgs = 2048;
    if (wgs < 1) wgs = 1;
    hipStream_t st = as_stream(stream);
    const float* a2 = K2 > 0 ? A2 : nullptr;
    switch ((N + 15) / 16) {
    case 1: cl_launch<1, 4>(wgs, st, R, P, K1, K2, N, T, A1, a2, W, bias, cat, Y); break;
    case 2: cl_launch<2, 2>(wgs, st, R, P, K1, K2, N, T, A1, a2, W, bias, cat, Y); break;
    case 3: cl_launch<3, 2>(wgs, st, R, P, K1, K2, N, T, A1, a2, W, bias, cat, Y); break;
    default: cl_launch<4, 2>(wgs, st, R, P, K1, K2, N, T, A1, a2, W, bias, cat, Y); break;
    }
    return check_launch("sph3d_pointwise_gemm_cond");
}

extern "C" size_t sph3d_pointwise_gemm_cond_grad_workspace(int B, int P, int N, int T)
{
    if (!cl_grad_ok(B, P, N, T)) return 0;
    int S, rows_per_slice;
    cl_slices(B, P, S, rows_per_slice);
    return sizeof(float) * (size_t)B * (size_t)S * (size_t)N;
}

extern "C" int sph3d_pointwise_gemm_cond_grad(int B, int P, int N, int T, const float* dY, const int* cat, float* dT, float* dbias,
                                              void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && P > 0 && N > 0 && T > 0, "pointwise_gemm_cond_grad: B, P, N, T > 0 required (got B=%d P=%d N=%d T=%d)", B, P, N, T);
    SPH3D_REQUIRE(cl_dims_ok(B, P), "pointwise_gemm_cond_grad: B * P = %lld rows do not fit an int", (long long)B * (long long)P);
    if (!cl_grad_ok(B, P, N, T)) {
        set_error("pointwise_gemm_cond_grad: needs N <= %d, T <= %d, B <= 65535 (got B=%d N=%d T=%d)", kClMaxN, kClMaxT, B, N, T);
        return SPH3D_EUNSUPPORTED;
    }
    SPH3D_REQUIRE(dY != nullptr && cat != nullptr && dT != nullptr, "pointwise_gemm_cond_grad: dY, cat and dT must not be NULL");
    const size_t need = sph3d_pointwise_gemm_cond_grad_workspace(B, P, N, T);
    SPH3D_REQUIRE(workspace != nullptr && workspace_bytes >= need, "pointwise_gemm_cond_grad: workspace %zu B < required %zu B",
                  workspace_bytes, need);
    int S, rows_per_slice;
    cl_slices(B, P, S, rows_per_slice);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(cond_grad_partial_kernel, dim3(S, B), dim3(256), 0, st, P, N, S, rows_per_slice, dY, (float*)workspace);
    hipLaunchKernelGGL(cond_grad_finish_kernel, dim3(T + (dbias != nullptr ? 1 : 0)), dim3(1024), 0, st, B, N, T, S,
                       (const float*)workspace, cat, dT, dbias);
    return check_launch("sph3d_pointwise_gemm_cond_grad");
}
