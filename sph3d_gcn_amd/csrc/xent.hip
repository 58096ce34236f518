// xent.hip — softmax cross-entropy with class weights, label smoothing and an ignore label, per block, gfx950.
//
// The statement is in include/sph3d.h (sph3d_softmax_xent) and, in float64 numpy, in harness/xent.py (xent_reference).  With
// every option at its default the call computes what loss.hip's masked_xent_kernel computes, in the same operation order and with
// the same thread-to-row map, so loss_part and dlogits are the same bits for N <= 16384.
//
// Two launches.  The denominators D_b are functions of the block's integer class histogram, which the caller wants anyway:
//   xent_count_kernel   grid (S, B): workgroup (s, b) counts the labels of the counted rows of its slice in LDS (integer
//                       atomics: exact, order-free) and stores its C counts in the workspace;
//   xent_kernel         grid (S, B): workgroup (s, b) adds the S slices' counts of block b (S * C integers), forms D_b and
//                       sum_c w_c from them in float64 in ascending c, and then handles its slice as loss.hip does.
// A recount per workgroup, as loss.hip does for its mask, reads S * N labels and mask values per block: at batch scope (one block
// of B * N rows, S = 128 at 131 072 rows) that is 128 passes over the labels; the first launch keeps it at one.
#include "common.hpp"

namespace sph3d {

constexpr int kXentThreads = 1024;
constexpr int kXentMaxC = 4096;      // weights and histogram of one block live in LDS: 8 * C bytes
constexpr int kXentMaxParts = 256;     // one workgroup per CU and block; beyond it a workgroup takes several trips

constexpr size_t kXentMaxLds = 144 * 1024;   // of the CU's 160 KB

// xent_kernel's LDS before the staged rows: the tree and the two scalars, the histogram, the weights; a multiple of 16
__host__ __device__ __forceinline__ size_t xent_head_bytes(int C) { return (128 + (size_t)C * 8 + 15) & ~(size_t)15; }

// the row stride of the staged form: C made odd, or 0 (every thread walks its row in memory) when 1024 such rows do not fit
static inline int xent_stride(int C)
{
    const int stride = C | 1;
    return xent_head_bytes(C) + (size_t)kXentThreads * stride * sizeof(float) <= kXentMaxLds ? stride : 0;
}

// block_sum_1024 of loss.hip: the butterfly of each wave, then the 16 waves in ascending order
__device__ __forceinline__ float xent_block_sum(float v, float* red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = (int)threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int k = 0; k < 16; k++) s += red[k];
    return s;
}

__device__ __forceinline__ long long xent_label(const void* __restrict__ label, int wide, size_t i)
{
    return wide ? static_cast<const long long*>(label)[i] : (long long)static_cast<const int*>(label)[i];
}

__global__ __launch_bounds__(kXentThreads) void xent_count_kernel(int N, int C, int chunk, const void* __restrict__ label, int wide,
                                                                  const float* __restrict__ inner, int has_ignore, long long ignore,
                                                                  int* __restrict__ part_hist)
{
    extern __shared__ __attribute__((aligned(16))) char xent_smem[];
    int* sh = reinterpret_cast<int*>(xent_smem);                       // [C]
    const int b = (int)blockIdx.y, sl = (int)blockIdx.x, S = (int)gridDim.x;
    for (int c = (int)threadIdx.x; c < C; c += kXentThreads) sh[c] = 0;
    __syncthreads();
    const int n0 = sl * chunk, n1 = (n0 + chunk) < N ? (n0 + chunk) : N;
    for (int n = n0 + (int)threadIdx.x; n < n1; n += kXentThreads) {
        const size_t i = (size_t)b * N + n;
        if (inner != nullptr && !(inner[i] > 0.f)) continue;
        const long long y = xent_label(label, wide, i);
        if (has_ignore && y == ignore) continue;
        if (y >= 0 && y < C) atomicAdd(&sh[(int)y], 1);
    }
    __syncthreads();
    int* out = part_hist + ((size_t)b * S + sl) * C;
    for (int c = (int)threadIdx.x; c < C; c += kXentThreads) out[c] = sh[c];
}

__global__ __launch_bounds__(kXentThreads) void xent_kernel(int N, int C, int chunk, const float* __restrict__ logits,
                                                            const void* __restrict__ label, int wide, const float* __restrict__ inner,
                                                            const float* __restrict__ weight, float omeps, float epsC, int has_ignore,
                                                            long long ignore, int by_weight, const int* __restrict__ part_hist,
                                                            float* __restrict__ lossPart, int* __restrict__ hist,
                                                            float* __restrict__ dlogits, int stride)
{
    extern __shared__ __attribute__((aligned(16))) char xent_smem[];
    float* red = reinterpret_cast<float*>(xent_smem);                  // [16] the tree's, [16] D, [17] sum_c w_c
    int* sh = reinterpret_cast<int*>(xent_smem + 128);                 // [C] the block's histogram
    float* sw = reinterpret_cast<float*>(xent_smem + 128) + C;         // [C] the weights (1 without)
    float* tile = reinterpret_cast<float*>(xent_smem + xent_head_bytes(C));   // [1024 * stride] a trip's rows (stride > 0)
    const int b = (int)blockIdx.y, sl = (int)blockIdx.x, S = (int)gridDim.x;
    const bool smooth = epsC != 0.f;

    for (int c = (int)threadIdx.x; c < C; c += kXentThreads) {
        const int* ph = part_hist + (size_t)b * S * C + c;
        int h = 0;
#pragma unroll 8
        for (int s = 0; s < S; s++) h += ph[(size_t)s * C];
        sh[c] = h;
        sw[c] = weight != nullptr ? weight[c] : 1.f;
        if (sl == 0) hist[(size_t)b * C + c] = h;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // D_b and sum_c w_c in float64, ascending c (the numpy statement does the same): one rounding to float32 each
        // (no branch inside the loops and eight classes per trip: the LDS reads of a trip are in flight together; with one wait per
        // read the walk took 90 ns a class, 0.37 ms at 4096 classes)
        long long cnt = 0;
        double dw = 0.0, ws = 0.0;
#pragma unroll 8
        for (int c = 0; c < C; c++) cnt += sh[c];
        if (weight != nullptr) {
#pragma unroll 8
            for (int c = 0; c < C; c++) {
                const double w = (double)sw[c];
                dw += (double)sh[c] * w;
                ws += w;
            }
        }
        red[16] = (by_weight && weight != nullptr) ? (float)dw : (float)cnt;
        red[17] = weight != nullptr ? (float)ws : (float)C;
    }
    __syncthreads();
    const float D = red[16], W = red[17];
    const float inv = D > 0.f ? 1.f / D : 0.f;

    const float* lg = logits + (size_t)b * N * C;
    const int n0 = sl * chunk, n1 = (n0 + chunk) < N ? (n0 + chunk) : N;
    float* dg = dlogits != nullptr ? dlogits + (size_t)b * N * C : nullptr;      // dlogits == NULL: the losses only
    float sum = 0.f;
    // a trip: the rows [base, base + 1024) of the slice, thread t on row base + t (loss.hip's map).  stride > 0: the trip's logits, one
    // contiguous span, come into LDS with coalesced loads, rows stride floats apart (odd: the threads' row walks hit 32 banks); the
    // gradient takes the logits' place row by row and leaves the same way.  stride == 0: every thread walks its row in memory.
    for (int base = n0; base < n1; base += kXentThreads) {
        const int rows = (n1 - base) < kXentThreads ? (n1 - base) : kXentThreads;
        if (stride > 0) {
            const float* src = lg + (size_t)base * C;
            for (int k = (int)threadIdx.x; k < rows * C; k += kXentThreads) tile[(k / C) * stride + (k % C)] = src[k];
            __syncthreads();
        }
        const int n = base + (int)threadIdx.x;
        if (n < n1) {
            const float* row = stride > 0 ? tile + (int)threadIdx.x * stride : lg + (size_t)n * C;
            float* drow = dlogits == nullptr ? nullptr : (stride > 0 ? tile + (int)threadIdx.x * stride : dg + (size_t)n * C);
            const size_t i = (size_t)b * N + n;
            bool counted = inner == nullptr || inner[i] > 0.f;
            long long y = 0;
            if (counted) {
                y = xent_label(label, wide, i);
                counted = !(has_ignore && y == ignore);
            }
            if (counted) {
                float m = row[0];
                for (int c = 1; c < C; c++) m = fmaxf(m, row[c]);
                float se = 0.f;
                for (int c = 0; c < C; c++) se += expf(row[c] - m);
                // a counted label outside [0, C): the block's loss and the row's gradient are NaN (loss.hip's rule); reads stay in range
                const bool bad = y < 0 || y >= C;
                y = bad ? 0 : y;
                const float wy = sw[y];
                const float lse = m + logf(se);
                float l = wy * (lse - row[y]);
                if (smooth) {
                    float s2 = 0.f;
                    for (int c = 0; c < C; c++) s2 += sw[c] * (lse - row[c]);
                    l = omeps * l + epsC * s2;
                }
                sum += bad ? __builtin_nanf("") : l;
                if (drow != nullptr) {
                    const float ty = omeps * wy;
                    const float A = smooth ? ty + epsC * W : ty;
                    const float r = (A * inv) / se;
                    for (int c = 0; c < C; c++) {
                        float t = c == (int)y ? ty : 0.f;
                        if (smooth) t += epsC * sw[c];
                        const float e = expf(row[c] - m);                      // (read before drow[c], the same word when staged)
                        drow[c] = bad ? __builtin_nanf("") : e * r - t * inv;
                    }
                }
            } else if (drow != nullptr) {
                for (int c = 0; c < C; c++) drow[c] = 0.f;
            }
        }
        if (stride > 0) {
            __syncthreads();
            if (dlogits != nullptr) {
                float* dst = dg + (size_t)base * C;
                for (int k = (int)threadIdx.x; k < rows * C; k += kXentThreads) dst[k] = tile[(k / C) * stride + (k % C)];
                __syncthreads();
            }
        }
    }
    sum = xent_block_sum(sum, red);
    if (threadIdx.x == 0) lossPart[(size_t)b * S + sl] = sum * inv;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_softmax_xent_parts(int N)
{
    const int s = (N + kXentThreads - 1) / kXentThreads;
    return s < 1 ? 1 : (s > kXentMaxParts ? kXentMaxParts : s);
}

extern "C" int sph3d_softmax_xent_supported(int N, int C) { return N > 0 && C > 0 && C <= kXentMaxC; }

extern "C" size_t sph3d_softmax_xent_workspace(int B, int N, int C)
{
    if (B <= 0 || N <= 0 || C <= 0) return 0;
    return (size_t)B * (size_t)sph3d_softmax_xent_parts(N) * (size_t)C * sizeof(int);
}

extern "C" int sph3d_softmax_xent(int B, int N, int C, const float* logits, const void* label, int label_bits, const float* inner,
                                  const float* weight, float label_smoothing, int has_ignore, long long ignore, int normalize,
                                  float* loss_part, int* hist, float* dlogits, void* workspace, size_t workspace_bytes,
                                  sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B >= 0 && N > 0 && C > 0, "softmax_xent: bad dims B=%d N=%d C=%d", B, N, C);
    // (N <= 2^30: a slice's end n0 + chunk and a trip's rows base + 1023 stay below 2^31 in the kernels' int arithmetic)
    SPH3D_REQUIRE(B < (1 << 16) && N <= (1 << 30) && (long long)B * N < (1LL << 31),
                  "softmax_xent: bad dims B=%d N=%d C=%d (B < 2^16, N <= 2^30, B N < 2^31)", B, N, C);
    SPH3D_REQUIRE(label_bits == 32 || label_bits == 64, "softmax_xent: label_bits should be 32 or 64, got %d", label_bits);
    SPH3D_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, "softmax_xent: label_smoothing should lie in [0, 1), got %g",
                  (double)label_smoothing);
    SPH3D_REQUIRE(normalize == 0 || normalize == 1, "softmax_xent: normalize should be 0 (count) or 1 (weight), got %d", normalize);
    if (!sph3d_softmax_xent_supported(N, C)) {
        set_error("softmax_xent: N=%d C=%d is not covered (C <= %d classes)", N, C, kXentMaxC);
        return SPH3D_EUNSUPPORTED;
    }
    if (B == 0) return SPH3D_OK;
    SPH3D_REQUIRE(logits != nullptr && label != nullptr && loss_part != nullptr && hist != nullptr,
                  "softmax_xent: null logits, label, loss_part or hist");
    SPH3D_REQUIRE(workspace != nullptr && (reinterpret_cast<size_t>(workspace) & 3) == 0, "softmax_xent: workspace must be 4-byte aligned");
    const size_t need = sph3d_softmax_xent_workspace(B, N, C);
    if (workspace_bytes < need) {
        set_error("softmax_xent: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return SPH3D_EWORKSPACE;
    }
    const int S = sph3d_softmax_xent_parts(N);
    const int chunk = (N + S - 1) / S;
    const int wide = label_bits == 64;
    const float omeps = 1.f - label_smoothing, epsC = label_smoothing / (float)C;
    int* part_hist = static_cast<int*>(workspace);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(xent_count_kernel, dim3(S, B), dim3(kXentThreads), (size_t)C * sizeof(int), st, N, C, chunk, label, wide, inner,
                       has_ignore != 0, ignore, part_hist);
    const int stride = xent_stride(C);
    const size_t lds = xent_head_bytes(C) + (size_t)kXentThreads * stride * sizeof(float);
    const int rc = launch_lds(xent_kernel, dim3(S, B), dim3(kXentThreads), lds, st, "sph3d_softmax_xent", N, C, chunk, logits, label,
                              wide, inner, weight, omeps, epsC, (int)(has_ignore != 0), ignore, normalize, (const int*)part_hist,
                              loss_part, hist, dlogits, stride);
    if (rc != SPH3D_OK) return rc;
    return check_launch("sph3d_softmax_xent");
}
