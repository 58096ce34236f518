// lovasz.hip — the Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018) per block, with its gradient, gfx950.
//
// The statement is in include/sph3d.h (sph3d_lovasz_softmax) and, in float64 numpy, in harness/lovasz.py.  Three launches:
//   lovasz_probs_kernel   one row per thread: the softmax of the row, ordered as masked_xent_kernel (loss.hip) orders it
//   lovasz_sort_kernel    one workgroup per (class, block): counts the block's labels (G, P_b, the bad-label flag: redundantly in
//                         every workgroup of a block, as loss.hip counts its mask), packs the valid rows into 64-bit keys whose
//                         unsigned order IS the statement's order (bits(e) | ~n | fg; e >= 0, so its bits order as the value),
//                         sorts them in LDS (bitonic, descending), scans fg over the sorted order, forms the Lovasz gradient by
//                         the closed form, sums e * g in a fixed tree and scatters coef
//   lovasz_grad_kernel    one row per thread: the softmax Jacobian row; workgroup 0 of every block sums class_loss into loss
// No float atomics, no workgroup waits for another: every reduction runs in a fixed order (bit-repeatable in either mode).
#include "common.hpp"

namespace sph3d {

constexpr int kLovMaxN = 16384;      // 8 bytes of key per padded row: 128 KB of the 160 KB a workgroup can ask for
constexpr int kLovMaxC = 1024;       // presence flags of the label count (static LDS)
constexpr int kLovThreads = 1024;

__global__ __launch_bounds__(256) void lovasz_probs_kernel(long long rows, int C, const float* __restrict__ logits,
                                                           float* __restrict__ probs)
{
    const long long r = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (r >= rows) return;
    const float* row = logits + (size_t)r * C;
    float* out = probs + (size_t)r * C;
    float m = row[0];
    for (int c = 1; c < C; c++) m = fmaxf(m, row[c]);
    float se = 0.f;
    for (int c = 0; c < C; c++) se += expf(row[c] - m);
    for (int c = 0; c < C; c++) out[c] = expf(row[c] - m) / se;
}

__device__ __forceinline__ bool lov_valid(const float* __restrict__ in, int n, long long y, long long ignore)
{
    return (in == nullptr || in[n] > 0.f) && y != ignore;       // (NaN > 0 is false)
}

// integer sum of v over the workgroup (1024 threads); red: 16 ints of LDS
__device__ __forceinline__ int lov_block_isum(int v, int* red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane_id() == 0) red[(int)threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int k = 0; k < 16; k++) s += red[k];
    return s;
}

// the classes present among the valid rows of a block, from present[0, C) (LDS flags, set before the call's barrier)
__device__ __forceinline__ int lov_count_present(int C, const int* present, int* red)
{
    int p = 0;
    for (int c = (int)threadIdx.x; c < C; c += kLovThreads) p += present[c];
    return lov_block_isum(p, red);
}

__device__ __forceinline__ float lov_block_fsum(float v, float* red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane_id() == 0) red[(int)threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int k = 0; k < 16; k++) s += red[k];
    return s;
}

// grid C * B, workgroup (c, b) = (blockIdx.x % C, blockIdx.x / C); dynamic LDS: Npad keys
__global__ __launch_bounds__(kLovThreads) void lovasz_sort_kernel(int N, int C, int Npad, const long long* __restrict__ label,
                                                                  const float* __restrict__ inner, long long ignore,
                                                                  const float* __restrict__ probs, float* __restrict__ coef,
                                                                  float* __restrict__ class_loss, int* __restrict__ order)
{
    extern __shared__ unsigned long long lov_keys[];
    __shared__ int present[kLovMaxC];
    __shared__ int red[16];
    __shared__ int wsum[16];
    __shared__ float fred[16];
    unsigned long long* keys = lov_keys;
    const int tid = (int)threadIdx.x;
    const int c = (int)(blockIdx.x % (unsigned)C), b = (int)(blockIdx.x / (unsigned)C);
    const long long* lb = label + (size_t)b * N;
    const float* in = inner != nullptr ? inner + (size_t)b * N : nullptr;
    const float* pr = probs + (size_t)b * N * C;
    float* cf = coef + (size_t)b * N * C;

    for (int k = tid; k < C; k += kLovThreads) present[k] = 0;
    __syncthreads();
    // one pass over the block's rows: the label count and this class's keys.  A row that is not valid and the padding get key 0,
    // below every valid key (a valid key holds 0x7fffffff - n > 0 above its lowest bit)
    int G = 0, bad = 0;
    for (int n = tid; n < Npad; n += kLovThreads) {
        unsigned long long key = 0ull;
        if (n < N) {
            const long long y = lb[n];
            if (lov_valid(in, n, y, ignore)) {
                if (y < 0 || y >= C) bad = 1;                       // nothing is clamped: the block is NaN
                else present[(int)y] = 1;                           // (every writer stores the same 1)
                const unsigned fg = y == (long long)c ? 1u : 0u;
                G += (int)fg;
                const float p = pr[(size_t)n * C + c];
                const float e = fg ? 1.f - p : p;
                if (!isfinite(e)) bad = 1;
                key = ((unsigned long long)__float_as_uint(e) << 32) | ((unsigned long long)(0x7fffffffu - (unsigned)n) << 1) | fg;
            } else {
                cf[(size_t)n * C + c] = 0.f;
            }
        }
        keys[n] = key;
    }
    G = lov_block_isum(G, red);
    bad = lov_block_isum(bad, red);
    const int P = lov_count_present(C, present, red);

    // bitonic network, descending; the keys of valid rows are distinct
    const int half = Npad >> 1;
    for (int k = 2; k <= Npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < half; t += kLovThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = keys[i], d = keys[l];
                if ((i & k) == 0 ? a < d : a > d) {
                    keys[i] = d;
                    keys[l] = a;
                }
            }
        }
    }
    __syncthreads();

    // thread t owns the sorted positions [t * E, t * E + E): fg counted per thread, scanned over the wave, then over the waves
    const int E = Npad > kLovThreads ? Npad / kLovThreads : 1;
    const int base = tid * E;
    int cnt = 0;
    for (int q = 0; q < E; q++)
        if (base + q < Npad) cnt += (int)(keys[base + q] & 1ull);
    int inc = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane_id() >= o) inc += v;
    }
    if (lane_id() == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    int F = inc - cnt;
    for (int k = 0; k < (tid >> 6); k++) F += wsum[k];

    const bool live = G > 0 && bad == 0;
    const float invP = P > 0 ? 1.f / (float)P : 0.f;
    const float nanv = __builtin_nanf("");
    int* ord = order != nullptr ? order + ((size_t)b * C + c) * N : nullptr;
    float sum = 0.f;
    for (int q = 0; q < E; q++) {
        const int j = base + q;
        if (j >= N) break;
        const unsigned long long key = keys[j];
        if (key == 0ull) {                                           // past the valid rows
            if (ord != nullptr) ord[j] = -1;
            continue;
        }
        const int fg = (int)(key & 1ull);
        const int n = (int)(0x7fffffffu - (unsigned)((key >> 1) & 0x7fffffffull));
        F += fg;
        if (ord != nullptr) ord[j] = n;
        float cv = 0.f;
        if (live) {
            const float e = __uint_as_float((unsigned)(key >> 32));
            const int U = G + (j + 1) - F;
            const float g = fg ? 1.f / (float)U : (float)(G - F) / ((float)U * (float)(U - 1));
            sum += e * g;
            cv = (fg ? -g : g) * invP;
        }
        cf[(size_t)n * C + c] = bad ? nanv : cv;
    }
    sum = lov_block_fsum(sum, fred);
    if (tid == 0) class_loss[(size_t)b * C + c] = bad ? nanv : (live ? sum : 0.f);
}

// grid (S, B): workgroup (s, b) handles the rows [s * 1024, (s + 1) * 1024) of block b; workgroup (0, b) also counts the block's
// classes and writes loss[b].  dlogits == NULL: the launch is (1, B) and only that sum runs.
__global__ __launch_bounds__(kLovThreads) void lovasz_grad_kernel(int N, int C, const long long* __restrict__ label,
                                                                  const float* __restrict__ inner, long long ignore,
                                                                  const float* __restrict__ probs, const float* __restrict__ coef,
                                                                  const float* __restrict__ class_loss, float* __restrict__ loss,
                                                                  float* __restrict__ dlogits)
{
    __shared__ int present[kLovMaxC];
    __shared__ int red[16];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const long long* lb = label + (size_t)b * N;
    const float* in = inner != nullptr ? inner + (size_t)b * N : nullptr;
    const float* cl = class_loss + (size_t)b * C;
    bool bad = false;                                                // a NaN class loss: the whole block is NaN
    for (int c = 0; c < C; c++) bad = bad || isnan(cl[c]);
    const float nanv = __builtin_nanf("");

    if (blockIdx.x == 0) {
        for (int k = tid; k < C; k += kLovThreads) present[k] = 0;
        __syncthreads();
        for (int n = tid; n < N; n += kLovThreads) {
            const long long y = lb[n];
            if (lov_valid(in, n, y, ignore) && y >= 0 && y < C) present[(int)y] = 1;
        }
        const int P = lov_count_present(C, present, red);
        if (tid == 0) {
            float s = 0.f;
            for (int c = 0; c < C; c++) s += cl[c];                  // ascending c; an absent class holds an exact 0
            loss[b] = bad ? nanv : (P > 0 ? s / (float)P : 0.f);
        }
    }
    if (dlogits == nullptr) return;
    const int n = (int)blockIdx.x * kLovThreads + tid;
    if (n >= N) return;
    const float* p = probs + ((size_t)b * N + n) * C;
    const float* cf = coef + ((size_t)b * N + n) * C;
    float* d = dlogits + ((size_t)b * N + n) * C;
    if (bad) {
        for (int c = 0; c < C; c++) d[c] = nanv;
    } else if (!lov_valid(in, n, lb[n], ignore)) {
        for (int c = 0; c < C; c++) d[c] = 0.f;
    } else {
        float dot = 0.f;
        for (int c = 0; c < C; c++) dot += cf[c] * p[c];
        for (int c = 0; c < C; c++) d[c] = p[c] * (cf[c] - dot);
    }
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_lovasz_softmax_supported(int N, int C)
{
    return (N > 0 && N <= kLovMaxN && C > 0 && C <= kLovMaxC) ? 1 : 0;
}

extern "C" int sph3d_lovasz_softmax(int B, int N, int C, const float* logits, const long long* label, const float* inner,
                                    long long ignore, float* probs, float* coef, float* class_loss, float* loss, float* dlogits,
                                    int* order, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B >= 0 && N > 0 && C > 0, "lovasz_softmax: bad dims B=%d N=%d C=%d", B, N, C);
    SPH3D_REQUIRE((long long)B * N * C <= (1ll << 40) && (long long)B * C <= 0x7fffffffll && B <= 65535,
                  "lovasz_softmax: bad dims B=%d N=%d C=%d (B N C <= 2^40, B C < 2^31, B < 2^16)", B, N, C);
    if (!sph3d_lovasz_softmax_supported(N, C)) {
        set_error("lovasz_softmax: N=%d C=%d is not covered (N <= %d rows per block, C <= %d classes)", N, C, kLovMaxN, kLovMaxC);
        return SPH3D_EUNSUPPORTED;
    }
    if (B == 0) return SPH3D_OK;
    SPH3D_REQUIRE(logits != nullptr && label != nullptr && probs != nullptr && coef != nullptr && class_loss != nullptr &&
                      loss != nullptr,
                  "lovasz_softmax: null logits, label, probs, coef, class_loss or loss");
    hipStream_t st = as_stream(stream);
    const long long rows = (long long)B * N;
    hipLaunchKernelGGL(lovasz_probs_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, rows, C, logits, probs);
    int Npad = 1;
    while (Npad < N) Npad <<= 1;
    const int rc = launch_lds(lovasz_sort_kernel, dim3((unsigned)(B * C)), dim3(kLovThreads), sizeof(unsigned long long) * (size_t)Npad,
                              st, "sph3d_lovasz_softmax", N, C, Npad, label, inner, ignore, (const float*)probs, coef, class_loss,
                              order);
    if (rc != SPH3D_OK) return rc;
    const int S = dlogits != nullptr ? (N + kLovThreads - 1) / kLovThreads : 1;
    hipLaunchKernelGGL(lovasz_grad_kernel, dim3(S, B), dim3(kLovThreads), 0, st, N, C, label, inner, ignore, (const float*)probs,
                       (const float*)coef, (const float*)class_loss, loss, dlogits);
    return check_launch("sph3d_lovasz_softmax");
}
