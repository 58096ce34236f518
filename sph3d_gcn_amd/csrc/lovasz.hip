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
//
// Blocks of up to 2^20 rows (sph3d_lovasz_softmax_large; the host's choices are lovasz_plan.hpp's) sort in global memory, `slab`
// classes at a time:
//   lovasz_probs_kernel        as above
//   lovasz_large_count_kernel  G[b, c] and the block's bad flag, by integer atomics on zeroed counters
//   lovasz_run_sort_kernel     one workgroup per (run, class, block): the same keys, a run of `tile` of them sorted in LDS
//   lovasz_merge_kernel        ceil(log2(runs)) launches: a workgroup per 1024 output keys of a pair of runs (merge path)
//   lovasz_tile_count_kernel   the foreground keys of every 1024 sorted positions
//   lovasz_finish_kernel       F from those counts, then g, coef and order as lovasz_sort_kernel forms them; a partial sum per tile
//   lovasz_class_kernel        one wave per (class, block) adds the tiles' partial sums in a fixed tree
//   lovasz_large_grad_kernel   lovasz_grad_kernel with P_b taken from G
// Launch boundaries order the phases; nothing else does.
#include <stddef.h>
#include <string.h>
#include "common.hpp"
#include "lovasz_plan.hpp"

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

// one row of the softmax Jacobian (lovasz_grad_kernel, lovasz_large_grad_kernel): NaN through a bad block, zeros on a row that is
// not valid
__device__ __forceinline__ void lov_grad_row(int C, bool bad, bool valid, const float* __restrict__ p, const float* __restrict__ cf,
                                             float* __restrict__ d)
{
    if (bad) {
        const float nanv = __builtin_nanf("");
        for (int c = 0; c < C; c++) d[c] = nanv;
    } else if (!valid) {
        for (int c = 0; c < C; c++) d[c] = 0.f;
    } else {
        float dot = 0.f;
        for (int c = 0; c < C; c++) dot += cf[c] * p[c];
        for (int c = 0; c < C; c++) d[c] = p[c] * (cf[c] - dot);
    }
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
    lov_grad_row(C, bad, lov_valid(in, n, lb[n], ignore), probs + ((size_t)b * N + n) * C, coef + ((size_t)b * N + n) * C,
                 dlogits + ((size_t)b * N + n) * C);
}

// ---- blocks beyond kLovMaxN rows: the sort in global memory (sph3d_lovasz_softmax_large; the host's part is lovasz_plan.hpp) -----
// A SEGMENT is the npad = runs * tile keys of one (class, block); the key buffers hold [slab][B] segments, segment (cs, b) of a
// launch with grid (., slab, B) at index cs * B + b.  Phases are ordered by launch boundaries only.
__device__ __forceinline__ size_t lov_segment() { return (size_t)blockIdx.y * gridDim.z + blockIdx.z; }

// grid (ceil(N / 4096), B): G[b, c] = #{valid n: label = c} and the block's bad flag (a valid row with a label outside [0, C) or
// with probabilities that are not finite).  Integer atomics on zeroed counters: the counts do not depend on the order.
__global__ __launch_bounds__(kLovThreads) void lovasz_large_count_kernel(int N, int C, const long long* __restrict__ label,
                                                                         const float* __restrict__ inner, long long ignore,
                                                                         const float* __restrict__ probs, int* __restrict__ count,
                                                                         int* __restrict__ badflag)
{
    __shared__ int hist[kLovMaxC];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const long long* lb = label + (size_t)b * N;
    const float* in = inner != nullptr ? inner + (size_t)b * N : nullptr;
    for (int k = tid; k < C; k += kLovThreads) hist[k] = 0;
    __syncthreads();
    int bad = 0;
    for (int q = 0; q < kLovCountRows / kLovThreads; q++) {
        const int n = (int)blockIdx.x * kLovCountRows + q * kLovThreads + tid;
        if (n >= N) break;
        const long long y = lb[n];
        if (!lov_valid(in, n, y, ignore)) continue;
        if (y < 0 || y >= C) bad = 1;
        else atomicAdd(&hist[(int)y], 1);
        const float* p = probs + ((size_t)b * N + n) * C;
        for (int c = 0; c < C; c++)
            if (!isfinite(p[c])) bad = 1;
    }
    __syncthreads();
    for (int k = tid; k < C; k += kLovThreads)
        if (hist[k] != 0) atomicAdd(&count[(size_t)b * C + k], hist[k]);
    if (bad) atomicOr(&badflag[b], 1);
}

// grid (runs, slab, B), dynamic LDS: T keys.  Run r of class c0 + blockIdx.y: the keys of rows [r T, (r + 1) T) as
// lovasz_sort_kernel packs them (0 for a row that is not valid and past N), sorted descending by its network
__global__ __launch_bounds__(kLovThreads) void lovasz_run_sort_kernel(int N, int C, int T, int npad, int c0,
                                                                      const long long* __restrict__ label,
                                                                      const float* __restrict__ inner, long long ignore,
                                                                      const float* __restrict__ probs, float* __restrict__ coef,
                                                                      unsigned long long* __restrict__ keys_out)
{
    extern __shared__ unsigned long long lov_keys[];
    unsigned long long* keys = lov_keys;
    const int tid = (int)threadIdx.x;
    const int c = c0 + (int)blockIdx.y, b = (int)blockIdx.z, n0 = (int)blockIdx.x * T;
    const long long* lb = label + (size_t)b * N;
    const float* in = inner != nullptr ? inner + (size_t)b * N : nullptr;
    const float* pr = probs + (size_t)b * N * C;
    float* cf = coef + (size_t)b * N * C;
    for (int i = tid; i < T; i += kLovThreads) {
        const int n = n0 + i;
        unsigned long long key = 0ull;
        if (n < N) {
            const long long y = lb[n];
            if (lov_valid(in, n, y, ignore)) {
                const unsigned fg = y == (long long)c ? 1u : 0u;
                const float p = pr[(size_t)n * C + c];
                const float e = fg ? 1.f - p : p;
                key = ((unsigned long long)__float_as_uint(e) << 32) | ((unsigned long long)(0x7fffffffu - (unsigned)n) << 1) | fg;
            } else {
                cf[(size_t)n * C + c] = 0.f;
            }
        }
        keys[i] = key;
    }
    const int half = T >> 1;
    for (int k = 2; k <= T; k <<= 1) {
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
    unsigned long long* out = keys_out + lov_segment() * (size_t)npad + (size_t)n0;
    for (int i = tid; i < T; i += kLovThreads) out[i] = keys[i];
}

// the merge path: how many of the first d keys of the merged (descending) sequence come from a[0, la), the others from
// b[0, lb); of equal keys (the zeros) a's come first.  Reads a[i] with i < min(d, la) and b[i] with i < min(d, lb) only.
__device__ __forceinline__ int lov_merge_path(const unsigned long long* a, int la, const unsigned long long* b, int lb, int d)
{
    int lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] >= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid (mtiles, slab, B): output keys [1024 x, 1024 (x + 1)) of a segment.  Runs of L keys (a multiple of 1024) pair up from the
// segment's start; the last pair's second run may be shorter or missing (then the first is copied).  Two searches in global
// memory cut the pair at the tile's ends, the 1024 keys between the cuts go to LDS, and every thread merges four of them.
__global__ __launch_bounds__(kLovMergeBlock) void lovasz_merge_kernel(int npad, int L, const unsigned long long* __restrict__ src,
                                                                      unsigned long long* __restrict__ dst)
{
    __shared__ unsigned long long sk[kLovMergeTile];
    __shared__ int cut[2];
    const int tid = (int)threadIdx.x;
    const size_t base = lov_segment() * (size_t)npad;
    const int o0 = (int)blockIdx.x * kLovMergeTile;
    const int ps = o0 - o0 % (2 * L);                               // (L <= 2^20: 2 L fits an int)
    const int la = min(L, npad - ps), lb = min(L, npad - ps - la);
    const unsigned long long* A = src + base + ps;
    const unsigned long long* Bq = A + la;
    const int d0 = o0 - ps;
    if (tid < 2) cut[tid] = lov_merge_path(A, la, Bq, lb, d0 + tid * kLovMergeTile);        // (d0 + 1024 <= la + lb)
    __syncthreads();
    const int a0 = cut[0], nA = cut[1] - cut[0], nB = kLovMergeTile - nA, b0 = d0 - a0;
    for (int i = tid; i < kLovMergeTile; i += kLovMergeBlock) sk[i] = i < nA ? A[a0 + i] : Bq[b0 + (i - nA)];
    __syncthreads();
    constexpr int kPer = kLovMergeTile / kLovMergeBlock;
    const unsigned long long* sA = sk;
    const unsigned long long* sB = sk + nA;
    const int dd = tid * kPer;
    int ai = lov_merge_path(sA, nA, sB, nB, dd), bi = dd - ai;
    unsigned long long* out = dst + base + o0 + dd;
    for (int q = 0; q < kPer; q++) {
        const bool takeA = bi >= nB || (ai < nA && sA[ai] >= sB[bi]);
        out[q] = takeA ? sA[ai++] : sB[bi++];
    }
}

// grid (mtiles, slab, B): the foreground keys of every output tile of the sorted segments
__global__ __launch_bounds__(kLovThreads) void lovasz_tile_count_kernel(int npad, const unsigned long long* __restrict__ keys,
                                                                        int* __restrict__ tilecnt)
{
    __shared__ int red[16];
    const size_t seg = lov_segment();
    const int fg = (int)(keys[seg * (size_t)npad + (size_t)blockIdx.x * kLovMergeTile + threadIdx.x] & 1ull);
    const int s = lov_block_isum(fg, red);
    if (threadIdx.x == 0) tilecnt[seg * gridDim.x + blockIdx.x] = s;
}

// grid (mtiles, slab, B), a sorted position per thread: F from the tiles before this one (integers) and a scan of this tile, then
// g, coef and order as lovasz_sort_kernel forms them, operation for operation; the tile's sum of e g goes to a slot of its own.
// Summation tree of a tile: the 64 lanes of a wave by the 6-step butterfly, the 16 waves in order onto 0.f.
__global__ __launch_bounds__(kLovThreads) void lovasz_finish_kernel(int N, int C, int npad, int c0,
                                                                    const unsigned long long* __restrict__ keys,
                                                                    const int* __restrict__ tilecnt, const int* __restrict__ count,
                                                                    const int* __restrict__ badflag, float* __restrict__ coef,
                                                                    float* __restrict__ partial, int* __restrict__ order)
{
    __shared__ int red[16];
    __shared__ int wsum[16];
    __shared__ float fred[16];
    const int tid = (int)threadIdx.x;
    const int c = c0 + (int)blockIdx.y, b = (int)blockIdx.z, tile = (int)blockIdx.x, tiles = (int)gridDim.x;
    const size_t seg = lov_segment();
    int before = 0, present = 0;
    for (int k = tid; k < tile; k += kLovThreads) before += tilecnt[seg * tiles + k];
    for (int k = tid; k < C; k += kLovThreads) present += count[(size_t)b * C + k] > 0 ? 1 : 0;
    before = lov_block_isum(before, red);
    const int P = lov_block_isum(present, red);
    const int G = count[(size_t)b * C + c], bad = badflag[b];

    const int j = tile * kLovMergeTile + tid;
    const unsigned long long key = keys[seg * (size_t)npad + j];
    const int fg = (int)(key & 1ull);
    int inc = fg;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane_id() >= o) inc += v;
    }
    if (lane_id() == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    int F = before + inc;                                            // foreground rows among the sorted positions 0..j
    for (int k = 0; k < (tid >> 6); k++) F += wsum[k];

    const bool live = G > 0 && bad == 0;
    const float invP = P > 0 ? 1.f / (float)P : 0.f;
    const float nanv = __builtin_nanf("");
    float sum = 0.f;
    if (j < N) {
        int* ord = order != nullptr ? order + ((size_t)b * C + c) * N : nullptr;
        if (key == 0ull) {                                           // past the valid rows
            if (ord != nullptr) ord[j] = -1;
        } else {
            const int n = (int)(0x7fffffffu - (unsigned)((key >> 1) & 0x7fffffffull));
            if (ord != nullptr) ord[j] = n;
            float cv = 0.f;
            if (live) {
                const float e = __uint_as_float((unsigned)(key >> 32));
                const int U = G + (j + 1) - F;
                const float g = fg ? 1.f / (float)U : (float)(G - F) / ((float)U * (float)(U - 1));
                sum = e * g;
                cv = (fg ? -g : g) * invP;
            }
            coef[((size_t)b * N + n) * C + c] = bad ? nanv : cv;
        }
    }
    sum = lov_block_fsum(sum, fred);
    if (tid == 0) partial[seg * tiles + tile] = sum;
}

// grid (slab, B), one wave: class_loss = the tiles' partial sums, lane l adding the tiles l, l + 64, ... in order onto 0.f, then the
// 64 lanes by the 6-step butterfly
__global__ __launch_bounds__(64) void lovasz_class_kernel(int C, int tiles, int c0, const float* __restrict__ partial,
                                                          const int* __restrict__ count, const int* __restrict__ badflag,
                                                          float* __restrict__ class_loss)
{
    const int c = c0 + (int)blockIdx.x, b = (int)blockIdx.y;
    const size_t seg = (size_t)blockIdx.x * gridDim.y + blockIdx.y;
    float v = 0.f;
    for (int k = (int)threadIdx.x; k < tiles; k += 64) v += partial[seg * tiles + k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (threadIdx.x == 0)
        class_loss[(size_t)b * C + c] = badflag[b] ? __builtin_nanf("") : (count[(size_t)b * C + c] > 0 ? v : 0.f);
}

// lovasz_grad_kernel with the block's present classes and bad flag taken from the counts (a block of 2^20 rows is not walked by one
// workgroup again).  grid (S, B); dlogits == NULL: (1, B), the loss only.
__global__ __launch_bounds__(kLovThreads) void lovasz_large_grad_kernel(int N, int C, const long long* __restrict__ label,
                                                                        const float* __restrict__ inner, long long ignore,
                                                                        const float* __restrict__ probs, const float* __restrict__ coef,
                                                                        const float* __restrict__ class_loss,
                                                                        const int* __restrict__ count, const int* __restrict__ badflag,
                                                                        float* __restrict__ loss, float* __restrict__ dlogits)
{
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const bool bad = badflag[b] != 0;
    if (blockIdx.x == 0 && tid == 0) {
        const float* cl = class_loss + (size_t)b * C;
        int P = 0;
        float s = 0.f;
        for (int c = 0; c < C; c++) {
            P += count[(size_t)b * C + c] > 0 ? 1 : 0;
            s += cl[c];                                               // ascending c; an absent class holds an exact 0
        }
        loss[b] = bad ? __builtin_nanf("") : (P > 0 ? s / (float)P : 0.f);
    }
    if (dlogits == nullptr) return;
    const int n = (int)blockIdx.x * kLovThreads + tid;
    if (n >= N) return;
    const float* in = inner != nullptr ? inner + (size_t)b * N : nullptr;
    lov_grad_row(C, bad, lov_valid(in, n, label[(size_t)b * N + n], ignore), probs + ((size_t)b * N + n) * C,
                 coef + ((size_t)b * N + n) * C, dlogits + ((size_t)b * N + n) * C);
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

// ---- the large entry -----------------------------------------------------------------------------------------------------------------
// The plan of a call, or the status and message of the arguments it rejects (the entry and the plan query answer alike)
static int lovasz_checked_plan(LovaszPlan* p, int B, int N, int C, int tile_log2, int slab)
{
    *p = lovasz_large_plan(B, N, C, tile_log2, slab);
    SPH3D_REQUIRE(p->bad != kLovBadDims, "lovasz_softmax_large: bad dims B=%d N=%d C=%d", B, N, C);
    SPH3D_REQUIRE(p->bad != kLovBadSize, "lovasz_softmax_large: bad dims B=%d N=%d C=%d (B N C <= 2^40, B C < 2^31, B < 2^16)", B, N, C);
    if (p->bad == kLovBigN || p->bad == kLovBigC) {
        set_error("lovasz_softmax_large: N=%d C=%d is not covered (N <= %d rows per block, C <= %d classes)", N, C, kLovLargeMaxN,
                  kLovLargeMaxC);
        return SPH3D_EUNSUPPORTED;
    }
    SPH3D_REQUIRE(p->bad != kLovBadTile, "lovasz_softmax_large: tile_log2 %d is neither 0 (the default, %d) nor in [%d, %d]", tile_log2,
                  kLovDefaultTileLog2, kLovMinTileLog2, kLovMaxTileLog2);
    SPH3D_REQUIRE(p->bad != kLovBadSlab, "lovasz_softmax_large: slab %d is neither 0 (the plan's choice) nor in [1, C = %d]", slab, C);
    return SPH3D_OK;
}

extern "C" int sph3d_lovasz_softmax_large_supported(int N, int C)
{
    return (N > 0 && N <= kLovLargeMaxN && C > 0 && C <= kLovLargeMaxC) ? 1 : 0;
}

// 0 for arguments the entry rejects
extern "C" size_t sph3d_lovasz_softmax_large_workspace(int B, int N, int C)
{
    return (size_t)lovasz_large_plan(B, N, C, 0, 0).workspace_bytes;
}

extern "C" int sph3d_lovasz_softmax_large_plan(int B, int N, int C, int tile_log2, int slab, long long* out)
{
    LovaszPlan p;
    const int rc = lovasz_checked_plan(&p, B, N, C, tile_log2, slab);
    if (rc) return rc;
    SPH3D_REQUIRE(out != nullptr, "sph3d_lovasz_softmax_large_plan: out is NULL");
    static_assert(offsetof(LovaszPlan, bad) == SPH3D_LOVASZ_PLAN_FIELDS * sizeof(long long),
                  "the plan starts with the documented fields, in their order");
    memcpy(out, &p, SPH3D_LOVASZ_PLAN_FIELDS * sizeof(long long));
    return SPH3D_OK;
}

extern "C" int sph3d_lovasz_softmax_large(int B, int N, int C, const float* logits, const long long* label, const float* inner,
                                          long long ignore, float* probs, float* coef, float* class_loss, float* loss, float* dlogits,
                                          int* order, void* workspace, size_t workspace_bytes, int tile_log2, int slab,
                                          sph3d_stream_t stream)
{
    LovaszPlan p;
    int rc = lovasz_checked_plan(&p, B, N, C, tile_log2, slab);
    if (rc) return rc;
    if (B == 0) return SPH3D_OK;
    SPH3D_REQUIRE(logits != nullptr && label != nullptr && probs != nullptr && coef != nullptr && class_loss != nullptr &&
                      loss != nullptr,
                  "lovasz_softmax_large: null logits, label, probs, coef, class_loss or loss");
    if (workspace == nullptr || workspace_bytes < (size_t)p.workspace_bytes || (reinterpret_cast<size_t>(workspace) & 15) != 0) {
        set_error("lovasz_softmax_large: workspace of %zu bytes, 16-byte aligned, required (got %zu)", (size_t)p.workspace_bytes,
                  workspace_bytes);
        return SPH3D_EWORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    char* ws = (char*)workspace;
    unsigned long long* kbuf[2] = {(unsigned long long*)(ws + p.off_keys0), (unsigned long long*)(ws + p.off_keys1)};
    int* tilecnt = (int*)(ws + p.off_tilecnt);
    float* partial = (float*)(ws + p.off_partial);
    int* count = (int*)(ws + p.off_count);
    int* badflag = (int*)(ws + p.off_bad);
    const int T = (int)p.tile, npad = (int)p.npad, mtiles = (int)p.mtiles;

    hipLaunchKernelGGL(lovasz_probs_kernel, dim3((unsigned)p.probs_grid), dim3(256), 0, st, (long long)B * N, C, logits, probs);
    rc = zero_async(count, sizeof(int) * ((size_t)B * C + (size_t)B), st, "lovasz_softmax_large: memset");
    if (rc != SPH3D_OK) return rc;
    hipLaunchKernelGGL(lovasz_large_count_kernel, dim3((unsigned)p.count_grid, B), dim3(kLovThreads), 0, st, N, C, label, inner, ignore,
                       (const float*)probs, count, badflag);
    for (int c0 = 0; c0 < C; c0 += (int)p.slab) {
        const int S = C - c0 < (int)p.slab ? C - c0 : (int)p.slab;
        rc = launch_lds(lovasz_run_sort_kernel, dim3((unsigned)p.runs, S, B), dim3(kLovThreads), (size_t)p.sort_lds, st,
                        "sph3d_lovasz_softmax_large", N, C, T, npad, c0, label, inner, ignore, (const float*)probs, coef, kbuf[0]);
        if (rc != SPH3D_OK) return rc;
        int cur = 0;
        for (int pass = 0; pass < (int)p.passes; pass++, cur ^= 1)
            hipLaunchKernelGGL(lovasz_merge_kernel, dim3(mtiles, S, B), dim3(kLovMergeBlock), 0, st, npad, T << pass,
                               (const unsigned long long*)kbuf[cur], kbuf[cur ^ 1]);
        const unsigned long long* sorted = kbuf[cur];
        hipLaunchKernelGGL(lovasz_tile_count_kernel, dim3(mtiles, S, B), dim3(kLovThreads), 0, st, npad, sorted, tilecnt);
        hipLaunchKernelGGL(lovasz_finish_kernel, dim3(mtiles, S, B), dim3(kLovThreads), 0, st, N, C, npad, c0, sorted,
                           (const int*)tilecnt, (const int*)count, (const int*)badflag, coef, partial, order);
        hipLaunchKernelGGL(lovasz_class_kernel, dim3(S, B), dim3(64), 0, st, C, mtiles, c0, (const float*)partial, (const int*)count,
                           (const int*)badflag, class_loss);
    }
    hipLaunchKernelGGL(lovasz_large_grad_kernel, dim3(dlogits != nullptr ? (unsigned)p.grad_grid : 1u, B), dim3(kLovThreads), 0, st, N, C,
                       label, inner, ignore, (const float*)probs, (const float*)coef, (const float*)class_loss, (const int*)count,
                       (const int*)badflag, loss, dlogits);
    return check_launch("sph3d_lovasz_softmax_large");
}
