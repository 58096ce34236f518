// idsample.hip — keyed inverse-density sampling (include/sph3d.h: sph3d_ids_sample; harness/idsample.py states it in numpy).
//
// The sample of a cloud is a pure function of (nn_dist, nn_count, seed, step, level): point i of cloud b gets the 64-bit key
//     (bits(t) << 32) | i,   t = E / w,   E = sph3d_neglog32(u),   u from the counter-based draws of feed_draws.hpp,
// w the mean of its neighbour distances (sequential fp32 adds, one correctly rounded division), t = +inf for a point without a
// positive finite weight — and the output is the low words of the S smallest keys in ascending order.  Keys are distinct (the
// index is part of them), so the order is total: nothing here depends on which workgroup or lane comes first.
//
//   ids_sort_kernel   one workgroup per (cloud, chunk of kIdsChunk points): every thread computes its points' keys straight from
//                     nn_dist / nn_count into LDS, the tail of the power-of-two sort size is padded with all-ones keys, and the
//                     workgroup runs a bitonic sort there (8 bytes per key: 16 KiB of LDS for a full chunk).  A
//                     one-chunk cloud writes out[] directly; otherwise the sorted chunk goes to the caller's workspace.
//   ids_rank_kernel   more than one chunk: one thread per key.  Final rank = position in the key's own sorted chunk + the count
//                     of smaller keys in every other chunk (binary search; exact because keys are distinct).  A key whose rank
//                     is below S stores its index to out[rank].  A key leaves as soon as its rank reaches S.
// No atomics, no floating-point reduction across lanes.  LDS exchanges: a compare-exchange distance j >= 32 keys has the lanes
// of a wave on consecutive 8-byte words (conflict-free ds_read_b64 / ds_write_b64); the short distances j < 32 leave gaps of j
// keys between runs of j, at most a 2-way conflict on the 64-bank read.
#pragma clang fp contract(off)
#include "common.hpp"
#include "feed_draws.hpp"
#include "../../include/sph3d_log32.h"

namespace sph3d {

// keys per workgroup (a power of two).  Measured at 16 x 8192 -> 2048 (tools/exp_ids.py): chunks of 8192 keys — one workgroup per
// cloud, 91 barrier steps of 4 exchanges per thread on 16 of the 256 CUs — 214 us; chunks of 2048 — 64 workgroups, 66 steps of
// one exchange per thread, then the rank pass — 83 us.
constexpr int kIdsChunk = 2048;
constexpr int kIdsMaxN = 1 << 20;               // 512 chunks: the rank pass is linear in the chunk count per key
constexpr int kIdsLevels = 8;
constexpr unsigned long long kIdsPad = ~0ull;   // above every key: bits(t) <= 0x7f800000 (+inf)

static inline int ids_chunks(int N) { return (N + kIdsChunk - 1) / kIdsChunk; }

__device__ __forceinline__ unsigned long long ids_key(const float* __restrict__ dist, int count, int K, bool vec,
                                                      unsigned long long ck, unsigned long long purpose, unsigned i)
{
    const int c = count < K ? count : K;
    float t = __int_as_float(0x7f800000);
    if (c > 0) {
        float sum;
        if (vec) {
            // (whole 16-byte groups of the row: the slots >= c of the last group are loaded and not used)
            const float4* __restrict__ d4 = reinterpret_cast<const float4*>(dist);
            float4 v = d4[0];
            sum = v.x;
            if (c > 1) sum = sum + v.y;
            if (c > 2) sum = sum + v.z;
            if (c > 3) sum = sum + v.w;
            for (int k = 4; k < c; k += 4) {
                v = d4[k >> 2];
                sum = sum + v.x;
                if (k + 1 < c) sum = sum + v.y;
                if (k + 2 < c) sum = sum + v.z;
                if (k + 3 < c) sum = sum + v.w;
            }
        } else {
            sum = dist[0];
            for (int k = 1; k < c; ++k) sum = sum + dist[k];
        }
        const float w = sum / (float)c;
        if (isfinite(w) && w > 0.0f) {
            const unsigned hi = (unsigned)(feed_draw(ck, purpose, i) >> 32);
            const float u = (float)((hi >> 8) + 1u) * 0x1p-24f;
            t = sph3d_neglog32(u) / w;
        }
    }
    return ((unsigned long long)(unsigned)__float_as_int(t) << 32) | i;
}

// P = the sort size (a power of two, n <= P <= kIdsChunk, P >= 2 * blockDim is not required); dynamic LDS: P keys
__global__ void __launch_bounds__(1024)
ids_sort_kernel(int N, int K, int S, int chunks, int P, int vec, const float* __restrict__ nn_dist, const int* __restrict__ nn_count,
                unsigned long long seed, unsigned long long step, int level, int* __restrict__ out,
                unsigned long long* __restrict__ sorted)
{
    extern __shared__ unsigned long long keys[];
    const int b = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x - b * chunks;
    const int base = chunk * kIdsChunk;
    const int n = min(N - base, kIdsChunk);                           // points of this chunk (>= 1)
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    const unsigned long long purpose = kFeedIds + (unsigned long long)level;
    for (int p = (int)threadIdx.x; p < P; p += (int)blockDim.x) {
        unsigned long long key = kIdsPad;
        if (p < n) {
            const size_t row = (size_t)b * N + (size_t)(base + p);
            key = ids_key(nn_dist + row * (size_t)K, nn_count[row], K, vec != 0, ck, purpose, (unsigned)(base + p));
        }
        keys[p] = key;
    }
    __syncthreads();
    // bitonic network: stage k merges runs of k keys, step j exchanges keys j apart; pair t of a step is (i, i | j) with i = t
    // with a zero inserted at bit log2(j)
    const int half = P >> 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = (int)threadIdx.x; t < half; t += (int)blockDim.x) {
                const int i = 2 * t - (t & (j - 1));
                const int l = i | j;
                const unsigned long long a = keys[i], c = keys[l];
                const bool up = (i & k) == 0;
                if ((a > c) == up) {
                    keys[i] = c;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
    }
    if (chunks == 1) {
        // (S <= N = n <= P: the first S keys are points)
        for (int p = (int)threadIdx.x; p < S; p += (int)blockDim.x) out[(size_t)b * S + p] = (int)(unsigned)keys[p];
    } else {
        // (here P == kIdsChunk)
        unsigned long long* dst = sorted + (size_t)blockIdx.x * kIdsChunk;
        for (int p = (int)threadIdx.x; p < kIdsChunk; p += (int)blockDim.x) dst[p] = keys[p];
    }
}

// number of keys of the ascending run s[0, kIdsChunk) that are below `key`
__device__ __forceinline__ int ids_below(const unsigned long long* __restrict__ s, unsigned long long key)
{
    int lo = 0;
#pragma unroll
    for (int w = kIdsChunk >> 1; w > 0; w >>= 1)
        if (s[lo + w - 1] < key) lo += w;
    return lo + (s[lo] < key ? 1 : 0);
}

__global__ void __launch_bounds__(256)
ids_rank_kernel(int B, int S, int chunks, const unsigned long long* __restrict__ sorted, int* __restrict__ out)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)B * chunks * kIdsChunk) return;
    const int pos = (int)(g % kIdsChunk);
    if (pos >= S) return;                                             // (its rank is at least its position)
    const size_t bc = g / kIdsChunk;
    const int b = (int)(bc / chunks), own = (int)(bc - (size_t)b * chunks);
    const unsigned long long key = sorted[g];
    if (key == kIdsPad) return;
    const unsigned long long* cloud = sorted + (size_t)b * chunks * kIdsChunk;
    int rank = pos;
    for (int c = 0; c < chunks && rank < S; ++c)
        if (c != own) rank += ids_below(cloud + (size_t)c * kIdsChunk, key);
    if (rank < S) out[(size_t)b * S + rank] = (int)(unsigned)key;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_ids_sample_chunk(void) { return kIdsChunk; }

extern "C" size_t sph3d_ids_sample_workspace(int B, int N)
{
    if (B <= 0 || N <= kIdsChunk) return 0;
    return sizeof(unsigned long long) * (size_t)B * ids_chunks(N) * kIdsChunk;
}

extern "C" int sph3d_ids_sample(int B, int N, int K, int S, const float* nn_dist, const int* nn_count, unsigned long long seed,
                                unsigned long long step, int level, int* out, void* workspace, size_t workspace_bytes,
                                sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && N > 0 && K > 0 && S > 0, "InverseDensitySample: positive B, N, K, S required, got B=%d N=%d K=%d S=%d",
                  B, N, K, S);
    SPH3D_REQUIRE(S <= N, "InverseDensitySample: S=%d samples of N=%d points", S, N);
    SPH3D_REQUIRE(level >= 0 && level < kIdsLevels, "InverseDensitySample: level %d outside 0..%d", level, kIdsLevels - 1);
    SPH3D_REQUIRE(nn_dist != nullptr && nn_count != nullptr && out != nullptr, "InverseDensitySample: null nn_dist, nn_count or out");
    if (N > kIdsMaxN) {
        set_error("InverseDensitySample: N=%d exceeds the supported %d points", N, kIdsMaxN);
        return SPH3D_EUNSUPPORTED;
    }
    const int chunks = ids_chunks(N);
    if ((long long)B * chunks > (1ll << 26)) {                      // (the rank pass: B * chunks * kIdsChunk / 256 workgroups)
        set_error("InverseDensitySample: B=%d clouds of %d chunks exceed one launch", B, chunks);
        return SPH3D_EUNSUPPORTED;
    }
    const size_t need = sph3d_ids_sample_workspace(B, N);
    if (need && (workspace == nullptr || workspace_bytes < need)) {
        set_error("InverseDensitySample: workspace %zu B < required %zu B", workspace_bytes, need);
        return SPH3D_EWORKSPACE;
    }
    SPH3D_REQUIRE(need == 0 || ((uintptr_t)workspace & 7) == 0, "InverseDensitySample: workspace must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    int P = kIdsChunk;
    if (chunks == 1) {
        P = 128;
        while (P < N) P <<= 1;
    }
    const int threads = P / 2 < kRefBlock ? P / 2 : kRefBlock;        // 64 .. 1024
    unsigned long long* sorted = (unsigned long long*)workspace;
    const int vec = (K & 3) == 0 && ((uintptr_t)nn_dist & 15) == 0;   // rows of whole, aligned 16-byte groups
    int rc = launch_lds(ids_sort_kernel, dim3((unsigned)(B * chunks)), dim3(threads), sizeof(unsigned long long) * (size_t)P, st,
                        "sph3d_ids_sample", N, K, S, chunks, P, vec, nn_dist, nn_count, seed, step, level, out, sorted);
    if (rc) return rc;
    if (chunks > 1) {
        rc = check_launch("sph3d_ids_sample (sort pass)");
        if (rc) return rc;
        const size_t total = (size_t)B * chunks * kIdsChunk;
        hipLaunchKernelGGL(ids_rank_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, B, S, chunks,
                           (const unsigned long long*)sorted, out);
    }
    return check_launch("sph3d_ids_sample");
}
