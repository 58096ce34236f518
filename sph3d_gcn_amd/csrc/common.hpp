// common.hpp — shared host/device helpers for libsph3d (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/sph3d.h"

namespace sph3d {

constexpr int kWave = 64;           // CDNA wavefront width
constexpr int kRefGrid = 32;        // the reference launches every kernel <<<32,1024>>>;
constexpr int kRefBlock = 1024;     // its thread->work mapping defines the radius-growth chains and FPS tie-break

// ---- host-side status plumbing ------------------------------------------------
void set_error(const char* fmt, ...);   // stores a thread-local message (api.cpp)

#define SPH3D_REQUIRE(cond, ...)                    \
    do {                                            \
        if (!(cond)) {                              \
            ::sph3d::set_error(__VA_ARGS__);        \
            return SPH3D_EINVAL;                    \
        }                                           \
    } while (0)

static inline int check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return SPH3D_ELAUNCH;
    }
    return SPH3D_OK;
}

// api.cpp: a library-owned device buffer of at least `bytes` for work queued on `stream` of the current device (one per
// (device, stream, kind), grown on demand and kept; nullptr if the allocation fails or the stream is being captured).
// kind 0: only for state that is dead when the call's last kernel has run.  kind 1: zero-initialised; its users leave the
// first 16 KB zero (arrival counters, gemm.hip)
void* stream_scratch(hipStream_t stream, size_t bytes, int kind = 0);

static inline int check_hip(hipError_t e, const char* what)
{
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return SPH3D_ELAUNCH;
    }
    return SPH3D_OK;
}

static inline hipStream_t as_stream(sph3d_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Launch of a kernel whose dynamic LDS may exceed what a kernel gets without asking: above kOptIn bytes (64 KB; the separable
// convolutions ask from 48 KB, as they always have) the kernel's limit is raised first, on every such launch: nothing is cached.
// -> SPH3D_OK once the launch is queued; the caller still ends its launches with check_launch().  `who` heads the error message.
template <size_t kOptIn = 64 * 1024, class... Params, class... Args>
static inline int launch_lds(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const char* who,
                             Args... args)
{
    if (lds > kOptIn) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e));
            return SPH3D_ELAUNCH;
        }
    }
    kern<<<grid, block, lds, stream>>>(args...);
    return SPH3D_OK;
}

// The library reads no environment except the test hooks listed in sph3d.h; they reach code that ordinary inputs rarely do.
// -> the variable's value as atoi() reads it, `unset` if it is not set.  Each caller decides when it reads (per call or once).
static inline int test_hook(const char* name, int unset)
{
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}

// gemm.hip: deterministic mode (sph3d_set_deterministic) is on
bool deterministic_on();

// graph.hip: stream-ordered zero fill of `bytes` bytes at `p` (4-byte aligned, bytes % 4 == 0).  hipMemsetAsync's fill kernel
// runs 256 workgroups whatever the size: 245 us for the 17 MB of level-0 segment counters (70 GB/s; rocprofv3 trace of round 5);
// large fills go through a kernel that covers the chip (8 us for the same buffer), small ones stay with the runtime.
int zero_async(void* p, size_t bytes, hipStream_t stream, const char* what);

// ---- workspace layout of the transposed-graph build (graph.hip; the fused neighbour search of nnquery.hip / nngrid.hip writes
// the counting phase's three arrays itself) ----
//   deg[B*L]        in-degree of every (source, bin) segment, L = N*F; the fill cursors' zero state after the scan
//   bin_used[F]     1 for every bin that occurs
//   status[B*chunks]  64-bit (flag << 32 | value) words of the single-pass scan (decoupled look-back), chunks = ceil(L / 2048)
//   slot_pos[B*M*K] position of every edge inside its segment
// deg .. status are ONE zero fill (tg_zero_words words from deg).
constexpr int kTgChunk = 2048;
struct TgWs {
    int* deg; int* bin_used; unsigned long long* status; int* slot_pos; int L; int chunks; size_t zero_words; size_t total_words;
};
static inline TgWs tg_ws(void* workspace, int B, int N, int M, int K, int F)
{
    TgWs w;
    w.L = N * F;
    w.chunks = (w.L + kTgChunk - 1) / kTgChunk;
    const size_t head = ((size_t)B * w.L + (size_t)F + 1) & ~(size_t)1;         // status words are 8-byte aligned
    w.deg = (int*)workspace;
    w.bin_used = w.deg + (size_t)B * w.L;
    w.status = reinterpret_cast<unsigned long long*>(w.deg + head);
    w.zero_words = head + 2 * (size_t)B * w.chunks;
    w.slot_pos = w.deg + w.zero_words;
    w.total_words = w.zero_words + (size_t)B * M * K;
    return w;
}

// ---- the transposed graph itself inside a caller's workspace (the one-call gradients of conv3d.hip and pool3d.hip): the arrays
// sph3d_graph_transpose writes, each on a 256-byte boundary, then the build's scratch (tg_ws above).  workspace == nullptr:
// null pointers, `bytes` is what the size functions report.
struct TgLayout {
    int* offsets; int* key; float* scale; int* active; void* scratch; size_t scratch_bytes; size_t bytes;
};
static inline TgLayout tg_layout(void* workspace, int B, int N, int M, int K, int F)
{
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = workspace ? (char*)workspace + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    TgLayout t;
    t.offsets = (int*)take(sizeof(int) * (size_t)B * ((size_t)N * F + 1));
    t.key = (int*)take(sizeof(int) * (size_t)B * M * K);
    t.scale = (float*)take(sizeof(float) * (size_t)B * M * K);
    t.active = (int*)take(sizeof(int) * ((size_t)F + 1));
    const size_t scratch_off = off;
    t.scratch = take(sph3d_graph_transpose_workspace(B, N, M, K, F));
    t.scratch_bytes = off - scratch_off;
    t.bytes = off;
    return t;
}

// ---- packed entries of the transposed graph (round 6) ----------------------------------------------------------------------------
// ent_scale == NULL: an entry word of ent_key is  m | nn_count[m] << 24  (un-weighted graphs with at most 2^24 rows and K <= 255):
// the fill pass then makes ONE scattered 4-byte store per edge instead of two, and a consumer takes the row and its 1 / count
// (the same correctly rounded division the fill pass would have done) from one word.
constexpr unsigned kTgKeyMask = 0x00ffffffu;
static inline bool tg_packable(int M, int K, const void* weight) { return weight == nullptr && M <= (1 << 24) && K <= 255; }

// ---- row link of a pooling graph (graph.hip: sph3d_gather_rows_link; pool3d.hip: sph3d_max_pool3d_grad_rows) ----
// first[b, p] = 0 or (1 + pooled row that copies intra row p) | kRowLinkMore when further rows copy p (they follow in next[])
constexpr unsigned kRowLinkMore = 0x80000000u;
constexpr unsigned kRowLinkMask = 0x7fffffffu;

// ---- the vote entry points (vote.hip, shapeeval.hip): what they all require of a batch and its row range; `what` heads the message
constexpr int kVoteMaxClasses = 64;
static inline int vote_check_args(const char* what, int B, int C, int num_blocks, long long total_rows, long long row_base,
                                  long long batch_rows)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "%s: batch 0<B<=65535 required, got %d", what, B);
    SPH3D_REQUIRE(C > 0 && C <= kVoteMaxClasses, "%s: 0<C<=%d classes required, got %d", what, kVoteMaxClasses, C);
    SPH3D_REQUIRE(num_blocks > 0 && total_rows > 0, "%s: empty pool (num_blocks=%d total_rows=%lld)", what, num_blocks, total_rows);
    SPH3D_REQUIRE(row_base >= 0 && batch_rows > 0 && batch_rows <= 0x7fffffffll && row_base + batch_rows <= total_rows,
                  "%s: rows [%lld, %lld + %lld) are not a range of the pool's %lld", what, row_base, row_base, batch_rows, total_rows);
    return SPH3D_OK;
}

// ---- device helpers -----------------------------------------------------------
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ int tg_key(int word, bool packed) { return packed ? (int)((unsigned)word & kTgKeyMask) : word; }
__device__ __forceinline__ float tg_packed_scale(int word) { return 1.0f / (float)((unsigned)word >> 24); }

// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ int prefix_popc(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// ELU (alpha = 1) as every kernel with a fused tail takes it (norm.hip, gemm.hip, sepring.hip, sepconv.hip).  exp(y) - 1 through
// v_exp_f32: absolute error ~1e-7 on (-inf, 0] (measured: tools/micro/elu_err.hip), far inside the 1e-5 activation bound; the software
// expm1f made the HBM-streaming kernels of norm.hip VALU-bound (3.7 ms/step, no better than the unfused torch ops)
__device__ __forceinline__ float elu1(float y) { return y > 0.f ? y : __expf(y) - 1.f; }

// make a wave-uniform int visibly scalar to the compiler
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniformf(float v)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// vote.hip, scene.hip, shapeeval.hip — the rows of cloud b of a batch inside the pool and inside the batch's row range: -> n (0: the cloud takes no part), lo = its first pool row
__device__ __forceinline__ long long vote_cloud(int b, int P, long long T, const long long* __restrict__ offsets,
                                                const int* __restrict__ block_ids, long long row_base, long long batch_rows,
                                                long long& lo)
{
    const int id = block_ids[b];
    lo = 0;
    if (id < 0 || id >= P) return 0;
    lo = offsets[id];
    const long long n = offsets[id + 1] - lo;
    if (n <= 0 || n > 0x7fffffffll || lo < 0 || lo + n > T) return 0;
    if (lo < row_base || lo + n > row_base + batch_rows) return 0;
    return n;
}

// the first maximum of v[lo, lo + n) as np.argmax takes it (a NaN is a maximum); finite: all C entries of v are finite
__device__ __forceinline__ int vote_argmax(const float* __restrict__ v, int lo, int n, int C, bool& finite)
{
    finite = true;
    for (int c = 0; c < lo; ++c) finite = finite && isfinite(v[c]);
    float best = v[lo];
    int arg = lo;
    finite = finite && isfinite(best);
    for (int c = lo + 1; c < lo + n; ++c) {
        const float x = v[c];
        finite = finite && isfinite(x);
        if (!isnan(best) && (x > best || isnan(x))) {
            best = x;
            arg = c;
        }
    }
    for (int c = lo + n; c < C; ++c) finite = finite && isfinite(v[c]);
    return arg;
}

// scene.hip, prep.hip — a float as an unsigned whose integer order is the float order (for atomicMin / atomicMax), and back
__device__ __forceinline__ unsigned f2ord(float f)
{
    const unsigned u = (unsigned)__float_as_int(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o)
{
    return __int_as_float((int)((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o));
}

// XCD-affine work decode.  Workgroup `bid` runs on XCD (bid % 8) (observed placement, used for
// L2 locality only, never for correctness).  Clouds are dealt to XCDs round-robin so that all
// workgroups of one cloud share one L2: returns (cloud, part) for this block or cloud = -1.
// Batches of fewer than five clouds would leave XCDs without work that way (ONE cloud: the whole launch on 32 of the 256 CUs —
// the ScanNet-shape line until round 5): such a batch gives every cloud 2, 4 or 8 XCDs and deals the cloud's parts over them.
__host__ __device__ __forceinline__ int xcd_spread_log2(int B) { return B >= 5 ? 0 : (B >= 3 ? 1 : (B == 2 ? 2 : 3)); }
__device__ __forceinline__ void xcd_decode(int bid, int B, int parts, int& cloud, int& part)
{
    const int ls = xcd_spread_log2(B), s = 1 << ls;       // XCDs per cloud
    const int x = bid & 7;
    const int y = bid >> 3;
    const int pps = (parts + s - 1) >> ls;                // parts per XCD of a cloud
    const int row = y / pps;
    cloud = (x >> ls) + (8 >> ls) * row;
    part = (x & (s - 1)) + s * (y - row * pps);
    if (cloud >= B || part >= parts) cloud = -1;
}
static inline int xcd_grid(int B, int parts)
{
    const int ls = xcd_spread_log2(B), s = 1 << ls, cpr = 8 >> ls;
    return 8 * ((B + cpr - 1) / cpr) * ((parts + s - 1) >> ls);
}

}  // namespace sph3d
