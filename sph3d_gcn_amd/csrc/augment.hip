// augment.hip — the augmentation stage: what the indoor-segmentation recipes published since the reference add to its 2019 recipe
// (chromatic auto-contrast, translation, jitter and drop; flips; anisotropic scaling; elastic distortion; Mix3D scene mixing),
// applied IN PLACE to an assembled batch on the feed's stream.  harness/augment.py states every transform in numpy; the integer
// outputs (label, inner, which slot came from which cloud, the counters) equal that statement bit for bit, the floats are held to
// the per-element bound tests/_augment_ref.py derives.  The draws are feed_draws.hpp's, purposes 32..38.
//
//   gates     bit k of cloud b: enabled and hi32(draw(ck_b, kFeedAugGate, k)) < threshold[k]; MIX from the even cloud of the pair
//   launches  1 stats     one workgroup per HALF cloud: min / max of xyz and rgb (selection: exact and order-free); the gates, the
//                         cell boxes' start values and the mixed-pairs counter per cloud
//             2 main      one thread per point: MIX exchange, flips, scaling, colour; int atomic min / max of the pass-1 cell box
//             3 lattice   pass 1: one workgroup per (cloud, component): raw draws over the cloud's node box, three separable
//                         [1,2,3,2,1] blurs, kept as EXACT int32 (|value| <= 729 * 2^20), in LDS where the box fits
//             4 elastic   pass 1: 8 loads per component and a trilinear blend per point; the pass-2 cell box
//             5, 6        the same for pass 2
//   MIX       the thread of slot j >= N/2 of the EVEN cloud of a mixed pair reads both elements, transforms each with its
//             destination's parameters and writes them crossed; every element has exactly one reader and one writer.
//   skipping  a pass whose node box leaves [-500, 500] or holds more than max_nodes nodes leaves its cloud alone and counts it.
// Evaluating the blurred field per point instead would be 5^3 raw nodes for each of 8 corners, 216 distinct draws per point and
// pass: 2 * 216 * 131072 = 57 M splitmix rounds per batch against 2 * 3 * ~6000 * 16 = 0.6 M here.
#include <limits.h>

#include "feed_draws.hpp"

namespace sph3d {

enum : unsigned { kAugMix = 1, kAugFlipX = 2, kAugFlipY = 4, kAugAscale = 8, kAugElastic = 16, kAugContrast = 32,
                  kAugCtranslate = 64, kAugCjitter = 128, kAugCdrop = 256, kAugColour = 32 | 64 | 128 | 256 };
constexpr int kAugGates = 9;
constexpr int kAugNodeLimit = 500;          // node indices are biased by 512 into 10 bits of the draw's counter
constexpr int kAugLdsNodes = 8192;          // two int buffers of this many nodes are the lattice kernel's 64 KB of LDS
constexpr int kAugHead = 40;                // workspace words per cloud in front of the lattices:
constexpr int kAugCells = 24;               //   [0, 24) float min[6], max[6] (xyz, rgb) of slots [0, h) and of [h, N)
constexpr int kAugGateWord = 36;            //   [24, 36) int cell min[3], max[3] of pass 1 and of pass 2;  [36] the gates

static inline size_t aug_head_bytes(int B) { return ((size_t)B * kAugHead * 4 + 255) & ~(size_t)255; }

__device__ __forceinline__ int aug_cell(float x, float inv_g)
{
    return (int)floorf(fminf(fmaxf(x * inv_g, -1000.f), 1000.f));
}

// the cells [min, max] of a cloud -> may the pass run, and the cells per axis
__device__ __forceinline__ bool aug_box(const int* cell, int max_nodes, int& nx, int& ny, int& nz)
{
    nx = ny = nz = 0;
    for (int a = 0; a < 3; ++a)
        if (cell[a] > cell[3 + a] || cell[a] - 2 < -kAugNodeLimit || cell[3 + a] + 3 > kAugNodeLimit) return false;
    nx = cell[3] - cell[0] + 1; ny = cell[4] - cell[1] + 1; nz = cell[5] - cell[2] + 1;
    return (long long)(nx + 5) * (ny + 5) * (nz + 5) <= (long long)max_nodes;
}

__device__ __forceinline__ unsigned aug_gates(const sph3d_augment_params& p, unsigned long long seed, unsigned long long step,
                                              int b, int B)
{
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    unsigned m = 0;
    for (int k = 1; k < kAugGates; ++k)
        if (((p.enable >> k) & 1u) && (unsigned long long)(unsigned)(feed_draw(ck, kFeedAugGate, (unsigned)k) >> 32) < p.threshold[k])
            m |= 1u << k;
    const int even = b & ~1;
    if ((p.enable & kAugMix) && even + 1 < B) {
        const unsigned long long ek = feed_cloud_key(seed, step, (unsigned)even);
        if ((unsigned long long)(unsigned)(feed_draw(ek, kFeedAugGate, 0u) >> 32) < p.threshold[0]) m |= kAugMix;
    }
    return m;
}

// ---- 1: statistics of a half cloud ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void aug_stats_kernel(int B, int N, int C, sph3d_augment_params p, unsigned long long seed,
                                                         unsigned long long step, const float* __restrict__ points,
                                                         float* __restrict__ head, long long* __restrict__ status)
{
    __shared__ float red[16][12];
    const int b = (int)(blockIdx.x >> 1), half = (int)(blockIdx.x & 1), h = N / 2;
    const int lo = half ? h : 0, hi = half ? N : h;
    float mn[6], mx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
    const float* src = points + (size_t)b * N * C;
    for (int j = lo + (int)threadIdx.x; j < hi; j += 1024) {
        const float* e = src + (size_t)j * C;
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float v = e[a]; mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v); }
        if (p.rgb_offset >= 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { const float v = e[p.rgb_offset + a]; mn[3 + a] = fminf(mn[3 + a], v); mx[3 + a] = fmaxf(mx[3 + a], v); }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
        }
    const int wave = (int)(threadIdx.x >> 6);
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { red[wave][k] = mn[k]; red[wave][6 + k] = mx[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        float v = red[0][threadIdx.x];
        for (int w = 1; w < 16; ++w) v = threadIdx.x < 6 ? fminf(v, red[w][threadIdx.x]) : fmaxf(v, red[w][threadIdx.x]);
        head[(size_t)b * kAugHead + half * 12 + threadIdx.x] = v;
    }
    if (half == 0 && threadIdx.x == 0) {
        int* hi_ = reinterpret_cast<int*>(head) + (size_t)b * kAugHead;
        for (int q = 0; q < 2; ++q)
            for (int a = 0; a < 3; ++a) { hi_[kAugCells + q * 6 + a] = INT_MAX; hi_[kAugCells + q * 6 + 3 + a] = INT_MIN; }
        const unsigned g = aug_gates(p, seed, step, b, B);
        hi_[kAugGateWord] = (int)g;
        if ((g & kAugMix) && !(b & 1) && status != nullptr) atomicAdd(reinterpret_cast<unsigned long long*>(status + 2), 1ull);
    }
}

// int min / max of a cloud's cells: one set of atomics per wave where the wave serves one cloud (cloud < 0: the lane has none)
__device__ __forceinline__ void aug_cell_reduce(int cloud, const int (&c)[3], int* head_i, int pass)
{
    const unsigned long long act = __ballot(cloud >= 0);
    if (act == 0ull) return;
    const int first = __shfl(cloud, __ffsll((long long)act) - 1);
    if (__all(cloud < 0 || cloud == first)) {
        int mn[3], mx[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = cloud >= 0 ? c[a] : INT_MAX;
            mx[a] = cloud >= 0 ? c[a] : INT_MIN;
            for (int off = 32; off > 0; off >>= 1) {
                mn[a] = min(mn[a], __shfl_xor(mn[a], off));
                mx[a] = max(mx[a], __shfl_xor(mx[a], off));
            }
        }
        if (lane_id() == 0) {
            int* cell = head_i + (size_t)first * kAugHead + kAugCells + pass * 6;
#pragma unroll
            for (int a = 0; a < 3; ++a) { atomicMin(cell + a, mn[a]); atomicMax(cell + 3 + a, mx[a]); }
        }
    } else if (cloud >= 0) {
        int* cell = head_i + (size_t)cloud * kAugHead + kAugCells + pass * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(cell + a, c[a]); atomicMax(cell + 3 + a, c[a]); }
    }
}

// ---- 2: everything but the elastic passes ----------------------------------------------------------------------------------------
struct AugElem { float v[9]; int label, inner; };

__device__ __forceinline__ void aug_load(AugElem& e, int C, const float* points, const int* label, const int* inner, long long i)
{
#pragma unroll
    for (int c = 0; c < 9; ++c) e.v[c] = c < C ? points[i * C + c] : 0.f;
    e.label = label[i];
    e.inner = inner != nullptr ? inner[i] : 0;
}
__device__ __forceinline__ void aug_store(const AugElem& e, int C, float* points, int* label, int* inner, long long i)
{
#pragma unroll
    for (int c = 0; c < 9; ++c)
        if (c < C) points[i * C + c] = e.v[c];
    label[i] = e.label;
    if (inner != nullptr) inner[i] = e.inner;
}
__device__ __forceinline__ float aug_clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// e: an element of cloud `src` that lands in slot `slot` of cloud `dst` with gates g.  s0 / s1: the statistics of the two halves
// of src; d0 / d1: of the halves that make up dst after MIX.
__device__ __forceinline__ void aug_transform(AugElem& e, const sph3d_augment_params& p, unsigned g, unsigned long long ck,
                                              unsigned slot, const float* s0, const float* s1, const float* d0, const float* d1)
{
    if (g & kAugMix) {
        e.v[0] -= (fminf(s0[0], s1[0]) + fmaxf(s0[6], s1[6])) * 0.5f;
        e.v[1] -= (fminf(s0[1], s1[1]) + fmaxf(s0[7], s1[7])) * 0.5f;
        e.v[2] -= fminf(s0[2], s1[2]);
    }
    const int no = p.normal_offset;
    if (g & kAugFlipX) { e.v[0] = -e.v[0]; if (no >= 0) e.v[3] = -e.v[3]; }       // (no is 3 or -1)
    if (g & kAugFlipY) { e.v[1] = -e.v[1]; if (no >= 0) e.v[4] = -e.v[4]; }
    if (g & kAugAscale) {
        float s[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[a] = 0.9f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedAugScale, (unsigned)a) >> 32));
            e.v[a] *= s[a];
        }
        if (no >= 0) {
            const float n0 = e.v[3] / s[0], n1 = e.v[4] / s[1], n2 = e.v[5] / s[2];
            const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
            const bool ok = len > 0.f;
            e.v[3] = ok ? n0 / len : n0; e.v[4] = ok ? n1 / len : n1; e.v[5] = ok ? n2 / len : n2;
        }
    }
    if (!(g & kAugColour)) return;
    const float lo = p.rgb_lo, hi = p.rgb_hi, range = hi - lo;
    float alpha = 0.f, z[3] = {0.f, 0.f, 0.f};
    if (g & kAugContrast) alpha = feed_uniform((unsigned)(feed_draw(ck, kFeedAugContrast, 0u) >> 32));
    if (g & kAugCjitter) {
        float unused;
        feed_normal_pair(feed_draw(ck, kFeedAugCnoise, 2u * slot), z[0], z[1]);
        feed_normal_pair(feed_draw(ck, kFeedAugCnoise, 2u * slot + 1u), z[2], unused);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float c = a == 0 ? e.v[3] : (a == 1 ? e.v[4] : e.v[5]);           // rgb_offset 3 ..
        if (p.rgb_offset == 6) c = e.v[6 + a];                            // .. or 6
        if (g & kAugContrast) {
            const float mn = fminf(d0[3 + a], d1[3 + a]), mx = fmaxf(d0[9 + a], d1[9 + a]);
            if (mx > mn) {
                const float cp = lo + (c - mn) * (range / (mx - mn));
                c = (1.0f - alpha) * c + alpha * cp;
            }
        }
        if (g & kAugCtranslate) {
            const float u = feed_uniform((unsigned)(feed_draw(ck, kFeedAugCtrans, (unsigned)a) >> 32));
            c = aug_clip(c + (u - 0.5f) * (0.1f * range), lo, hi);
        }
        if (g & kAugCjitter) c = aug_clip(c + (0.01f * range) * z[a], lo, hi);
        if (g & kAugCdrop) c = (lo + hi) * 0.5f;
        if (p.rgb_offset == 6) e.v[6 + a] = c;
        else if (a == 0) e.v[3] = c;
        else if (a == 1) e.v[4] = c;
        else e.v[5] = c;
    }
}

__global__ __launch_bounds__(256) void aug_main_kernel(int B, int N, int C, sph3d_augment_params p, unsigned long long seed,
                                                       unsigned long long step, float* points, int* label, int* inner, float* head)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool live = i < (long long)B * N;
    const int b = live ? (int)(i / N) : 0;
    const unsigned slot = (unsigned)(i - (long long)b * N);
    int* head_i = reinterpret_cast<int*>(head);
    const unsigned g = live ? (unsigned)head_i[(size_t)b * kAugHead + kAugGateWord] : 0u;
    const bool cross = live && (g & kAugMix) && (int)slot >= N / 2;
    if (cross && (b & 1)) live = false;                    // the even cloud's thread serves both elements
    int d0 = -1, d1 = -1, c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    if (live && !cross && g != 0u) {
        const float* s0 = head + (size_t)b * kAugHead;
        const float* s1 = s0 + 12;
        const float* m1 = (g & kAugMix) ? head + (size_t)(b ^ 1) * kAugHead + 12 : s1;
        AugElem e;
        aug_load(e, C, points, label, inner, i);
        aug_transform(e, p, g, feed_cloud_key(seed, step, (unsigned)b), slot, s0, s1, s0, m1);
        aug_store(e, C, points, label, inner, i);
        if (g & kAugElastic) { d0 = b; for (int a = 0; a < 3; ++a) c0[a] = aug_cell(e.v[a], p.inv_g[0]); }
    } else if (live && cross) {
        // (b, slot) -> (b + 1, slot) and (b + 1, slot) -> (b, slot): both read before either is written
        const long long k = i + N;
        const unsigned g1 = (unsigned)head_i[(size_t)(b + 1) * kAugHead + kAugGateWord];
        const float* a0 = head + (size_t)b * kAugHead;
        const float* b0 = head + (size_t)(b + 1) * kAugHead;
        AugElem ea, eb;
        aug_load(ea, C, points, label, inner, i);
        aug_load(eb, C, points, label, inner, k);
        aug_transform(ea, p, g1, feed_cloud_key(seed, step, (unsigned)(b + 1)), slot, a0, a0 + 12, b0, a0 + 12);
        aug_transform(eb, p, g, feed_cloud_key(seed, step, (unsigned)b), slot, b0, b0 + 12, a0, b0 + 12);
        aug_store(ea, C, points, label, inner, k);
        aug_store(eb, C, points, label, inner, i);
        if (g & kAugElastic) { d0 = b; for (int a = 0; a < 3; ++a) c0[a] = aug_cell(eb.v[a], p.inv_g[0]); }
        if (g1 & kAugElastic) { d1 = b + 1; for (int a = 0; a < 3; ++a) c1[a] = aug_cell(ea.v[a], p.inv_g[0]); }
    }
    if (p.enable & kAugElastic) {
        aug_cell_reduce(d0, c0, head_i, 0);
        aug_cell_reduce(d1, c1, head_i, 0);
    }
}

// ---- 3, 5: the blurred lattice of one (cloud, component) ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void aug_lattice_kernel(int pass, sph3d_augment_params p, unsigned long long seed,
                                                           unsigned long long step, const int* __restrict__ head_i, int* lat,
                                                           long long* __restrict__ status)
{
    __shared__ int lds[2][kAugLdsNodes];
    const int b = (int)(blockIdx.x / 3), comp = (int)(blockIdx.x % 3);
    if (!((unsigned)head_i[(size_t)b * kAugHead + kAugGateWord] & kAugElastic)) return;
    const int* cell = head_i + (size_t)b * kAugHead + kAugCells + pass * 6;
    int nx, ny, nz;
    if (!aug_box(cell, p.max_nodes, nx, ny, nz)) {
        if (comp == 0 && threadIdx.x == 0 && status != nullptr) atomicAdd(reinterpret_cast<unsigned long long*>(status + pass), 1ull);
        return;
    }
    const int ry = ny + 5, rz = nz + 5, ox = nx + 1, oy = ny + 1, oz = nz + 1;
    const int raw = (nx + 5) * ry * rz;                                     // <= max_nodes
    int* out = lat + (size_t)(b * 3 + comp) * 3 * p.max_nodes;
    int* A = raw <= kAugLdsNodes ? lds[0] : out + p.max_nodes;
    int* Bf = raw <= kAugLdsNodes ? lds[1] : out + 2 * (size_t)p.max_nodes;
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    const unsigned bx = (unsigned)(cell[0] - 2 + 512), by = (unsigned)(cell[1] - 2 + 512), bz = (unsigned)(cell[2] - 2 + 512);
    for (int n = (int)threadIdx.x; n < raw; n += 1024) {
        const int iz = n % rz, t = n / rz, iy = t % ry, ix = t / ry;
        const unsigned counter = ((bx + (unsigned)ix) << 20) | ((by + (unsigned)iy) << 10) | (bz + (unsigned)iz);
        const unsigned long long w = feed_draw(ck, kFeedAugField + (unsigned long long)pass, counter);
        A[n] = (int)((w >> (21 * comp)) & 0x1fffffull) - (1 << 20);
    }
    __syncthreads();
    const int sx = ry * rz;
    for (int n = (int)threadIdx.x; n < ox * sx; n += 1024) {                // x: A [nx+5][ry][rz] -> Bf [ox][ry][rz]
        const int* s = A + n;
        Bf[n] = s[0] + 2 * s[sx] + 3 * s[2 * sx] + 2 * s[3 * sx] + s[4 * sx];
    }
    __syncthreads();
    for (int n = (int)threadIdx.x; n < ox * oy * rz; n += 1024) {           // y: Bf [ox][ry][rz] -> A [ox][oy][rz]
        const int iz = n % rz, t = n / rz, iy = t % oy, ix = t / oy;
        const int* s = Bf + ((size_t)ix * ry + iy) * rz + iz;
        A[n] = s[0] + 2 * s[rz] + 3 * s[2 * rz] + 2 * s[3 * rz] + s[4 * rz];
    }
    __syncthreads();
    for (int n = (int)threadIdx.x; n < ox * oy * oz; n += 1024) {           // z: A [ox][oy][rz] -> out [ox][oy][oz]
        const int iz = n % oz, t = n / oz;
        const int* s = A + (size_t)t * rz + iz;
        out[n] = s[0] + 2 * s[1] + 3 * s[2] + 2 * s[3] + s[4];
    }
}

// ---- 4, 6: the displacement of every point -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aug_elastic_kernel(int B, int N, int C, int pass, sph3d_augment_params p, float* points,
                                                          int* head_i, const int* __restrict__ lat)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < (long long)B * N;
    const int b = live ? (int)(i / N) : 0;
    int d = -1, cn[3] = {0, 0, 0};
    if (live && ((unsigned)head_i[(size_t)b * kAugHead + kAugGateWord] & kAugElastic)) {
        float* e = points + i * C;
        float x[3] = {e[0], e[1], e[2]};
        const int* cell = head_i + (size_t)b * kAugHead + kAugCells + pass * 6;
        int n[3];
        if (aug_box(cell, p.max_nodes, n[0], n[1], n[2])) {
            int l[3];
            float w[3][2];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float t = x[a] * p.inv_g[pass], fl = floorf(t), f = t - fl;
                l[a] = min(max((int)fl - cell[a], 0), n[a] - 1);            // (inside the box by construction; never an address outside it)
                w[a][0] = 1.0f - f;
                w[a][1] = f;
            }
            const int oy = n[1] + 1, oz = n[2] + 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int* L = lat + (size_t)(b * 3 + c) * 3 * p.max_nodes + ((size_t)l[0] * oy + l[1]) * oz + l[2];
                float acc = 0.f;
#pragma unroll
                for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                        for (int dz = 0; dz < 2; ++dz)
                            acc = acc + ((w[0][dx] * w[1][dy]) * w[2][dz]) * (float)L[((size_t)dx * oy + dy) * oz + dz];
                x[c] = x[c] + acc * p.scale[pass];
            }
            e[0] = x[0]; e[1] = x[1]; e[2] = x[2];
        }
        if (pass == 0) { d = b; for (int a = 0; a < 3; ++a) cn[a] = aug_cell(x[a], p.inv_g[1]); }
    }
    if (pass == 0) aug_cell_reduce(d, cn, head_i, 1);
}

}  // namespace sph3d

using namespace sph3d;

extern "C" size_t sph3d_augment_workspace(int B, int N, int max_nodes)
{
    if (B <= 0 || N <= 0 || max_nodes <= 0) return 0;
    return aug_head_bytes(B) + (size_t)B * 9 * (size_t)max_nodes * sizeof(int);
}

extern "C" int sph3d_augment_apply(int B, int N, int C, float* points, int* label, int* inner, unsigned long long seed,
                                   unsigned long long step, sph3d_augment_params params, void* workspace, size_t workspace_bytes,
                                   long long* status, sph3d_stream_t stream)
{
    const sph3d_augment_params& p = params;
    SPH3D_REQUIRE(B > 0 && N > 0, "augment_apply: B>0 and N>0 required, got %d, %d", B, N);
    SPH3D_REQUIRE(C == 3 || C == 6 || C == 9, "augment_apply: C must be 3, 6 or 9, got %d", C);
    SPH3D_REQUIRE((long long)B * N <= 0x7fffffffll, "augment_apply: B*N=%lld too large", (long long)B * N);
    SPH3D_REQUIRE(points != nullptr && label != nullptr, "augment_apply: null points or label");
    SPH3D_REQUIRE(p.enable < (1u << kAugGates), "augment_apply: enable has bits above %d", kAugGates - 1);
    for (int k = 0; k < kAugGates; ++k)
        SPH3D_REQUIRE(p.threshold[k] <= (1ull << 32), "augment_apply: threshold[%d] above 2^32", k);
    SPH3D_REQUIRE(p.rgb_offset == -1 || ((p.rgb_offset == 3 || p.rgb_offset == 6) && p.rgb_offset + 3 <= C),
                  "augment_apply: rgb_offset must be -1, 3 or 6 and inside C=%d channels, got %d", C, p.rgb_offset);
    SPH3D_REQUIRE(p.normal_offset == -1 || (p.normal_offset == 3 && C >= 6 && p.rgb_offset != 3),
                  "augment_apply: normal_offset must be -1 or 3, beside the colour, got %d", p.normal_offset);
    SPH3D_REQUIRE(!(p.enable & kAugColour) || p.rgb_offset >= 0, "augment_apply: a colour bit is enabled but rgb_offset is -1");
    SPH3D_REQUIRE(p.rgb_hi > p.rgb_lo, "augment_apply: rgb range (%g, %g) is empty", (double)p.rgb_lo, (double)p.rgb_hi);
    if (p.enable == 0u) return SPH3D_OK;                  // every cloud is copied bit for bit: it is in place already
    SPH3D_REQUIRE(p.max_nodes >= 216 && p.max_nodes <= (1 << 24), "augment_apply: 216<=max_nodes<=2^24 required, got %d", p.max_nodes);
    if (p.enable & kAugElastic)
        for (int q = 0; q < 2; ++q)
            SPH3D_REQUIRE(p.inv_g[q] > 0.f && p.inv_g[q] <= 1e6f && p.scale[q] >= 0.f && p.scale[q] <= 1.f,
                          "augment_apply: elastic pass %d: bad 1/g or scale", q);
    SPH3D_REQUIRE(workspace != nullptr && (reinterpret_cast<size_t>(workspace) & 15) == 0, "augment_apply: workspace must be 16-byte aligned");
    const size_t need = (p.enable & kAugElastic) ? sph3d_augment_workspace(B, N, p.max_nodes) : aug_head_bytes(B);
    if (workspace_bytes < need) {
        set_error("augment_apply: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return SPH3D_EWORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    float* head = reinterpret_cast<float*>(workspace);
    int* head_i = reinterpret_cast<int*>(workspace);
    int* lat = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + aug_head_bytes(B));
    const unsigned grid = (unsigned)(((long long)B * N + 255) / 256);
    hipLaunchKernelGGL(aug_stats_kernel, dim3(2u * (unsigned)B), dim3(1024), 0, st, B, N, C, p, seed, step, points, head, status);
    hipLaunchKernelGGL(aug_main_kernel, dim3(grid), dim3(256), 0, st, B, N, C, p, seed, step, points, label, inner, head);
    if (p.enable & kAugElastic)
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(aug_lattice_kernel, dim3(3u * (unsigned)B), dim3(1024), 0, st, pass, p, seed, step, head_i, lat, status);
            hipLaunchKernelGGL(aug_elastic_kernel, dim3(grid), dim3(256), 0, st, B, N, C, pass, p, points, head_i, lat);
        }
    return check_launch("sph3d_augment_apply");
}
