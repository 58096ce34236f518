// fuzzy.hip — the fuzzy spherical kernel for gfx950: trilinear bin weights, the depthwise convolution over them, its gradients.
//
// The hard kernel (sphere_bin.hpp) puts a neighbour into one of the n*p*q + 1 bins, so the layer jumps when a neighbour crosses a
// bin boundary.  Here a neighbour contributes to the (up to) eight bins around it with interpolation weights that sum to 1
// (the fuzzy spherical kernel of the reference authors' follow-up work; the reference tree has no such op: DESIGN.md 4.27).
//
// Two words per graph slot:
//   filt_index  1 + i0 + n*j0 + n*p*k0, the hard format applied to the LOWER corner (sector i0, band j0, shell k0);
//               0 = a centre slot (the hard rule) or a slot k >= nn_count
//   filt_frac   fa8 | fb8 << 8 | fg8 << 16: the position between the lower and the upper corner per axis in 1/256
// A consumer's axis weights are the integers (256 - f8, f8); a corner's coefficient is the product of its three axis weights
// times 2^-24: an integer of at most 2^24 scaled by a power of two, exact in fp32, and the eight sum to exactly 1 in any order.
// The azimuth wraps (upper sector (i0 + 1) mod n), elevation and radius clamp (upper = min(lower + 1, last)); corners that coincide
// simply add up.  A centre slot is bin 0 with coefficient 1.  Every corner bin is clamped to [0, F - 1]; bits 24..31 are ignored.
//
// Kernels (lanes own output columns / channels; the filter table of a column slice sits in LDS; a slice is at most 512 columns
// and 64 KB, so wide layers run as several slices and no shape is refused for its width):
//   fuzzy_kernel_kernel   one lane per slot, coalesced over k
//   fuzzy_fwd_kernel      per edge: blend the (non-zero) corner rows into the edge's effective weight, one fmaf per gathered value
//   fuzzy_gf_kernel       grad_filter: walks the forward graph by rows with go[m] / cnt in registers, plain LDS
//                         read-modify-writes (one per corner) into a table whose columns each belong to ONE lane (no atomics); row
//                         groups of a workgroup own a table each, summed in group order; one partial table per workgroup goes to
//                         the caller's workspace and fuzzy_gf_reduce adds them in workgroup order: the same bits on every run
//   fuzzy_gi_kernel       grad_input: gather over the un-binned transposed graph whose entries name the EDGE m*K + k
//                         (sph3d_graph_transpose_finish_edges, graph.hip), so the kernel reads the slot's two words
// W lanes (a power of two) share a graph row / source point, CPT adjacent columns each.  With W >= 64 (slices wider than 32
// columns) a wave works on ONE row: its lanes decode 64 slots at once, one each (the two integer divisions and the eight
// coefficient products happen once per slot, not once per lane and slot), and the slot in turn is broadcast through v_readlane,
// so bins and coefficients are scalars and a zero coefficient is a scalar branch around its row.  Narrower slices put several rows
// into a wave and every lane decodes its row's slot itself.
// No float atomics anywhere.  Built with -ffp-contract=off: every fmaf below is written out.
#include "common.hpp"
#include "sphere_bin.hpp"

namespace sph3d {

constexpr int kFuzzyMaxCols = 512;          // columns of a slice (four per lane, 128 lanes per row)
constexpr int kFuzzyLdsWords = 16384;       // 64 KB of table per workgroup
constexpr int kFuzzyMaxParts = 2048;        // partial filter-gradient tables of a launch (one per workgroup of a column slice) ...
constexpr long long kFuzzyMaxPartBytes = 64ll << 20;   // ... halved, down to 128, while they would take more than this

// ---- the slot's two words -------------------------------------------------------------------------------------------------------
// lower corner and fraction byte of a clamped axis (elevation, radius): v in units of bins, `last` = bins - 1
__device__ __forceinline__ void fuzzy_axis_clamped(float v, int last, int& lo, int& f8)
{
    const float a = v - 0.5f;
    const float fl = floorf(a);
    const float fr = a - fl;
    int b = (int)floorf(fr * 256.0f);
    b = b < 255 ? b : 255;
    if (!(fl >= 0.0f)) { lo = 0; f8 = 0; return; }                   // below the first bin centre (and NaN)
    if (fl >= (float)last) { lo = last; f8 = 0; return; }            // at or above the last bin centre
    lo = (int)fl;
    f8 = b;
}

__device__ __forceinline__ void fuzzy_slot(float dx, float dy, float dz, float dist, float radius, int n, int p, int q,
                                           int& index, int& frac)
{
    // alpha, beta, gamma and the centre rule exactly as sphere_bin<false> (sphere_bin.hpp :49-68)
    const float M_EPSf = 1.01e-3F;
    float dist2D = dx * dx + dy * dy;
    dist2D = sqrtf(dist2D);
    index = 0;
    frac = 0;
    if (!(dist > M_EPSf && (double)fabsf(dist - M_EPSf) > 1e-6)) return;
    float theta = sph3d_atan2f(dy, dx);
    float phi = sph3d_atan2f(dz, dist2D);
    theta = (float)((double)theta < SPH3D_PI ? (double)theta : -SPH3D_PI);
    theta = (float)((double)theta > -SPH3D_PI ? (double)theta : -SPH3D_PI);
    theta = (float)((double)theta + SPH3D_PI);
    phi = (float)((double)phi < (SPH3D_PI / 2) ? (double)phi : (SPH3D_PI / 2));
    phi = (float)((double)phi > (-SPH3D_PI / 2) ? (double)phi : (-SPH3D_PI / 2));
    phi = (float)((double)phi + SPH3D_PI / 2);
    const float alpha = (float)((double)((theta * (float)n) / 2.0f) / SPH3D_PI);
    const float beta = (float)((double)(phi * (float)p) / SPH3D_PI);
    const float gamma = (dist * (float)q) / (radius + 1e-6F);
    // azimuth: periodic
    const float a = alpha - 0.5f;
    const float fl = floorf(a);
    const float fa = a - fl;
    int fa8 = (int)floorf(fa * 256.0f);
    fa8 = fa8 < 255 ? fa8 : 255;                    // a just under 0: a - floor(a) rounds to 1
    int i0 = (int)fl % n;
    i0 = i0 < 0 ? i0 + n : i0;
    int j0, fb8, k0, fg8;
    fuzzy_axis_clamped(beta, p - 1, j0, fb8);
    fuzzy_axis_clamped(gamma, q - 1, k0, fg8);
    index = 1 + i0 + n * j0 + n * p * k0;
    frac = fa8 | (fb8 << 8) | (fg8 << 16);
}

__global__ __launch_bounds__(256) void fuzzy_kernel_kernel(
    int B, int N, int M, int K, int n, int p, int q, float radius,
    const float* __restrict__ database, const float* __restrict__ query,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const float* __restrict__ nnDist,
    int* __restrict__ filtIndex, int* __restrict__ filtFrac)
{
    const long long total = (long long)B * M * K;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long row = e / K;          // (b, m)
        const int k = (int)(e - row * K);
        const int b = (int)(row / M);
        int index = 0, frac = 0;              // slots >= nn_count stay 0
        if (k < nnCount[row]) {
            const int ptID = nnIndex[e];
            const float* pt = database + ((size_t)b * N + ptID) * 3;
            const float* qp = query + (size_t)row * 3;
            fuzzy_slot(pt[0] - qp[0], pt[1] - qp[1], pt[2] - qp[2], nnDist[e], radius, n, p, q, index, frac);
        }
        filtIndex[e] = index;
        filtFrac[e] = frac;
    }
}

// ---- a slot's corners as every consumer derives them ----------------------------------------------------------------------------
// corner t: bit 0 = upper sector, bit 1 = upper band, bit 2 = upper shell
__device__ __forceinline__ void fuzzy_corners(int fi, int fr, int n, int p, int q, int F, int (&bin)[8], float (&coef)[8])
{
    int i[2] = {0, 0}, j[2] = {0, 0}, k[2] = {0, 0};
    int wa[2] = {256, 0}, wb[2] = {256, 0}, wg[2] = {256, 0};
    const bool centre = fi <= 0;
    if (!centre) {
        const int c = fi - 1;
        const int t = c / n;
        i[0] = c - t * n;
        k[0] = t / p;
        j[0] = t - k[0] * p;
        i[1] = i[0] + 1 == n ? 0 : i[0] + 1;
        j[1] = j[0] + 1 < p ? j[0] + 1 : p - 1;
        k[1] = k[0] + 1 < q ? k[0] + 1 : q - 1;
        const int fa = fr & 255, fb = (fr >> 8) & 255, fg = (fr >> 16) & 255;
        wa[0] = 256 - fa; wa[1] = fa;
        wb[0] = 256 - fb; wb[1] = fb;
        wg[0] = 256 - fg; wg[1] = fg;
    }
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const int a = t & 1, b = (t >> 1) & 1, g = (t >> 2) & 1;
        int f = centre ? 0 : 1 + i[a] + n * j[b] + n * p * k[g];
        f = f < 0 ? 0 : (f >= F ? F - 1 : f);
        bin[t] = f;
        coef[t] = (float)(wa[a] * wb[b] * wg[g]) * 0x1p-24f;
    }
}

// A decoded slot in one lane's registers (bins packed nine bits each), and the slot a wave (UNI) or a lane works on
struct FuzzyDec {
    int pk[3];
    float coef[8];
};

__device__ __forceinline__ void fuzzy_decode(int fi, int fr, int n, int p, int q, int F, FuzzyDec& d)
{
    int bin[8];
    fuzzy_corners(fi, fr, n, p, q, F, bin, d.coef);
    d.pk[0] = bin[0] | (bin[1] << 9) | (bin[2] << 18);
    d.pk[1] = bin[3] | (bin[4] << 9) | (bin[5] << 18);
    d.pk[2] = bin[6] | (bin[7] << 9);
}

__device__ __forceinline__ float readlane_f(float v, int j)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// the slot of lane j of the wave, in scalars (UNI), or the lane's own
template <bool UNI>
__device__ __forceinline__ void fuzzy_take(const FuzzyDec& d, int j, int (&bin)[8], float (&coef)[8])
{
    int pk[3];
#pragma unroll
    for (int i = 0; i < 3; i++) pk[i] = UNI ? __builtin_amdgcn_readlane(d.pk[i], j) : d.pk[i];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        bin[t] = (pk[t / 3] >> (9 * (t % 3))) & 511;
        coef[t] = UNI ? readlane_f(d.coef[t], j) : d.coef[t];
    }
}

// lanes per row and columns per lane of a slice of `cols` columns (<= 512): W a power of two, W * CPT >= cols
static inline void fuzzy_shape(int cols, int& W, int& CPT)
{
    CPT = cols <= 64 ? 1 : (cols <= 128 ? 2 : 4);
    const int need = (cols + CPT - 1) / CPT;
    W = 1;
    while (W < need) W <<= 1;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// grid (column slices, row blocks); 256 / W rows at a time; table [F][S4 * 4], S4 * 4 >= JS
template <int CPT, bool UNI>
__global__ __launch_bounds__(256) void fuzzy_fwd_kernel(
    int B, int N, int M, int K, int F, int C, int r, int n, int p, int q, int JS, int S4, int W,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ filtIndex,
    const int* __restrict__ filtFrac, const float* __restrict__ input, const float* __restrict__ filter, float* __restrict__ output)
{
    extern __shared__ __attribute__((aligned(16))) float tab[];
    const int J = C * r;
    const int j_lo = (int)blockIdx.x * JS;
    const int js = (J - j_lo) < JS ? (J - j_lo) : JS;
    const int stride = S4 * 4;
    for (int i = (int)threadIdx.x; i < F * js; i += 256) {
        const int f = i / js, j = i - f * js;
        tab[f * stride + j] = filter[(size_t)f * J + j_lo + j];
    }
    __syncthreads();
    const int lane = (int)threadIdx.x & 63;
    const int tc = (int)threadIdx.x & (W - 1), tr = (int)threadIdx.x / W, G = 256 / W;
    const int col0 = tc * CPT;
    const int rcol = col0 < js ? col0 : 0;          // lanes past the slice read (and drop) the first columns: never past the table
    int ch[CPT];
    bool live[CPT];
#pragma unroll
    for (int v = 0; v < CPT; v++) {
        live[v] = col0 + v < js;
        ch[v] = live[v] ? (j_lo + col0 + v) / r : 0;
    }
    const long long nrows = (long long)B * M;
    for (long long row = (long long)blockIdx.y * G + tr; row < nrows; row += (long long)gridDim.y * G) {
        int cnt = nnCount[row];
        if (UNI) cnt = uniform(cnt);
        const int lim = cnt < K ? cnt : K;
        const int b = (int)(row / M);
        const float* __restrict__ xb = input + (size_t)b * N * C;
        float acc[CPT];
#pragma unroll
        for (int v = 0; v < CPT; v++) acc[v] = 0.0f;
        auto fetch = [&](int id, float (&x)[CPT]) {
            const float* __restrict__ xrow = xb + (size_t)id * C;
#pragma unroll
            for (int v = 0; v < CPT; v++) x[v] = live[v] ? xrow[ch[v]] : 0.0f;
        };
        auto edge = [&](const float (&x)[CPT], const int (&bin)[8], const float (&coef)[8]) {
            float w[CPT];
#pragma unroll
            for (int v = 0; v < CPT; v++) w[v] = 0.0f;
#pragma unroll
            for (int t = 0; t < 8; t++) {
                if (coef[t] != 0.0f) {
                    const float* __restrict__ trow = tab + (bin[t] * S4) * 4 + rcol;
#pragma unroll
                    for (int v = 0; v < CPT; v++) w[v] = fmaf(coef[t], trow[v], w[v]);
                }
            }
#pragma unroll
            for (int v = 0; v < CPT; v++) {
                if (live[v]) acc[v] = fmaf(x[v], w[v], acc[v]);
            }
        };
        int bin[8];
        float coef[8];
        if (UNI) {
            for (int k0 = 0; k0 < lim; k0 += 64) {
                const int chunk = (lim - k0) < 64 ? (lim - k0) : 64;
                FuzzyDec d = {};
                int id = 0;
                if (lane < chunk) {
                    const long long e = row * K + k0 + lane;
                    id = nnIndex[e];
                    fuzzy_decode(filtIndex[e], filtFrac[e], n, p, q, F, d);
                }
                for (int j = 0; j < chunk; j += 4) {            // four gathers in flight, then their four blends
                    float x[4][CPT];
#pragma unroll
                    for (int u = 0; u < 4; u++) fetch(__builtin_amdgcn_readlane(id, (j + u) < chunk ? (j + u) : (chunk - 1)), x[u]);
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (j + u < chunk) {
                            fuzzy_take<true>(d, j + u, bin, coef);
                            edge(x[u], bin, coef);
                        }
                    }
                }
            }
        } else {
            for (int k = 0; k < lim; k++) {
                const long long e = row * K + k;
                fuzzy_corners(filtIndex[e], filtFrac[e], n, p, q, F, bin, coef);
                float x[CPT];
                fetch(nnIndex[e], x);
                edge(x, bin, coef);
            }
        }
        const float inv = lim > 0 ? 1.0f / (float)cnt : 0.0f;
#pragma unroll
        for (int v = 0; v < CPT; v++) {
            if (live[v]) output[(size_t)row * J + j_lo + col0 + v] = acc[v] * inv;
        }
    }
}

// ---- grad_filter -----------------------------------------------------------------------------------------------------------------
// grid (column slices, parts); G row groups of W lanes, each with its own table [F][S4 * 4]; partial[part][F][J]
template <int CPT, bool UNI>
__global__ __launch_bounds__(256) void fuzzy_gf_kernel(
    int B, int N, int M, int K, int F, int C, int r, int n, int p, int q, int JS, int S4, int W, int G,
    const int* __restrict__ nnIndex, const int* __restrict__ nnCount, const int* __restrict__ filtIndex,
    const int* __restrict__ filtFrac, const float* __restrict__ input, const float* __restrict__ gradOutput,
    float* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float tab[];
    const int J = C * r;
    const int j_lo = (int)blockIdx.x * JS;
    const int js = (J - j_lo) < JS ? (J - j_lo) : JS;
    const int stride = S4 * 4;
    const int tsize = F * stride;
    for (int i = (int)threadIdx.x; i < G * tsize; i += 256) tab[i] = 0.0f;
    __syncthreads();
    const int lane = (int)threadIdx.x & 63;
    const int tc = (int)threadIdx.x & (W - 1), tr = (int)threadIdx.x / W;
    if (tr < G) {
        float* my = tab + tr * tsize;
        const int col0 = tc * CPT;
        int ch[CPT];
        bool live[CPT];
#pragma unroll
        for (int v = 0; v < CPT; v++) {
            live[v] = col0 + v < js;
            ch[v] = live[v] ? (j_lo + col0 + v) / r : 0;
        }
        const long long nrows = (long long)B * M;
        for (long long row = (long long)blockIdx.y * G + tr; row < nrows; row += (long long)gridDim.y * G) {
            int cnt = nnCount[row];
            if (UNI) cnt = uniform(cnt);
            const int lim = cnt < K ? cnt : K;
            if (lim <= 0) continue;
            const int b = (int)(row / M);
            const float* __restrict__ xb = input + (size_t)b * N * C;
            const float inv = 1.0f / (float)cnt;
            float g[CPT];
#pragma unroll
            for (int v = 0; v < CPT; v++) g[v] = live[v] ? gradOutput[(size_t)row * J + j_lo + col0 + v] * inv : 0.0f;
            auto fetch = [&](int id, float (&x)[CPT]) {
                const float* __restrict__ xrow = xb + (size_t)id * C;
#pragma unroll
                for (int v = 0; v < CPT; v++) x[v] = live[v] ? xrow[ch[v]] : 0.0f;
            };
            auto edge = [&](const float (&x)[CPT], const int (&bin)[8], const float (&coef)[8]) {
                float gx[CPT];
#pragma unroll
                for (int v = 0; v < CPT; v++) gx[v] = g[v] * x[v];
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    if (coef[t] != 0.0f && col0 < js) {             // these columns of every table row are this lane's alone
                        float* cell = my + (bin[t] * S4) * 4 + col0;
#pragma unroll
                        for (int v = 0; v < CPT; v++) cell[v] = fmaf(coef[t], gx[v], cell[v]);
                    }
                }
            };
            int bin[8];
            float coef[8];
            if (UNI) {
                for (int k0 = 0; k0 < lim; k0 += 64) {
                    const int chunk = (lim - k0) < 64 ? (lim - k0) : 64;
                    FuzzyDec d = {};
                    int id = 0;
                    if (lane < chunk) {
                        const long long e = row * K + k0 + lane;
                        id = nnIndex[e];
                        fuzzy_decode(filtIndex[e], filtFrac[e], n, p, q, F, d);
                    }
                    for (int j = 0; j < chunk; j += 4) {        // four gathers in flight, then their read-modify-writes
                        float x[4][CPT];
#pragma unroll
                        for (int u = 0; u < 4; u++) fetch(__builtin_amdgcn_readlane(id, (j + u) < chunk ? (j + u) : (chunk - 1)), x[u]);
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            if (j + u < chunk) {
                                fuzzy_take<true>(d, j + u, bin, coef);
                                edge(x[u], bin, coef);
                            }
                        }
                    }
                }
            } else {
                for (int k = 0; k < lim; k++) {
                    const long long e = row * K + k;
                    fuzzy_corners(filtIndex[e], filtFrac[e], n, p, q, F, bin, coef);
                    float x[CPT];
                    fetch(nnIndex[e], x);
                    edge(x, bin, coef);
                }
            }
        }
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < F * js; i += 256) {
        const int f = i / js, j = i - f * js;
        float s = tab[f * stride + j];
        for (int g = 1; g < G; g++) s += tab[g * tsize + f * stride + j];
        partial[((size_t)blockIdx.y * F + f) * J + j_lo + j] = s;
    }
}

__global__ __launch_bounds__(256) void fuzzy_gf_reduce(int total, int parts, const float* __restrict__ partial,
                                                        float* __restrict__ gradFilter)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= total) return;
    float s = partial[i];
    for (int y = 1; y < parts; y++) s += partial[(size_t)y * total + i];
    gradFilter[i] = s;
}

// ---- grad_input ------------------------------------------------------------------------------------------------------------------
// grid (channel slices, source blocks); table [F][S4 * 4] of the slice's CS * r columns; entEdge: in-edge lists of edge ids m*K + k
template <int CPT, bool UNI>
__global__ __launch_bounds__(256) void fuzzy_gi_kernel(
    int B, int N, int M, int K, int F, int C, int r, int n, int p, int q, int CS, int S4, int W,
    const int* __restrict__ offsets, const int* __restrict__ entEdge, const int* __restrict__ nnCount,
    const int* __restrict__ filtIndex, const int* __restrict__ filtFrac, const float* __restrict__ filter,
    const float* __restrict__ gradOutput, float* __restrict__ gradInput)
{
    extern __shared__ __attribute__((aligned(16))) float tab[];
    const int J = C * r;
    const int c_lo = (int)blockIdx.x * CS;
    const int cs = (C - c_lo) < CS ? (C - c_lo) : CS;
    const int js = cs * r, j_lo = c_lo * r;
    const int stride = S4 * 4;
    for (int i = (int)threadIdx.x; i < F * js; i += 256) {
        const int f = i / js, j = i - f * js;
        tab[f * stride + j] = filter[(size_t)f * J + j_lo + j];
    }
    __syncthreads();
    const int lane = (int)threadIdx.x & 63;
    const int tc = (int)threadIdx.x & (W - 1), tr = (int)threadIdx.x / W, G = 256 / W;
    const int c0 = tc * CPT;
    bool live[CPT];
#pragma unroll
    for (int v = 0; v < CPT; v++) live[v] = c0 + v < cs;
    const long long nsrc = (long long)B * N;
    const long long MK = (long long)M * K;
    for (long long s = (long long)blockIdx.y * G + tr; s < nsrc; s += (long long)gridDim.y * G) {
        const int b = (int)(s / N);
        const int nloc = (int)(s - (long long)b * N);
        const int* __restrict__ ob = offsets + (size_t)b * ((size_t)N + 1) + nloc;
        int e0 = ob[0], e1 = ob[1];
        if (UNI) {
            e0 = uniform(e0);
            e1 = uniform(e1);
        }
        float acc[CPT];
#pragma unroll
        for (int v = 0; v < CPT; v++) acc[v] = 0.0f;
        // the row's first two columns per channel (all of them at r <= 2) are fetched ahead of the blends, four edges at a time
        auto fetch = [&](int m, float (&gv)[CPT][2]) {
            const float* __restrict__ gorow = gradOutput + ((size_t)b * M + m) * J + j_lo;
#pragma unroll
            for (int v = 0; v < CPT; v++) {
                gv[v][0] = live[v] ? gorow[(c0 + v) * r] : 0.0f;
                gv[v][1] = (live[v] && r > 1) ? gorow[(c0 + v) * r + 1] : 0.0f;
            }
        };
        auto edge = [&](int m, float inv, const float (&gv)[CPT][2], const int (&bin)[8], const float (&coef)[8]) {
            const float* __restrict__ gorow = gradOutput + ((size_t)b * M + m) * J + j_lo;
            if (r == 2) {
                // the plans' multiplier: a channel's two table words as one 8-byte LDS read (word by word, lanes two words
                // apart collide on the banks); the same fmaf sequence as the general loop below
#pragma unroll
                for (int v = 0; v < CPT; v++) {
                    if (!live[v]) continue;
                    float w0 = 0.0f, w1 = 0.0f;
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        if (coef[c] != 0.0f) {
                            const float2 t2 = *reinterpret_cast<const float2*>(tab + (bin[c] * S4) * 4 + (c0 + v) * 2);
                            w0 = fmaf(coef[c], t2.x, w0);
                            w1 = fmaf(coef[c], t2.y, w1);
                        }
                    }
                    float t = fmaf(gv[v][0], w0, 0.0f);
                    t = fmaf(gv[v][1], w1, t);
                    acc[v] = fmaf(t, inv, acc[v]);
                }
                return;
            }
#pragma unroll
            for (int v = 0; v < CPT; v++) {
                if (!live[v]) continue;
                float t = 0.0f;
                for (int rho = 0; rho < r; rho++) {
                    const int jj = (c0 + v) * r + rho;
                    float w = 0.0f;
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        if (coef[c] != 0.0f) w = fmaf(coef[c], tab[(bin[c] * S4) * 4 + jj], w);
                    }
                    const float g = rho == 0 ? gv[v][0] : (rho == 1 ? gv[v][1] : gorow[jj]);
                    t = fmaf(g, w, t);
                }
                acc[v] = fmaf(t, inv, acc[v]);
            }
        };
        int bin[8];
        float coef[8];
        if (UNI) {
            for (int i0 = e0; i0 < e1; i0 += 64) {
                const int chunk = (e1 - i0) < 64 ? (e1 - i0) : 64;
                FuzzyDec d = {};
                int m = 0;
                float inv = 0.0f;
                if (lane < chunk) {
                    const int e = entEdge[i0 + lane];
                    m = e / K;
                    inv = 1.0f / (float)nnCount[(long long)b * M + m];
                    const long long ge = (long long)b * MK + e;
                    fuzzy_decode(filtIndex[ge], filtFrac[ge], n, p, q, F, d);
                }
                for (int j = 0; j < chunk; j += 4) {
                    float gv[4][CPT][2];
                    int mm[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        mm[u] = __builtin_amdgcn_readlane(m, (j + u) < chunk ? (j + u) : (chunk - 1));
                        fetch(mm[u], gv[u]);
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (j + u < chunk) {
                            fuzzy_take<true>(d, j + u, bin, coef);
                            edge(mm[u], readlane_f(inv, j + u), gv[u], bin, coef);
                        }
                    }
                }
            }
        } else {
            for (int i = e0; i < e1; i++) {
                const int e = entEdge[i];
                const int m = e / K;
                const long long ge = (long long)b * MK + e;
                fuzzy_corners(filtIndex[ge], filtFrac[ge], n, p, q, F, bin, coef);
                float gv[CPT][2];
                fetch(m, gv);
                edge(m, 1.0f / (float)nnCount[(long long)b * M + m], gv, bin, coef);
            }
        }
#pragma unroll
        for (int v = 0; v < CPT; v++) {
            if (live[v]) gradInput[(size_t)s * C + c_lo + c0 + v] = acc[v];
        }
    }
}

// ---- host-side launch shapes -----------------------------------------------------------------------------------------------------
// columns of a slice for a table of F rows: everything when it fits, else a multiple of 64 (of 4 when F leaves fewer than 64)
static inline int fuzzy_slice_cols(int F, int J)
{
    int js = (kFuzzyLdsWords / F) & ~3;
    js = js < kFuzzyMaxCols ? js : kFuzzyMaxCols;
    if (J <= js) return J;
    return js >= 64 ? js & ~63 : js;
}

static inline int fuzzy_parts(int B, int M, int F, int J)
{
    const long long rows = (long long)B * M;
    long long parts = (rows + 31) / 32;
    parts = parts < 1 ? 1 : parts;
    parts = parts < kFuzzyMaxParts ? parts : kFuzzyMaxParts;
    while (parts > 128 && parts * F * J * (long long)sizeof(float) > kFuzzyMaxPartBytes) parts >>= 1;
    return (int)parts;
}

// row blocks of a gather launch: every workgroup stages its slice's table (up to 64 KB) first, so a launch runs about 2048
// workgroups over all its slices, each looping over many rows, not one workgroup per few rows
static inline long long fuzzy_row_blocks(long long row_groups, int slices)
{
    long long cap = 2048 / slices;
    cap = cap < 64 ? 64 : cap;
    row_groups = row_groups < 1 ? 1 : row_groups;
    return row_groups < cap ? row_groups : cap;
}

static int fuzzy_conv_dims_ok(const char* who, int B, int N, int M, int F, int C, int r, int K, int n, int p, int q)
{
    SPH3D_REQUIRE(B >= 0 && N > 0 && M >= 0 && K > 0, "%s: bad dims B=%d N=%d M=%d K=%d", who, B, N, M, K);
    SPH3D_REQUIRE(C > 0 && r > 0, "%s: bad dims C=%d r=%d", who, C, r);
    SPH3D_REQUIRE(n > 2 && n % 2 == 0 && p > 0 && p % 2 == 0 && q > 0, "%s: kernel needs n>2 even, p>0 even, q>0, got [%d, %d, %d]", who,
                  n, p, q);
    SPH3D_REQUIRE((long long)n * p * q + 1 == F && F <= 257, "%s: the filter needs n*p*q + 1 = %lld <= 257 bins, got F=%d", who,
                  (long long)n * p * q + 1, F);
    SPH3D_REQUIRE((long long)C * r < (1LL << 24), "%s: C*r=%lld is too wide", who, (long long)C * r);
    SPH3D_REQUIRE((long long)F * ((r + 3) & ~3) <= kFuzzyLdsWords, "%s: F*r=%lld exceeds the %d table words of a workgroup", who,
                  (long long)F * r, kFuzzyLdsWords);
    SPH3D_REQUIRE((long long)B * M * K < (1LL << 31), "%s: B*M*K overflows int32", who);
    return SPH3D_OK;
}

// the instantiation for (CPT, W): KERNEL<1, false> below a wave per row, else KERNEL<CPT, true>
#define FUZZY_DISPATCH(KERNEL, CPT, W, ...)                                      \
    do {                                                                         \
        if ((W) < 64) hipLaunchKernelGGL((KERNEL<1, false>), __VA_ARGS__);       \
        else if ((CPT) == 1) hipLaunchKernelGGL((KERNEL<1, true>), __VA_ARGS__); \
        else if ((CPT) == 2) hipLaunchKernelGGL((KERNEL<2, true>), __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<4, true>), __VA_ARGS__);                 \
    } while (0)

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_fuzzy_spherical_kernel(int B, int N, int M, int K, int n, int p, int q, float radius,
                                            const float* database, const float* query,
                                            const int* nn_index, const int* nn_count, const float* nn_dist,
                                            int* filt_index, int* filt_frac, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(radius > 0, "Range search requires radius>0, got %g", (double)radius);
    SPH3D_REQUIRE(n > 2 && n % 2 == 0, "Need n_>2 and n_%%2==0, got %d", n);
    SPH3D_REQUIRE(p > 0 && p % 2 == 0, "Need p_>0 and p_%%2==0, got %d", p);
    SPH3D_REQUIRE(q > 0, "Need q_>0, got %d", q);
    SPH3D_REQUIRE((long long)n * p * q + 1 <= 257, "FuzzySphericalKernel: n*p*q + 1 = %lld bins exceed 257", (long long)n * p * q + 1);
    SPH3D_REQUIRE(B >= 0 && N > 0 && M >= 0 && K > 0, "FuzzySphericalKernel: bad dims B=%d N=%d M=%d K=%d", B, N, M, K);
    const long long total = (long long)B * M * K;
    if (total == 0) return SPH3D_OK;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(fuzzy_kernel_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                       B, N, M, K, n, p, q, radius, database, query, nn_index, nn_count, nn_dist, filt_index, filt_frac);
    return check_launch("sph3d_fuzzy_spherical_kernel");
}

extern "C" int sph3d_fuzzy_depthwise_conv3d(int B, int N, int M, int F, int C, int r, int K, int n, int p, int q,
                                            const int* nn_index, const int* nn_count, const int* filt_index, const int* filt_frac,
                                            const float* input, const float* filter, float* output, sph3d_stream_t stream)
{
    int rc = fuzzy_conv_dims_ok("fuzzy_depthwise_conv3d", B, N, M, F, C, r, K, n, p, q);
    if (rc || B == 0 || M == 0) return rc;
    const int J = C * r;
    const int JS = fuzzy_slice_cols(F, J);
    const int slices = (J + JS - 1) / JS;
    const int S4 = (JS + 3) / 4;                      // table row stride in units of four words
    int W, CPT;
    fuzzy_shape(JS, W, CPT);
    const int G = 256 / W;
    const long long gy = fuzzy_row_blocks(((long long)B * M + G - 1) / G, slices);
    const size_t lds = sizeof(float) * (size_t)F * S4 * 4;
    const dim3 grid((unsigned)slices, (unsigned)gy);
    FUZZY_DISPATCH(fuzzy_fwd_kernel, CPT, W, grid, dim3(256), lds, as_stream(stream), B, N, M, K, F, C, r, n, p, q, JS, S4, W, nn_index,
                   nn_count, filt_index, filt_frac, input, filter, output);
    return check_launch("sph3d_fuzzy_depthwise_conv3d");
}

// partial filter-gradient tables: fuzzy_parts(B, M, F, C * r) * F * C * r floats
extern "C" size_t sph3d_fuzzy_depthwise_conv3d_grad_workspace(int B, int N, int M, int F, int C, int r, int K)
{
    (void)N;
    (void)K;
    if (B <= 0 || M <= 0 || F <= 0 || C <= 0 || r <= 0) return 0;
    return sizeof(float) * (size_t)fuzzy_parts(B, M, F, C * r) * F * C * r;
}

extern "C" int sph3d_fuzzy_depthwise_conv3d_grad(int B, int N, int M, int F, int C, int r, int K, int n, int p, int q,
                                                 const int* nn_index, const int* nn_count, const int* filt_index,
                                                 const int* filt_frac, const int* offsets, const int* ent_edge,
                                                 const float* input, const float* filter, const float* grad_output,
                                                 float* grad_input, float* grad_filter,
                                                 void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    int rc = fuzzy_conv_dims_ok("fuzzy_depthwise_conv3d_grad", B, N, M, F, C, r, K, n, p, q);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const int J = C * r;
    if (B == 0 || M == 0) {          // no edges: both gradients are zero
        rc = zero_async(grad_filter, sizeof(float) * (size_t)F * J, st, "fuzzy_depthwise_conv3d_grad: memset");
        if (rc || B == 0) return rc;
        return zero_async(grad_input, sizeof(float) * (size_t)B * N * C, st, "fuzzy_depthwise_conv3d_grad: memset");
    }
    const size_t need = sph3d_fuzzy_depthwise_conv3d_grad_workspace(B, N, M, F, C, r, K);
    if (workspace == nullptr || workspace_bytes < need) {
        set_error("fuzzy_depthwise_conv3d_grad: workspace %zu B < required %zu B", workspace_bytes, need);
        return SPH3D_EWORKSPACE;
    }
    // grad_filter: per-workgroup tables over the forward graph, then the fixed-order reduce
    {
        const int JS = fuzzy_slice_cols(F, J);
        const int slices = (J + JS - 1) / JS;
        const int S4 = (JS + 3) / 4;
        // as many lanes per row as the slice has columns: a table serves W / 64 waves, and tables are what limits the waves of a CU
        const int CPT = JS <= 256 ? 1 : 2;
        int W = 1;
        while (W * CPT < JS) W <<= 1;
        int G = kFuzzyLdsWords / (F * S4 * 4);
        G = G < 256 / W ? G : 256 / W;
        G = G < 1 ? 1 : G;
        const int parts = fuzzy_parts(B, M, F, J);
        const size_t lds = sizeof(float) * (size_t)G * F * S4 * 4;
        const dim3 grid((unsigned)slices, (unsigned)parts);
        float* partial = (float*)workspace;
        FUZZY_DISPATCH(fuzzy_gf_kernel, CPT, W, grid, dim3(256), lds, st, B, N, M, K, F, C, r, n, p, q, JS, S4, W, G, nn_index, nn_count,
                       filt_index, filt_frac, input, grad_output, partial);
        const int total = F * J;
        hipLaunchKernelGGL(fuzzy_gf_reduce, dim3((total + 255) / 256), dim3(256), 0, st, total, parts, partial, grad_filter);
    }
    // grad_input: gather over the edge-id transposed graph
    {
        int CS = fuzzy_slice_cols(F, J) / r;         // channels of a slice: its table holds CS * r columns
        CS = CS < 1 ? 1 : (CS < C ? CS : C);
        const int slices = (C + CS - 1) / CS;
        const int S4 = (CS * r + 3) / 4;
        int W, CPT;
        fuzzy_shape(CS, W, CPT);
        const int G = 256 / W;
        const long long gy = fuzzy_row_blocks(((long long)B * N + G - 1) / G, slices);
        const size_t lds = sizeof(float) * (size_t)F * S4 * 4;
        const dim3 grid((unsigned)slices, (unsigned)gy);
        FUZZY_DISPATCH(fuzzy_gi_kernel, CPT, W, grid, dim3(256), lds, st, B, N, M, K, F, C, r, n, p, q, CS, S4, W, offsets, ent_edge,
                       nn_count, filt_index, filt_frac, filter, grad_output, grad_input);
    }
    return check_launch("sph3d_fuzzy_depthwise_conv3d_grad");
}
