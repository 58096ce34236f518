// sepconv.hpp — what the three one-kernel separable layers share (sepring.hip: sepconv_ring_kernel, inference and training;
// sepconv.hip: sepconv_fused_kernel, sepconv_general_kernel): the host's launch choice, stated once (sep_plan; reported by
// sph3d_separable_conv3d_plan), and the device code all of them run, force-inlined into each kernel.
#pragma once
#include <stddef.h>
#include <string.h>
#include <type_traits>
#include "common.hpp"

namespace sph3d {

typedef float sep_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSepWaves = 16;               // waves of a workgroup, one workgroup per CU
constexpr int kSepGrid = 256;
constexpr int kSrRows = 16;                 // ring: points per row block (one MFMA row block)
constexpr int kScTile = 32;                 // small kernel: output points per tile (two per wave in the gather phase)
constexpr size_t kSepLds = 160 * 1024;

// ---- the plan: everything the host decides about a launch ------------------------------------------------------------------------
enum { kSepNone = 0, kSepRing = 1, kSepSmall = 2, kSepGeneral = 3 };

struct SepPlan {
    int kernel;                     // kSepNone: the shape is not covered
    int R, LPE, KT;                 // the instantiation: depth multiplier, lanes per edge (16: C <= 64, 32), padded C r / 16 (ring, small)
    int RBK, rbk_by_points;         // general: row blocks per tile, and what the point count alone asks for (before the LDS step-down)
    int NB, G;                      // ring: slots, wave groups
    int lds, grid;                  // dynamic LDS bytes; workgroups (0: nothing is launched)
    int stats_blocks;               // training: rows of the partial statistics
    int train;                      // (not reported) the ring kernel's TRAIN
};

static inline int sep_check_dims(const char* who, int B, int N, int M, int F, int C, int K, int Cout)
{
    SPH3D_REQUIRE(B >= 0 && N > 0 && M >= 0 && F > 0 && C > 0 && K > 0 && Cout > 0, "%s: bad dims B=%d N=%d M=%d F=%d C=%d K=%d Cout=%d", who, B, N,
                  M, F, C, K, Cout);
    return SPH3D_OK;
}

// train: sph3d_separable_conv3d_train (the ring kernel or nothing; B == 0 or M == 0 still launch: the all-zero partial rows the
// statistics finalize reads), else sph3d_separable_conv3d_fused (the ring kernel wherever it covers the shape, else the small
// kernel, else the general one).  32-bit byte offsets into a cloud's input and 24-bit neighbour ids bound N; a bin id is a byte
static inline SepPlan sep_plan(bool train, int B, int N, int M, int F, int C, int r, int K, int Cout)
{
    SepPlan p = {};
    p.train = train;
    if (!((r == 1 || r == 2) && C % 4 == 0 && C >= 4 && F <= 254 && N <= (1 << 24) && K > 0 &&
          (unsigned long long)N * C * 4ull + 1024ull < (1ull << 32)))
        return p;
    const int lpe = C <= 64 ? 16 : 32;
    const size_t filt = sizeof(float) * (size_t)(F + 1) * 4 * lpe * r;          // the filter table (general: a slice) and its zero row
    const bool cout16 = Cout % 16 == 0 && Cout >= 16;
    // ring and small: the pointwise weights' columns stay in a wave's registers
    int KT = 0, NB = 0;
    size_t ring_block = 0, small_lds = 0;
    bool ring = false, small = false;
    if (C <= 128 && C * r <= 256) {
        const int kt = (C * r + 15) / 16;
        KT = kt <= 4 ? 4 : (kt <= 8 ? 8 : 16);
        const size_t row = sizeof(float) * (KT * 16 + 4);                       // a row of the ring / of the A tile
        // ring depth: as many 16-point row blocks as fit beside the filter table, at most 8, at least 3
        ring_block = kSrRows * row;
        const size_t fixed = filt + 256;
        NB = fixed + 3 * ring_block > kSepLds ? 0 : (int)((kSepLds - fixed) / ring_block);
        NB = NB > 8 ? 8 : NB;
        // Cout: the column-block owners must divide the 16 waves
        ring = NB >= 3 && cout16 && Cout <= 256 && (Cout & (Cout - 1)) == 0;
        small_lds = filt + 2 * kScTile * row;                                   // the A tile is double buffered
        small = small_lds <= kSepLds && cout16 && Cout <= 128;
    }
    // general: C <= 128 (one, possibly partial, slice) or a multiple of 128; the smallest tile (one row block) must fit beside the
    // filter slice
    auto general_lds = [&](int rbk) { return filt + sizeof(float) * (size_t)(16 * rbk) * (4 * lpe * r + 4); };
    const bool general = general_lds(1) <= kSepLds && (C <= 128 || (C % 128 == 0 && C <= 4096)) && cout16 && Cout <= 512;
    if (train ? !ring : (!small && !general)) return p;
    p.R = r;
    p.LPE = lpe;
    p.grid = (train || (B > 0 && M > 0)) ? kSepGrid : 0;
    if (ring) {
        p.kernel = kSepRing;
        p.KT = KT;
        p.NB = NB;
        p.G = kSepWaves / (Cout >> 4);
        p.lds = (int)(filt + NB * ring_block + sizeof(int) * (2 + 2 * NB));
        p.stats_blocks = train ? kSepGrid * p.G : 0;
    } else if (small) {
        p.kernel = kSepSmall;
        p.KT = KT;
        p.lds = (int)small_lds;
    } else {
        p.kernel = kSepGeneral;
        // tile height: as many row blocks as still leave every CU a tile; many bins: a lower tile beside the larger filter slice
        const long long pts = (long long)B * M;
        p.RBK = p.rbk_by_points = pts >= 64LL * 512 ? 4 : (pts >= 32LL * 256 ? 2 : 1);
        while (p.RBK > 1 && general_lds(p.RBK) > kSepLds) p.RBK >>= 1;
        p.lds = (int)general_lds(p.RBK);
    }
    return p;
}

// ---- the launcher (sepconv.hip): the kernel a plan names; only the instantiations some plan reaches are compiled -----------------
struct SepArgs {
    int B, N, M, F, C, K, Cout, act;
    const int *nn_index, *nn_count, *bin_index;
    const float *input, *dw_filter, *W, *bias, *scale, *shift;
    float *output, *dw_out, *stats;                 // dw_out, stats: training
};
int sep_launch(const SepPlan& p, const SepArgs& a, hipStream_t st);

// the five (R, LPE, KT) some (C, r) yields, for the ring and the small kernel: LPE follows C, KT follows C r.  -> f(R, LPE, KT) as
// integral constants, nullptr for any other triple
template <class Fn>
static inline auto sep_with_triple(const SepPlan& p, Fn f) -> decltype(f(std::integral_constant<int, 1>{}, std::integral_constant<int, 16>{},
                                                                         std::integral_constant<int, 4>{}))
{
    using std::integral_constant;
    const int R = p.R, L = p.LPE, KT = p.KT;
    if (R == 1 && L == 16 && KT == 4) return f(integral_constant<int, 1>{}, integral_constant<int, 16>{}, integral_constant<int, 4>{});
    if (R == 2 && L == 16 && KT == 4) return f(integral_constant<int, 2>{}, integral_constant<int, 16>{}, integral_constant<int, 4>{});
    if (R == 2 && L == 16 && KT == 8) return f(integral_constant<int, 2>{}, integral_constant<int, 16>{}, integral_constant<int, 8>{});
    if (R == 1 && L == 32 && KT == 8) return f(integral_constant<int, 1>{}, integral_constant<int, 32>{}, integral_constant<int, 8>{});
    if (R == 2 && L == 32 && KT == 16) return f(integral_constant<int, 2>{}, integral_constant<int, 32>{}, integral_constant<int, 16>{});
    return nullptr;
}

typedef void (*SepRingKernel)(int, int, int, int, int, int, int, int, int, const int*, const int*, const int*, const float*, const float*,
                              const float*, const float*, const float*, const float*, float*, float*, float*);
SepRingKernel sepring_kernel(const SepPlan& p);     // sepring.hip

// ---- device code ---------------------------------------------------------------------------------------------------------------------
// The units of this workgroup — 16-point row blocks (ring) or tiles (small, general), per_cloud of them in a cloud: a contiguous range
// [begin, end) of the units of its XCD's clouds (B % 8 == 0; unit j is in cloud xcd + 8 (j / per_cloud)) or of all clouds'
__device__ __forceinline__ void sep_units(int B, int per_cloud, bool& affine, int& xcd, int& begin, int& end)
{
    const int WPX = (int)gridDim.x >> 3;
    const int wi = (int)blockIdx.x >> 3;
    xcd = (int)blockIdx.x & 7;
    affine = (B & 7) == 0;
    long long total, part, parts;
    if (affine) { total = (long long)(B >> 3) * per_cloud; part = wi; parts = WPX; }
    else { total = (long long)B * per_cloud; part = (long long)xcd * WPX + wi; parts = 8LL * WPX; }
    begin = (int)(total * part / parts), end = (int)(total * (part + 1) / parts);
}

// depthwise filter table -> LDS (dwconv_fwd_multi's layout [F + 1][R][SLI]), zero row F for padding slots
template <int R, int SLI>
__device__ __forceinline__ void sep_load_filter(float* lfilt, const float* dwFilter, int F, int CR, int tid)
{
    for (int e = tid * 4; e < F * CR; e += kSepWaves * 64 * 4) {
        const int f = e / CR;
        const int cl = e - f * CR;
        const int l4 = cl / (4 * R), q = (cl >> 2) % R;
        *reinterpret_cast<float4*>(&lfilt[f * (SLI * R) + q * SLI + l4 * 4]) = *reinterpret_cast<const float4*>(&dwFilter[(size_t)f * CR + cl]);
    }
    for (int e = tid; e < SLI * R; e += kSepWaves * 64) lfilt[F * (SLI * R) + e] = 0.f;
}

// The depthwise sums of one output point, gathered by one wave exactly like dwconv_fwd_multi (conv3d.hip): 64 neighbour ids and bins
// per trip, handed over packed (id | bin << 24; slots past cnt name the zero filter row F), 64 / LPE edges at a time, four loads in
// flight, R filter rows per edge.  lane, g = lane / LPE: as the kernel holds them (handed in: with g derived here the __shfl index
// becomes four induction variables, 4 VGPRs more in the R = 1 kernels); inb: the cloud's input; live: the point exists (m < M);
// row: its row of nnCount / nnIndex / binIndex; lfb: the filter table in LDS; rowb = 4 C; xoff, foff: this lane's byte offset in
// an input row and in a filter row (they differ in the general kernel: the slice's).
// -> v[4 R], folded over the wave's edge groups and NOT yet divided by cnt; the division, the LDS row and everything after it (the
// ring: the `filled` counter, then the HBM store) stay with the caller, in its order
template <int R>
struct SepSums {
    float v[4 * R];
    int cnt;
};
template <int R, int LPE>
__device__ __forceinline__ SepSums<R> sep_gather(int lane, int g, const char* inb, bool live, size_t row, int K, int F, const int* nnCount,
                                                 const int* nnIndex, const int* binIndex, const char* lfb, unsigned rowb, unsigned xoff,
                                                 unsigned foff)
{
    constexpr int EPL = 64 / LPE;
    constexpr int NO = 4 * R;
    constexpr int SLI = 4 * LPE;
    constexpr int FSTB = SLI * R * 4;            // bytes per filter row in LDS
    float acc[NO];                               // (copied out at the end: accumulating in the result costs the R = 1 kernels 4 VGPRs)
#pragma unroll
    for (int v = 0; v < NO; v++) acc[v] = 0.f;
    const int cnt = live ? uniform(nnCount[row]) : 0;
    for (int kt = 0; kt < cnt; kt += 64) {
        const int myk = kt + lane;
        const int kn = (cnt - kt) < 64 ? (cnt - kt) : 64;
        const int mykc = myk < cnt ? myk : kt;
        const int idxv = nnIndex[row * K + mykc];
        int binv = binIndex[row * K + mykc];
        binv = binv < 0 ? 0 : (binv >= F ? F - 1 : binv);
        binv = myk < cnt ? binv : F;
        const unsigned pk = ((unsigned)idxv & 0xffffffu) | ((unsigned)binv << 24);
        for (int k0 = 0; k0 < kn; k0 += 4 * EPL) {
            float4 x[4];
            unsigned fo[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int kq2 = k0 + u * EPL + g;
                const unsigned pp = (unsigned)__shfl((int)pk, kq2);
                const unsigned off = __umul24(pp, rowb) + xoff;
                fo[u] = __umul24(pp >> 24, (unsigned)FSTB) + foff;
                x[u] = *reinterpret_cast<const float4*>(inb + off);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float xs[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                for (int q = 0; q < R; q++) {
                    const float4 w4 = *reinterpret_cast<const float4*>(lfb + fo[u] + q * (SLI * 4));
                    acc[4 * q + 0] = fmaf(xs[(4 * q + 0) / R], w4.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = fmaf(xs[(4 * q + 1) / R], w4.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(xs[(4 * q + 2) / R], w4.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(xs[(4 * q + 3) / R], w4.w, acc[4 * q + 3]);
                }
            }
        }
    }
#pragma unroll
    for (int o = LPE; o < 64; o <<= 1)
#pragma unroll
        for (int v = 0; v < NO; v++) acc[v] += __shfl_xor(acc[v], o);
    SepSums<R> s;
#pragma unroll
    for (int v = 0; v < NO; v++) s.v[v] = acc[v];
    s.cnt = cnt;
    return s;
}

// ring, small: the 16 columns of column block cb of W in a wave's registers for the whole launch (C r x 16 floats = 64 VGPRs at
// C r = 256).  k-order of the product: lane (i = lane % 16, kq = lane / 16) supplies A[i][16t + 4kq + u] and B[16t + 4kq + u][j] at step (t, u): any
// pairing is legal as long as A and B use the same one, and this one makes a lane's four A values of a t ONE ds_read_b128
template <int KT>
__device__ __forceinline__ void sep_load_w(float (&wreg)[KT][4], const float* W, int CR, int Cout, int cb, int i16, int kq, bool gemm_wave)
{
#pragma unroll
    for (int t = 0; t < KT; t++)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = 16 * t + 4 * kq + u;
            wreg[t][u] = (gemm_wave && k < CR) ? W[(size_t)k * Cout + cb * 16 + i16] : 0.f;
        }
}

// one 16 x 16 block of the product: the row block at arow (this lane's row i, k offset 4 kq) with wreg.  Four independent
// accumulation chains (one per k-slot of the 16-byte read), added by the caller: one chain of 4 KT dependent MFMAs leaves the wave
// waiting for its own previous result (skinny.hip: 46 -> 33 us from the same change)
struct SepChains {
    sep_f32x4 d0, d1, d2, d3;
};
template <int KT>
__device__ __forceinline__ SepChains sep_product(const float* arow, const float (&wreg)[KT][4])
{
    sep_f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0, d2 = d0, d3 = d0;
#pragma unroll
    for (int t = 0; t < KT; t++) {
        const sep_f32x4 a = *reinterpret_cast<const sep_f32x4*>(arow + 16 * t);
        d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wreg[t][0], d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wreg[t][1], d1, 0, 0, 0);
        d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wreg[t][2], d2, 0, 0, 0);
        d3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wreg[t][3], d3, 0, 0, 0);
    }
    return {d0, d1, d2, d3};
}

}  // namespace sph3d
