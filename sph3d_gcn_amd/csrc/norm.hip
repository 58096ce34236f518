// norm.hip — fused ELU + batch-normalisation tail of the separable convolution, gfx950.
//
// The reference's separable_conv3d / pointwise_conv3d end with  matmul -> (bias) -> ELU -> batch_norm
// (utils/sph3gcn_util.py:152-161, 208-220; tf.nn.elu + tf.layers.batch_normalization(momentum 0.99, eps 1e-3), stock TF
// ops there).  As separate passes that tail moves the [R,C] activation through HBM five times forward (ELU r+w, stats r,
// normalise r+w) and eight times backward; it was 3.7 ms of a 20 ms step.  Fused:
//   forward : stats pass  reads y            -> per-channel sum / sum of squares of z = elu(y)   (partials, no atomics)
//             apply pass  reads y, writes out   out = (elu(y) - mean) * rstd * gamma + beta
//   backward: reduce pass reads y, dout      -> dbeta = sum dout, dgamma = sum dout * zhat
//             apply pass  reads y, dout, writes dy = gamma*rstd*(dout - dbeta/R - zhat*dgamma/R) * elu'(y)
// Only y (the GEMM output) is kept for the backward pass; z is recomputed (one v_exp per element).
// All kernels are HBM-streaming: float4 per lane, rows strided over the workgroup, per-workgroup partial sums reduced in
// double by a single small kernel (deterministic).  Requires C % 4 == 0 and C <= 1024 (the plans' 64..512).
#include "common.hpp"

namespace sph3d {

constexpr int kNormMaxBlocks = 1024;

// partial[blk][0][C] = sum a, partial[blk][1][C] = sum b over the block's rows, where
//   BWD = false: a = z,    b = z*z            (z = elu(y))
//   BWD = true : a = dout, b = dout * zhat    (zhat = (z - mean) * rstd)
template <bool BWD>
__global__ __launch_bounds__(256) void norm_reduce_kernel(int R, int C, const float* __restrict__ y,
                                                          const float* __restrict__ dout, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, float* __restrict__ partial)
{
    __shared__ float4 red[2][256];
    const int cg = C >> 2;                          // channel groups of 4
    const int rows_per_iter = 256 / cg > 0 ? 256 / cg : 1;
    const int tx = (int)threadIdx.x % cg, ty = (int)threadIdx.x / cg;
    const bool act = ty < rows_per_iter;
    const int rows_per_block = (R + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r0 = (int)blockIdx.x * rows_per_block;
    const int r1 = (r0 + rows_per_block) < R ? (r0 + rows_per_block) : R;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    float4 mu = a, rs = a;
    if (BWD && act) {
        mu = *reinterpret_cast<const float4*>(&mean[tx * 4]);
        rs = *reinterpret_cast<const float4*>(&rstd[tx * 4]);
    }
    if (act) {
        // four rows per trip, their loads issued together: with one row per trip the kernel ran at a third of the HBM
        // rate (one or two 16-B loads in flight per lane)
        constexpr int UN = 4;
        for (int rb = r0 + ty; rb < r1; rb += UN * rows_per_iter) {
            float4 v[UN], g[UN];
#pragma unroll
            for (int u = 0; u < UN; u++) {
                const int r = rb + u * rows_per_iter;
                const int rc = r < r1 ? r : rb;                      // clamped: re-reads the trip's first row
                v[u] = *reinterpret_cast<const float4*>(&y[(size_t)rc * C + tx * 4]);
                if (BWD) g[u] = *reinterpret_cast<const float4*>(&dout[(size_t)rc * C + tx * 4]);
            }
#pragma unroll
            for (int u = 0; u < UN; u++) {
                if (rb + u * rows_per_iter < r1) {
                    const float4 z = make_float4(elu1(v[u].x), elu1(v[u].y), elu1(v[u].z), elu1(v[u].w));
                    if (!BWD) {
                        a.x += z.x; a.y += z.y; a.z += z.z; a.w += z.w;
                        b.x = fmaf(z.x, z.x, b.x); b.y = fmaf(z.y, z.y, b.y); b.z = fmaf(z.z, z.z, b.z); b.w = fmaf(z.w, z.w, b.w);
                    } else {
                        a.x += g[u].x; a.y += g[u].y; a.z += g[u].z; a.w += g[u].w;
                        b.x = fmaf(g[u].x, (z.x - mu.x) * rs.x, b.x);
                        b.y = fmaf(g[u].y, (z.y - mu.y) * rs.y, b.y);
                        b.z = fmaf(g[u].z, (z.z - mu.z) * rs.z, b.z);
                        b.w = fmaf(g[u].w, (z.w - mu.w) * rs.w, b.w);
                    }
                }
            }
        }
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    if (ty == 0 && tx < cg) {                        // fold the ty rows of the workgroup, fixed order
        for (int j = 1; j < rows_per_iter; j++) {
            const float4 p = red[0][j * cg + tx], q = red[1][j * cg + tx];
            a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
            b.x += q.x; b.y += q.y; b.z += q.z; b.w += q.w;
        }
        float* out = partial + (size_t)blockIdx.x * 2 * C;
        *reinterpret_cast<float4*>(&out[tx * 4]) = a;
        *reinterpret_cast<float4*>(&out[C + tx * 4]) = b;
    }
}

// Sum the per-workgroup partials of 32 channels with 1024 threads (32 partial-lanes per channel, double precision, fixed
// order); the result is valid for threads with py == 0.  (A one-thread-per-channel loop over 1024 partials took 67 us,
// 8 partial-lanes per channel 12 us per finalize launch = 0.4 ms per step over the 34 launches.)
constexpr int kFinLanes = 32;
__device__ __forceinline__ void sum_partials_32x8(int C, int nblk, const float* __restrict__ partial, int c, int py,
                                                  double& s, double& q)
{
    __shared__ double red[2][kFinLanes][32];
    s = 0.0; q = 0.0;
    if (c < C) {
        // eight rows per trip, their sixteen loads issued together: one row per trip is a chain of up to 32 dependent
        // round trips to L2 (the finalize kernels measured 8.5 us each, 34 of them per step, for a few microseconds of work)
        constexpr int UN = 8;
        for (int k0 = py; k0 < nblk; k0 += kFinLanes * UN) {
            float a[UN], b[UN];
#pragma unroll
            for (int u = 0; u < UN; u++) {
                const int k = k0 + u * kFinLanes;
                const int kc = k < nblk ? k : py;                    // clamped (py < nblk here), masked below
                a[u] = partial[(size_t)kc * 2 * C + c];
                b[u] = partial[(size_t)kc * 2 * C + C + c];
            }
#pragma unroll
            for (int u = 0; u < UN; u++) {
                if (k0 + u * kFinLanes < nblk) { s += (double)a[u]; q += (double)b[u]; }
            }
        }
    }
    const int cx = (int)threadIdx.x & 31;
    red[0][py][cx] = s;
    red[1][py][cx] = q;
    __syncthreads();
    if (py == 0) {
        for (int j = 1; j < kFinLanes; j++) { s += red[0][j][cx]; q += red[1][j][cx]; }
    }
}

// ---- what follows the sums, stated once: the uncut finalize kernels and the kernels after the cut both call these -----------------
// forward: mean / rstd of channel c from s = sum z, q = sum z*z over R rows (double), running statistics update
// running = (1-m)*running + m*batch with the BIASED batch variance: tf.layers.batch_normalization on rank-2/3 inputs takes
// the non-fused path (tf.nn.moments), which stores the population variance — torch's F.batch_norm would store the
// Bessel-corrected one (3 % larger at the ModelNet fc layers, where R = batch size)
__device__ __forceinline__ void norm_fwd_stats(int c, double s, double q, double R, float eps, float momentum, float* mean, float* rstd,
                                               float* run_mean, float* run_var)
{
    const double m = s / R;
    double var = q / R - m * m;
    if (var < 0.0) var = 0.0;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean != nullptr) {
        run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * m);
        run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * var);
    }
}

// backward: the two per-channel means the apply pass needs, coef [2][C] = dbeta/R, dgamma/R from s = sum dout, q = sum dout * zhat
__device__ __forceinline__ void norm_bwd_coef(int c, int C, double s, double q, double R, int training, float* coef)
{
    coef[c] = training ? (float)(s / R) : 0.f;          // with fixed (running) statistics the two mean terms vanish
    coef[C + c] = training ? (float)(q / R) : 0.f;
}

// forward finalize: the statistics from the partials
__global__ __launch_bounds__(1024) void norm_fwd_finalize(int R, int C, int nblk, const float* __restrict__ partial, float eps, float momentum,
                                  float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ run_mean,
                                  float* __restrict__ run_var)
{
    const int c = blockIdx.x * 32 + ((int)threadIdx.x & 31);
    const int py = (int)threadIdx.x >> 5;
    double s, q;
    sum_partials_32x8(C, nblk, partial, c, py, s, q);
    if (c >= C || py != 0) return;
    norm_fwd_stats(c, s, q, (double)R, eps, momentum, mean, rstd, run_mean, run_var);
}

// inference: statistics come from the running buffers
__global__ void norm_eval_stats(int C, const float* __restrict__ run_mean, const float* __restrict__ run_var, float eps,
                                float* __restrict__ mean, float* __restrict__ rstd)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    mean[c] = run_mean[c];
    rstd[c] = (float)(1.0 / sqrt((double)run_var[c] + (double)eps));
}

// backward finalize: dgamma, dbeta and coef
__global__ __launch_bounds__(1024) void norm_bwd_finalize(int R, int C, int nblk, int training, const float* __restrict__ partial,
                                  float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef)
{
    const int c = blockIdx.x * 32 + ((int)threadIdx.x & 31);
    const int py = (int)threadIdx.x >> 5;
    double s, q;
    sum_partials_32x8(C, nblk, partial, c, py, s, q);
    if (c >= C || py != 0) return;
    dbeta[c] = (float)s;
    dgamma[c] = (float)q;
    norm_bwd_coef(c, C, s, q, (double)R, training, coef);
}

// ---- the same two finalizes cut at the statistics (batch norm over the rows of several ranks) ---------------
// A rank's per-channel sums leave in double, a collective the caller issues adds the other ranks' on top, and the statistics are
// formed from what comes back by the two functions above, with the row count a double read from the buffer: unchanged sums give
// bit-identical statistics.

// forward, before the cut: sums[0..C) = sum z, sums[C..2C) = sum z*z, sums[2C] = R
__global__ __launch_bounds__(1024) void norm_fwd_sums(int R, int C, int nblk, const float* __restrict__ partial,
                                                      double* __restrict__ sums)
{
    const int c = blockIdx.x * 32 + ((int)threadIdx.x & 31);
    const int py = (int)threadIdx.x >> 5;
    double s, q;
    sum_partials_32x8(C, nblk, partial, c, py, s, q);
    if (c >= C || py != 0) return;
    sums[c] = s;
    sums[C + c] = q;
    if (c == 0) sums[2 * C] = (double)R;
}

// forward, after the cut: the statistics from the summed buffer; the global row count stays on the device
__global__ __launch_bounds__(256) void norm_fwd_stats_from_sums(int C, const double* __restrict__ sums, float eps, float momentum,
                                                                float* __restrict__ mean, float* __restrict__ rstd,
                                                                float* __restrict__ run_mean, float* __restrict__ run_var,
                                                                double* __restrict__ count)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    norm_fwd_stats(c, sums[c], sums[C + c], sums[2 * C], eps, momentum, mean, rstd, run_mean, run_var);
    if (c == 0) count[0] = sums[2 * C];
}

// backward, before the cut: this rank's dgamma / dbeta (they stay local sums: the gradient all-reduce adds the ranks') and
// sums[0..C) = sum dout, sums[C..2C) = sum dout * zhat
__global__ __launch_bounds__(1024) void norm_bwd_sums(int C, int nblk, const float* __restrict__ partial, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, double* __restrict__ sums)
{
    const int c = blockIdx.x * 32 + ((int)threadIdx.x & 31);
    const int py = (int)threadIdx.x >> 5;
    double s, q;
    sum_partials_32x8(C, nblk, partial, c, py, s, q);
    if (c >= C || py != 0) return;
    dbeta[c] = (float)s;
    dgamma[c] = (float)q;
    sums[c] = s;
    sums[C + c] = q;
}

// backward, after the cut: coef over the global rows
__global__ __launch_bounds__(256) void norm_bwd_coef_from_sums(int C, const double* __restrict__ sums, const double* __restrict__ count,
                                                               float* __restrict__ coef)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) norm_bwd_coef(c, C, sums[c], sums[C + c], count[0], 1, coef);
}

// BWD = false: out = (elu(y) - mean) * rstd * gamma + beta
// BWD = true : dy  = gamma * rstd * (dout - c0 - zhat * c1) * elu'(y)
template <bool BWD>
__global__ __launch_bounds__(256) void norm_apply_kernel(long long total4, int C, const float* __restrict__ y,
                                                         const float* __restrict__ dout, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ coef,
                                                         float* __restrict__ out)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int cg = C >> 2;
    // channel group of element i, carried from iteration to iteration: a 64-bit `i % cg` per float4 is ~60 VALU
    // instructions, as much time as the HBM traffic of this streaming kernel
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int cq = (int)(i0 % cg);
    const int cstep = (int)(stride % cg);
    for (long long i = i0; i < total4; i += stride) {
        const int c = cq * 4;
        cq += cstep;
        cq = cq >= cg ? cq - cg : cq;
        const float4 v = reinterpret_cast<const float4*>(y)[i];
        const float4 mu = *reinterpret_cast<const float4*>(&mean[c]);
        const float4 rs = *reinterpret_cast<const float4*>(&rstd[c]);
        const float4 ga = *reinterpret_cast<const float4*>(&gamma[c]);
        float4 o;
        if (!BWD) {
            const float4 be = *reinterpret_cast<const float4*>(&beta[c]);
            o.x = fmaf((elu1(v.x) - mu.x) * rs.x, ga.x, be.x);
            o.y = fmaf((elu1(v.y) - mu.y) * rs.y, ga.y, be.y);
            o.z = fmaf((elu1(v.z) - mu.z) * rs.z, ga.z, be.z);
            o.w = fmaf((elu1(v.w) - mu.w) * rs.w, ga.w, be.w);
        } else {
            const float4 g = reinterpret_cast<const float4*>(dout)[i];
            const float4 c0 = *reinterpret_cast<const float4*>(&coef[c]);
            const float4 c1 = *reinterpret_cast<const float4*>(&coef[C + c]);
#define SPH3D_BN_BWD(e)                                                             \
    {                                                                               \
        const float z = elu1(v.e);                                                  \
        const float zh = (z - mu.e) * rs.e;                                         \
        const float dz = ga.e * rs.e * (g.e - c0.e - zh * c1.e);                    \
        o.e = v.e > 0.f ? dz : dz * (z + 1.f);                                      \
    }
            SPH3D_BN_BWD(x) SPH3D_BN_BWD(y) SPH3D_BN_BWD(z) SPH3D_BN_BWD(w)
#undef SPH3D_BN_BWD
        }
        reinterpret_cast<float4*>(out)[i] = o;
    }
}

// ---- the host side: one preamble, one launcher per stage, seven entries ------------------------------------------------------------
// The most rows an entry takes: the largest R at which every int expression of norm_reduce_kernel is exact.  Its largest values:
//   rows_per_block = (R + gridDim.x - 1) / gridDim.x    the numerator, gridDim.x <= kNormMaxBlocks = 1024:     at most R + 1023
//   r0 + rows_per_block <= gridDim.x * ceil(R / gridDim.x)                                                    at most R + 1023
//   rb += UN * rows_per_iter, from a row rb <= r1 - 1 <= R - 1, UN = 4, rows_per_iter = 256 / cg <= 256:      at most R + 1023
//   rb + u * rows_per_iter, u <= 3, lies below that.
// So R + 1023 <= INT_MAX.  (Everything past the row index is size_t or long long: (size_t)rc * C, total4.)
constexpr int kNormMaxRows = 0x7fffffff - 1023;

// one workgroup per ~32 rows (the small levels have only a few thousand rows: 128-row blocks left most CUs idle)
static int norm_blocks(int R)
{
    const long long b = ((long long)R + 31) / 32;
    return b < 1 ? 1 : (b > kNormMaxBlocks ? kNormMaxBlocks : (int)b);
}

struct NormWorkspace {                               // the workspace's layout: partial[nblk][2][C], then coef[2][C]
    int nblk;
    float *partial, *coef;
};

}  // namespace sph3d

using namespace sph3d;

extern "C" size_t sph3d_elu_bn_workspace(int R, int C)
{
    return sizeof(float) * ((size_t)norm_blocks(R) * 2 * C + 2 * (size_t)C);
}

// What every entry does first: the dimension check and, for an entry that needs the workspace (ws != NULL), the workspace check and
// the carve.  Nothing is read or launched before it answers.
static int norm_enter(const char* who, int R, int C, NormWorkspace* ws = nullptr, void* workspace = nullptr, size_t workspace_bytes = 0)
{
    SPH3D_REQUIRE(R > 0 && R <= kNormMaxRows && C > 0 && C % 4 == 0 && C <= 1024, "%s: needs 0<R<=%d, C%%4==0, C<=1024 (got R=%d C=%d)", who,
                  kNormMaxRows, R, C);
    if (ws == nullptr) return SPH3D_OK;
    const size_t need = sph3d_elu_bn_workspace(R, C);
    if (workspace == nullptr || workspace_bytes < need) {
        set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
        return SPH3D_EWORKSPACE;
    }
    ws->nblk = norm_blocks(R);
    ws->partial = (float*)workspace;
    ws->coef = ws->partial + (size_t)ws->nblk * 2 * C;
    return SPH3D_OK;
}

template <bool BWD>
static void launch_reduce(hipStream_t st, int R, int C, const NormWorkspace& ws, const float* y, const float* dout, const float* mean,
                          const float* rstd)
{
    hipLaunchKernelGGL(norm_reduce_kernel<BWD>, dim3(ws.nblk), dim3(256), 0, st, R, C, y, dout, mean, rstd, ws.partial);
}

// the finalize family: a kernel that sums the partials takes 32 channels x kFinLanes threads per workgroup, one that starts from
// per-channel values 256 channels
template <class... Params, class... Args>
static void launch_stats(void (*kern)(Params...), bool sums_partials, int C, hipStream_t st, Args... args)
{
    const int per = sums_partials ? 32 : 256;
    kern<<<dim3((C + per - 1) / per), dim3(sums_partials ? 32 * kFinLanes : 256), 0, st>>>(args...);
}

template <bool BWD>
static void launch_apply(hipStream_t st, int R, int C, const float* y, const float* dout, const float* mean, const float* rstd,
                         const float* gamma, const float* beta, const float* coef, float* out)
{
    const long long total4 = (long long)R * C / 4;
    const long long blocks = (total4 + 255) / 256;
    hipLaunchKernelGGL(norm_apply_kernel<BWD>, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, total4, C, y, dout, mean,
                       rstd, gamma, beta, coef, out);
}

// training-mode forward once the partials exist: finalize + apply
static void forward_from_partials(hipStream_t st, int R, int C, int nblk, const float* partial, const float* y, const float* gamma,
                                  const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* out,
                                  float* save_mean, float* save_rstd)
{
    launch_stats(norm_fwd_finalize, true, C, st, R, C, nblk, partial, eps, momentum, save_mean, save_rstd, running_mean, running_var);
    launch_apply<false>(st, R, C, y, nullptr, save_mean, save_rstd, gamma, beta, nullptr, out);
}

// training != 0: batch statistics (saved to save_mean / save_rstd for the backward pass), running stats updated.
// training == 0: normalise with running_mean / running_var (save_* receive the statistics used).
extern "C" int sph3d_elu_bn_forward(int R, int C, const float* y, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, float momentum, float eps, int training,
                                    float* out, float* save_mean, float* save_rstd,
                                    void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    NormWorkspace ws;
    if (int rc = norm_enter("sph3d_elu_bn_forward", R, C, &ws, workspace, workspace_bytes)) return rc;
    hipStream_t st = as_stream(stream);
    if (training) {
        launch_reduce<false>(st, R, C, ws, y, nullptr, nullptr, nullptr);
        forward_from_partials(st, R, C, ws.nblk, ws.partial, y, gamma, beta, running_mean, running_var, momentum, eps, out, save_mean,
                              save_rstd);
    } else {
        SPH3D_REQUIRE(running_mean != nullptr && running_var != nullptr, "sph3d_elu_bn_forward: inference needs running statistics");
        launch_stats(norm_eval_stats, false, C, st, C, running_mean, running_var, eps, save_mean, save_rstd);
        launch_apply<false>(st, R, C, y, nullptr, save_mean, save_rstd, gamma, beta, nullptr, out);
    }
    return check_launch("sph3d_elu_bn_forward");
}

// The same op when the statistics' partial sums already exist (sph3d_pointwise_gemm_bnstats wrote them from the GEMM's
// epilogue: partial[nblk][2][C] = per row block sum elu(y), sum elu(y)^2): finalize + apply only, training mode.
extern "C" int sph3d_elu_bn_forward_partials(int R, int C, int nblk, const float* partial, const float* y, const float* gamma,
                                             const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                             float* out, float* save_mean, float* save_rstd, sph3d_stream_t stream)
{
    if (int rc = norm_enter("sph3d_elu_bn_forward_partials", R, C)) return rc;
    SPH3D_REQUIRE(nblk > 0, "sph3d_elu_bn_forward_partials: nblk=%d partial row blocks", nblk);
    forward_from_partials(as_stream(stream), R, C, nblk, partial, y, gamma, beta, running_mean, running_var, momentum, eps, out, save_mean,
                          save_rstd);
    return check_launch("sph3d_elu_bn_forward_partials");
}

extern "C" int sph3d_elu_bn_backward(int R, int C, const float* y, const float* dout, const float* gamma,
                                     const float* save_mean, const float* save_rstd, int training,
                                     float* dy, float* dgamma, float* dbeta,
                                     void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    NormWorkspace ws;
    if (int rc = norm_enter("sph3d_elu_bn_backward", R, C, &ws, workspace, workspace_bytes)) return rc;
    hipStream_t st = as_stream(stream);
    launch_reduce<true>(st, R, C, ws, y, dout, save_mean, save_rstd);
    launch_stats(norm_bwd_finalize, true, C, st, R, C, ws.nblk, training, ws.partial, dgamma, dbeta, ws.coef);
    launch_apply<true>(st, R, C, y, dout, save_mean, save_rstd, gamma, nullptr, ws.coef, dy);
    return check_launch("sph3d_elu_bn_backward");
}

// ---- batch norm over several ranks' rows: the two ops above cut at the statistics (include/sph3d.h) -------------------------
// partial == NULL: the statistics pass over y runs here, into the workspace; else partial[nblk][2][C] as in
// sph3d_elu_bn_forward_partials (no workspace needed).  sums: double [2C + 1] = sum elu(y), sum elu(y)^2, R.
extern "C" int sph3d_elu_bn_forward_sums(int R, int C, int nblk, const float* partial, const float* y, double* sums,
                                         void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    NormWorkspace ws;
    if (int rc = norm_enter("sph3d_elu_bn_forward_sums", R, C, partial == nullptr ? &ws : nullptr, workspace, workspace_bytes)) return rc;
    SPH3D_REQUIRE(sums != nullptr, "sph3d_elu_bn_forward_sums: sums is NULL");
    hipStream_t st = as_stream(stream);
    if (partial == nullptr) {
        SPH3D_REQUIRE(y != nullptr, "sph3d_elu_bn_forward_sums: y is NULL");
        launch_reduce<false>(st, R, C, ws, y, nullptr, nullptr, nullptr);
        nblk = ws.nblk;
        partial = ws.partial;
    } else {
        SPH3D_REQUIRE(nblk > 0, "sph3d_elu_bn_forward_sums: nblk=%d partial row blocks", nblk);
    }
    launch_stats(norm_fwd_sums, true, C, st, R, C, nblk, partial, sums);
    return check_launch("sph3d_elu_bn_forward_sums");
}

// sums: the [2C + 1] buffer after the ranks' buffers were added up.  count [1] receives the global row count (a double on the
// device: sph3d_elu_bn_backward_apply reads it there).
extern "C" int sph3d_elu_bn_forward_apply(int R, int C, const double* sums, const float* y, const float* gamma, const float* beta,
                                          float* running_mean, float* running_var, float momentum, float eps,
                                          float* out, float* save_mean, float* save_rstd, double* count, sph3d_stream_t stream)
{
    if (int rc = norm_enter("sph3d_elu_bn_forward_apply", R, C)) return rc;
    SPH3D_REQUIRE(sums != nullptr && count != nullptr, "sph3d_elu_bn_forward_apply: sums / count is NULL");
    hipStream_t st = as_stream(stream);
    launch_stats(norm_fwd_stats_from_sums, false, C, st, C, sums, eps, momentum, save_mean, save_rstd, running_mean, running_var, count);
    launch_apply<false>(st, R, C, y, nullptr, save_mean, save_rstd, gamma, beta, nullptr, out);
    return check_launch("sph3d_elu_bn_forward_apply");
}

// dgamma / dbeta [C]: this rank's sums (fp32, as sph3d_elu_bn_backward writes them); sums: double [2C] = sum dout, sum dout*zhat.
extern "C" int sph3d_elu_bn_backward_sums(int R, int C, const float* y, const float* dout, const float* save_mean,
                                          const float* save_rstd, float* dgamma, float* dbeta, double* sums,
                                          void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    NormWorkspace ws;
    if (int rc = norm_enter("sph3d_elu_bn_backward_sums", R, C, &ws, workspace, workspace_bytes)) return rc;
    SPH3D_REQUIRE(sums != nullptr, "sph3d_elu_bn_backward_sums: sums is NULL");
    hipStream_t st = as_stream(stream);
    launch_reduce<true>(st, R, C, ws, y, dout, save_mean, save_rstd);
    launch_stats(norm_bwd_sums, true, C, st, C, ws.nblk, ws.partial, dgamma, dbeta, sums);
    return check_launch("sph3d_elu_bn_backward_sums");
}

// sums: the [2C] buffer after the ranks' buffers were added up; count: what sph3d_elu_bn_forward_apply wrote.
extern "C" int sph3d_elu_bn_backward_apply(int R, int C, const double* sums, const double* count, const float* y, const float* dout,
                                           const float* gamma, const float* save_mean, const float* save_rstd, float* dy,
                                           void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    NormWorkspace ws;
    if (int rc = norm_enter("sph3d_elu_bn_backward_apply", R, C, &ws, workspace, workspace_bytes)) return rc;
    SPH3D_REQUIRE(sums != nullptr && count != nullptr, "sph3d_elu_bn_backward_apply: sums / count is NULL");
    hipStream_t st = as_stream(stream);
    launch_stats(norm_bwd_coef_from_sums, false, C, st, C, sums, count, ws.coef);
    launch_apply<true>(st, R, C, y, dout, save_mean, save_rstd, gamma, nullptr, ws.coef, dy);
    return check_launch("sph3d_elu_bn_backward_apply");
}
