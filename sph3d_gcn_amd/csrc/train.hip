// train.hip — the two kernels of the training loop that are not the model's: the reference's optimiser update and its per-step metrics.
//
// sph3d_train_update: the update of train_s3dis.py:223-226 over the harness's flat fp32 buffers, in TensorFlow 1's arithmetic
// (optim.hip's adam_kernel is torch.optim.Adam's: the two differ by sqrt(1 - b2^step) on eps, a factor 0.03 at step 1).  ONE
// streaming pass like adam_kernel — 16-byte lanes where every pointer is 16-byte aligned, scalar lanes otherwise and for the tail;
// 28 B per parameter for Adam, 20 B for momentum.  With g = grad_scale * grad:
//     rule 0, tf.train.AdamOptimizer (training_ops.cc ApplyAdam, use_nesterov = false):
//         m += (1 - b1) (g - m);   v += (1 - b2) (g g - v);   p -= (lr_t m) / (sqrt(v) + eps),   lr_t = lr sqrt(1 - b2^step) / (1 - b1^step)
//     rule 1, tf.train.MomentumOptimizer(use_nesterov=True) (ApplyMomentum):
//         a = momentum a + g;   p -= g lr + (a momentum) lr
// every operation rounded once (-ffp-contract=off), sqrt and the division correctly rounded.  Elements whose g is not finite are
// updated like any other (the reference lets a NaN propagate) and counted: per wave one popcount of a ballot per lane component
// and at most one integer atomic, issued only when the wave's count is not zero.
//
// sph3d_train_update_guarded, sph3d_guard_restore: the same update behind a decision taken on the device — clip by the global norm,
// skip a step whose gradient is not finite, keep an averaged copy of the weights (stated where the kernels stand, below).
//
// sph3d_train_metrics: train_s3dis.py:371-376 and :461-474 without the copy of the logits to the host: arg-max per row, the
// confusion matrix of the counted rows and five counters, all accumulated.  A workgroup counts its rows into an LDS histogram
// (C * C <= 4096 words) and ballots, and adds only the non-zero words to the global ones: a 16 x 8192 x 13 batch issues at most
// 64 x 169 integer atomics instead of 131 072.  The loss shares of the step are added to one double by one thread in index order.
#include "common.hpp"

namespace sph3d {

constexpr int kRuleAdam = 0, kRuleNesterov = 1;

template <int RULE>
__global__ __launch_bounds__(256) void train_update_kernel(long long n4, long long n, float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ s0, float* __restrict__ s1, float lr, float b1,
                                                           float b2, float eps, float grad_scale,
                                                           unsigned long long* __restrict__ nonfinite)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const float c1 = 1.f - b1, c2 = 1.f - b2;
    auto upd = [&](float& pp, float raw, float& a, float& b) -> bool {
        const float gg = grad_scale * raw;
        if (RULE == kRuleAdam) {
            a = a + c1 * (gg - a);
            b = b + c2 * (gg * gg - b);
            pp = pp - (lr * a) / (sqrtf(b) + eps);
        } else {
            a = b1 * a + gg;                          // (b1 carries the momentum)
            pp = pp - (gg * lr + (a * b1) * lr);
        }
        return !isfinite(gg);
    };
    bool bad[4] = {false, false, false, false};
    if (i < n4) {
        float4 P = reinterpret_cast<float4*>(p)[i], A = reinterpret_cast<float4*>(s0)[i];
        float4 B = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RULE == kRuleAdam) B = reinterpret_cast<float4*>(s1)[i];
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        bad[0] = upd(P.x, G.x, A.x, B.x); bad[1] = upd(P.y, G.y, A.y, B.y);
        bad[2] = upd(P.z, G.z, A.z, B.z); bad[3] = upd(P.w, G.w, A.w, B.w);
        reinterpret_cast<float4*>(p)[i] = P; reinterpret_cast<float4*>(s0)[i] = A;
        if (RULE == kRuleAdam) reinterpret_cast<float4*>(s1)[i] = B;
    } else {
        const long long e = n4 * 4 + (i - n4);          // scalar lanes: the tail, or everything when a pointer is not 16-byte aligned
        if (e < n) {
            float P = p[e], A = s0[e], B = 0.f;
            if (RULE == kRuleAdam) B = s1[e];
            bad[0] = upd(P, g[e], A, B);
            p[e] = P; s0[e] = A;
            if (RULE == kRuleAdam) s1[e] = B;
        }
    }
    if (nonfinite != nullptr) {                          // (wave-uniform)
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt += __popcll(__ballot(bad[k]));
        if (cnt != 0 && lane_id() == 0) atomicAdd(nonfinite, (unsigned long long)cnt);
    }
}

// ---- the guarded update (harness/guard.py is the statement; the state's words are laid out in include/sph3d.h) -----------------
// Three launches, no workgroup waits for another, no floating-point atomic: (a) grad_sumsq_kernel leaves one float64 partial sum
// and one count of non-finite elements per workgroup, (b) guard_finalize_kernel reduces them in the statement's order, decides and
// writes the step's scalars into the state, (c) train_update_guarded_kernel reads them there and returns before any store when
// the step is skipped.  The sum of squares is the statement's fixed tree: lane l of 2^18 adds the squares (exact in float64) of
// the elements i = l (mod 2^18) in ascending i, and the lanes are reduced by adjacent pairs: thread t of workgroup w holds the
// lanes 1024 w + 4 t .. + 3, so the tree's levels are the thread's two pair sums, the wave's six-step xor butterfly (lane bit by
// lane bit: both lanes of a pair form the same sum), the four waves as (w0 + w1) + (w2 + w3), and the 256 partials once more.
constexpr int kGuardBlocks = 256, kGuardThreads = 256;
constexpr long long kGuardLanes = 4ll * kGuardBlocks * kGuardThreads;          // 2^18
enum { kGS = 0, kGBad, kGApplied, kGSkipped, kGClipped, kGB1Pow, kGB2Pow, kGLastNorm, kGMaxNorm, kGLrT, kGC32, kGOm, kGFlag };
static_assert(kGFlag < SPH3D_GUARD_STATE_WORDS, "the guard's state has SPH3D_GUARD_STATE_WORDS words");

// the levels of the tree inside one workgroup of 256 threads; the result is thread 0's
__device__ __forceinline__ double guard_block_sum(double x, double* lds)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + __shfl_xor(x, m);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(kGuardThreads) void grad_sumsq_kernel(long long n, const float* __restrict__ g, int vec, float grad_scale,
                                                                   double* __restrict__ part, unsigned long long* __restrict__ badpart)
{
    __shared__ double lds[4];
    __shared__ unsigned badcnt;
    if (threadIdx.x == 0) badcnt = 0u;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    unsigned bad = 0u;
    auto add = [&](double& a, float raw) {
        const float gg = grad_scale * raw;                       // the element the update forms
        const double d = (double)gg;
        a = a + d * d;                                           // (the square is exact; -ffp-contract=off: no fma)
        bad += isfinite(gg) ? 0u : 1u;
    };
    long long base = 4ll * ((long long)blockIdx.x * kGuardThreads + threadIdx.x);
    if (vec) {
#pragma unroll 4
        for (; base + 3 < n; base += kGuardLanes) {
            const float4 G = *reinterpret_cast<const float4*>(g + base);
            add(a0, G.x); add(a1, G.y); add(a2, G.z); add(a3, G.w);
        }
    }
    for (; base < n; base += kGuardLanes) {                      // scalar loads, the same lanes: the tail, or everything
        add(a0, g[base]);
        if (base + 1 < n) add(a1, g[base + 1]);
        if (base + 2 < n) add(a2, g[base + 2]);
        if (base + 3 < n) add(a3, g[base + 3]);
    }
    __syncthreads();                                             // (badcnt is zero)
    const double s = guard_block_sum((a0 + a1) + (a2 + a3), lds);
    if (bad) atomicAdd(&badcnt, bad);                            // (an integer in LDS)
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        badpart[blockIdx.x] = (unsigned long long)badcnt;
    }
}

__global__ __launch_bounds__(kGuardThreads) void guard_finalize_kernel(const double* __restrict__ part,
                                                                       const unsigned long long* __restrict__ badpart, int rule, float lr,
                                                                       float b1, float b2, float clip_norm, int skip_nonfinite, int has_ema,
                                                                       float ema_decay, unsigned long long* __restrict__ state,
                                                                       unsigned long long* __restrict__ nonfinite)
{
    __shared__ double lds[4];
    __shared__ unsigned long long badsum;
    if (threadIdx.x == 0) badsum = 0ull;
    __syncthreads();
    const double S = guard_block_sum(part[threadIdx.x], lds);
    const unsigned long long b = badpart[threadIdx.x];
    if (b) atomicAdd(&badsum, b);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* f = reinterpret_cast<double*>(state);
    const unsigned long long bad = badsum;
    f[kGS] = S;
    state[kGBad] = bad;
    if (nonfinite != nullptr && bad) atomicAdd(nonfinite, bad);
    if (skip_nonfinite && bad) {                                 // nothing else changes
        state[kGSkipped] += 1ull;
        state[kGFlag] = 0ull;
        return;
    }
    const double norm = sqrt(S);
    bool clipped = false;
    float c32 = 1.f;
    if (clip_norm > 0.f && bad == 0ull) {
        const double c = (double)clip_norm / (norm + 1e-6);
        clipped = c < 1.0;
        c32 = (float)c;
    }
    const unsigned long long before = state[kGApplied];
    state[kGApplied] = before + 1ull;
    float lr_t = lr;
    if (rule == kRuleAdam) {
        const double p1 = f[kGB1Pow] * (double)b1, p2 = f[kGB2Pow] * (double)b2;
        f[kGB1Pow] = p1;
        f[kGB2Pow] = p2;
        lr_t = (float)((double)lr * sqrt(1.0 - p2) / (1.0 - p1));
    }
    float om = 0.f;
    if (has_ema) {
        const double a = (double)before, warm = (1.0 + a) / (10.0 + a), d = (double)ema_decay;
        om = (float)(1.0 - (d < warm ? d : warm));
    }
    if (clipped) state[kGClipped] += 1ull;
    f[kGLastNorm] = norm;
    if (norm > f[kGMaxNorm]) f[kGMaxNorm] = norm;                // (a NaN norm never replaces the maximum)
    f[kGLrT] = (double)lr_t;
    f[kGC32] = (double)c32;
    f[kGOm] = (double)om;
    state[kGFlag] = clipped ? 3ull : 1ull;
}

// train_update_kernel's two lane forms; 28 B per parameter for Adam, 36 B with the EMA
template <int RULE, bool EMA>
__global__ __launch_bounds__(256) void train_update_guarded_kernel(long long n4, long long n, float* __restrict__ p,
                                                                   const float* __restrict__ g, float* __restrict__ s0,
                                                                   float* __restrict__ s1, float* __restrict__ ema, float b1, float b2,
                                                                   float eps, float grad_scale,
                                                                   const unsigned long long* __restrict__ state)
{
    const unsigned long long flag = state[kGFlag];
    if (flag == 0ull) return;                                    // a skipped step: no store
    const double* f = reinterpret_cast<const double*>(state);
    const float lr = (float)f[kGLrT], c32 = (float)f[kGC32], om = (float)f[kGOm];      // (fp32 values kept in 8-byte words)
    const bool clip = (flag & 2ull) != 0ull;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const float c1 = 1.f - b1, c2 = 1.f - b2;
    auto upd = [&](float& pp, float raw, float& a, float& b, float& ev) {
        float gg = grad_scale * raw;
        if (clip) gg = c32 * gg;
        if (RULE == kRuleAdam) {
            a = a + c1 * (gg - a);
            b = b + c2 * (gg * gg - b);
            pp = pp - (lr * a) / (sqrtf(b) + eps);
        } else {
            a = b1 * a + gg;
            pp = pp - (gg * lr + (a * b1) * lr);
        }
        if (EMA) ev = ev - (ev - pp) * om;
    };
    if (i < n4) {
        float4 P = reinterpret_cast<float4*>(p)[i], A = reinterpret_cast<float4*>(s0)[i];
        float4 B = make_float4(0.f, 0.f, 0.f, 0.f), E = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RULE == kRuleAdam) B = reinterpret_cast<float4*>(s1)[i];
        if (EMA) E = reinterpret_cast<float4*>(ema)[i];
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        upd(P.x, G.x, A.x, B.x, E.x); upd(P.y, G.y, A.y, B.y, E.y);
        upd(P.z, G.z, A.z, B.z, E.z); upd(P.w, G.w, A.w, B.w, E.w);
        reinterpret_cast<float4*>(p)[i] = P; reinterpret_cast<float4*>(s0)[i] = A;
        if (RULE == kRuleAdam) reinterpret_cast<float4*>(s1)[i] = B;
        if (EMA) reinterpret_cast<float4*>(ema)[i] = E;
    } else {
        const long long e = n4 * 4 + (i - n4);
        if (e < n) {
            float P = p[e], A = s0[e], B = 0.f, E = 0.f;
            if (RULE == kRuleAdam) B = s1[e];
            if (EMA) E = ema[e];
            upd(P, g[e], A, B, E);
            p[e] = P; s0[e] = A;
            if (RULE == kRuleAdam) s1[e] = B;
            if (EMA) ema[e] = E;
        }
    }
}

__global__ __launch_bounds__(256) void guard_restore_kernel(long long n4, long long n, float* __restrict__ dst,
                                                            const float* __restrict__ src, const unsigned long long* __restrict__ state)
{
    if (state[kGFlag] != 0ull) return;                           // the last decision was to apply: nothing is written
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) {
        reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        const long long e = n4 * 4 + (i - n4);
        if (e < n) dst[e] = src[e];
    }
}

constexpr int kMetricsBlock = 256;
constexpr int kMetricsMaxBlocks = 64;

__global__ __launch_bounds__(kMetricsBlock) void train_metrics_kernel(long long R, int C, const float* __restrict__ logits,
                                                                      const int* __restrict__ label, const int* __restrict__ inner,
                                                                      const float* __restrict__ loss_part, int loss_parts,
                                                                      unsigned long long* __restrict__ confusion,
                                                                      unsigned long long* __restrict__ counters,
                                                                      double* __restrict__ loss_sum)
{
    __shared__ unsigned hist[kVoteMaxClasses * kVoteMaxClasses];
    __shared__ unsigned cnt[4];
    const int CC = C * C;
    for (int k = threadIdx.x; k < CC; k += kMetricsBlock) hist[k] = 0u;
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0u;
    __syncthreads();
    // every thread of a wave makes the same number of trips: the ballots below see whole waves
    const long long stride = (long long)gridDim.x * kMetricsBlock;
    const long long trips = (R + stride - 1) / stride;
    long long r = (long long)blockIdx.x * kMetricsBlock + threadIdx.x;
    for (long long t = 0; t < trips; ++t, r += stride) {
        bool seen = false, correct = false, badl = false, nonfin = false;
        if (r < R && (inner == nullptr || inner[r] > 0)) {
            const int l = label[r];
            if (l < 0 || l >= C) {
                badl = true;
            } else {
                bool finite;
                const int pred = vote_argmax(logits + r * C, 0, C, C, finite);
                seen = true;
                correct = pred == l;
                nonfin = !finite;
                atomicAdd(&hist[l * C + pred], 1u);
            }
        }
        const int s = __popcll(__ballot(seen)), c = __popcll(__ballot(correct)), b = __popcll(__ballot(badl)),
                  f = __popcll(__ballot(nonfin));
        if (lane_id() == 0) {
            if (s) atomicAdd(&cnt[0], (unsigned)s);
            if (c) atomicAdd(&cnt[1], (unsigned)c);
            if (b) atomicAdd(&cnt[2], (unsigned)b);
            if (f) atomicAdd(&cnt[3], (unsigned)f);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < CC; k += kMetricsBlock) {
        const unsigned h = hist[k];
        if (h) atomicAdd(&confusion[k], (unsigned long long)h);
    }
    if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&counters[4], 1ull);
        if (loss_part != nullptr && loss_sum != nullptr) {
            // calls on one stream are ordered and only this thread touches the word: a plain read-modify-write, in index order
            double acc = loss_sum[0];
            for (int k = 0; k < loss_parts; ++k) acc += (double)loss_part[k];
            loss_sum[0] = acc;
        }
    }
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_train_update(long long n, float* param, const float* grad, float* slot0, float* slot1, int rule, float lr,
                                  float beta1_or_momentum, float beta2, float eps, int step, float grad_scale, long long* nonfinite,
                                  sph3d_stream_t stream)
{
    SPH3D_REQUIRE(rule == kRuleAdam || rule == kRuleNesterov, "train_update: rule 0 (Adam) or 1 (Nesterov momentum) required, got %d", rule);
    SPH3D_REQUIRE(n >= 0 && step >= 1, "train_update: bad n=%lld step=%d", n, step);
    if (n == 0) return SPH3D_OK;
    SPH3D_REQUIRE(param != nullptr && grad != nullptr && slot0 != nullptr && (rule == kRuleNesterov || slot1 != nullptr),
                  "train_update: null buffer");
    const size_t bits = reinterpret_cast<size_t>(param) | reinterpret_cast<size_t>(grad) | reinterpret_cast<size_t>(slot0) |
                        (rule == kRuleAdam ? reinterpret_cast<size_t>(slot1) : 0);
    const long long n4 = (bits & 15) == 0 ? n / 4 : 0;
    const long long threads = n4 + (n - n4 * 4);
    SPH3D_REQUIRE((threads + 255) / 256 <= 0x7fffffffll, "train_update: n=%lld is more than one launch covers", n);
    const dim3 grid((unsigned)((threads + 255) / 256));
    unsigned long long* nf = reinterpret_cast<unsigned long long*>(nonfinite);
    if (rule == kRuleAdam) {
        const double b1 = (double)beta1_or_momentum, b2 = (double)beta2;
        const float lr_t = (float)((double)lr * sqrt(1.0 - pow(b2, (double)step)) / (1.0 - pow(b1, (double)step)));
        hipLaunchKernelGGL(train_update_kernel<kRuleAdam>, grid, dim3(256), 0, as_stream(stream), n4, n, param, grad, slot0, slot1, lr_t,
                           beta1_or_momentum, beta2, eps, grad_scale, nf);
    } else {
        hipLaunchKernelGGL(train_update_kernel<kRuleNesterov>, grid, dim3(256), 0, as_stream(stream), n4, n, param, grad, slot0, slot1,
                           lr, beta1_or_momentum, 0.f, 0.f, grad_scale, nf);
    }
    return check_launch("sph3d_train_update");
}

extern "C" size_t sph3d_train_guard_workspace(long long n)
{
    (void)n;                                                     // one float64 and one count per workgroup, whatever n is
    return (size_t)kGuardBlocks * (sizeof(double) + sizeof(unsigned long long));
}

extern "C" int sph3d_train_update_guarded(long long n, float* param, const float* grad, float* slot0, float* slot1, float* ema, int rule,
                                          float lr, float beta1_or_momentum, float beta2, float eps, float grad_scale, float clip_norm,
                                          int skip_nonfinite, float ema_decay, long long* state, long long* nonfinite, void* workspace,
                                          size_t workspace_bytes, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(rule == kRuleAdam || rule == kRuleNesterov, "train_update_guarded: rule 0 (Adam) or 1 (Nesterov momentum) required, got %d", rule);
    SPH3D_REQUIRE(n >= 0, "train_update_guarded: bad n=%lld", n);
    SPH3D_REQUIRE(ema == nullptr || (ema_decay > 0.f && ema_decay < 1.f), "train_update_guarded: 0 < ema_decay < 1 required, got %g",
                  (double)ema_decay);
    SPH3D_REQUIRE(!(clip_norm != clip_norm), "train_update_guarded: clip_norm is NaN");
    if (n == 0) return SPH3D_OK;
    SPH3D_REQUIRE(param != nullptr && grad != nullptr && slot0 != nullptr && (rule == kRuleNesterov || slot1 != nullptr) && state != nullptr,
                  "train_update_guarded: null buffer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(state) & 7) == 0, "train_update_guarded: state must be 8-byte aligned");
    if (workspace == nullptr || workspace_bytes < sph3d_train_guard_workspace(n) || (reinterpret_cast<size_t>(workspace) & 7) != 0) {
        set_error("train_update_guarded: workspace of %zu bytes, 8-byte aligned, required (got %zu)", sph3d_train_guard_workspace(n),
                  workspace == nullptr ? (size_t)0 : workspace_bytes);
        return SPH3D_EWORKSPACE;
    }
    const size_t bits = reinterpret_cast<size_t>(param) | reinterpret_cast<size_t>(grad) | reinterpret_cast<size_t>(slot0) |
                        (rule == kRuleAdam ? reinterpret_cast<size_t>(slot1) : 0) | reinterpret_cast<size_t>(ema);
    const long long n4 = (bits & 15) == 0 ? n / 4 : 0;
    const long long threads = n4 + (n - n4 * 4);
    SPH3D_REQUIRE((threads + 255) / 256 <= 0x7fffffffll, "train_update_guarded: n=%lld is more than one launch covers", n);
    const dim3 grid((unsigned)((threads + 255) / 256));
    hipStream_t st = as_stream(stream);
    double* part = static_cast<double*>(workspace);
    unsigned long long* badpart = reinterpret_cast<unsigned long long*>(part + kGuardBlocks);
    unsigned long long* sw = reinterpret_cast<unsigned long long*>(state);
    const int vec = (reinterpret_cast<size_t>(grad) & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(kGuardBlocks), dim3(kGuardThreads), 0, st, n, grad, vec, grad_scale, part, badpart);
    hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(kGuardThreads), 0, st, part, badpart, rule, lr, beta1_or_momentum, beta2,
                       clip_norm, skip_nonfinite, ema != nullptr ? 1 : 0, ema_decay, sw, reinterpret_cast<unsigned long long*>(nonfinite));
    const float b2 = rule == kRuleAdam ? beta2 : 0.f, ep = rule == kRuleAdam ? eps : 0.f;
#define SPH3D_GUARDED(RULE, EMA)                                                                                                      \
    hipLaunchKernelGGL((train_update_guarded_kernel<RULE, EMA>), grid, dim3(256), 0, st, n4, n, param, grad, slot0, slot1, ema,       \
                       beta1_or_momentum, b2, ep, grad_scale, sw)
    if (rule == kRuleAdam) {
        if (ema != nullptr) SPH3D_GUARDED(kRuleAdam, true); else SPH3D_GUARDED(kRuleAdam, false);
    } else {
        if (ema != nullptr) SPH3D_GUARDED(kRuleNesterov, true); else SPH3D_GUARDED(kRuleNesterov, false);
    }
#undef SPH3D_GUARDED
    return check_launch("sph3d_train_update_guarded");
}

extern "C" int sph3d_guard_restore(long long n, float* dst, const float* src, const long long* state, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(n >= 0, "guard_restore: bad n=%lld", n);
    if (n == 0) return SPH3D_OK;
    SPH3D_REQUIRE(dst != nullptr && src != nullptr && state != nullptr, "guard_restore: null buffer");
    const size_t bits = reinterpret_cast<size_t>(dst) | reinterpret_cast<size_t>(src);
    const long long n4 = (bits & 15) == 0 ? n / 4 : 0;
    const long long threads = n4 + (n - n4 * 4);
    SPH3D_REQUIRE((threads + 255) / 256 <= 0x7fffffffll, "guard_restore: n=%lld is more than one launch covers", n);
    hipLaunchKernelGGL(guard_restore_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream), n4, n, dst, src,
                       reinterpret_cast<const unsigned long long*>(state));
    return check_launch("sph3d_guard_restore");
}

extern "C" int sph3d_train_metrics(int B, int N, int C, const float* logits, const int* label, const int* inner,
                                   const float* loss_part, int loss_parts, long long* confusion, long long* counters,
                                   double* loss_sum, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && N > 0 && C > 0, "train_metrics: B, N, C > 0 required, got %d %d %d", B, N, C);
    if (C > kVoteMaxClasses) {
        set_error("train_metrics: C=%d classes, at most %d are supported", C, kVoteMaxClasses);
        return SPH3D_EUNSUPPORTED;
    }
    SPH3D_REQUIRE(logits != nullptr && label != nullptr && confusion != nullptr && counters != nullptr, "train_metrics: null buffer");
    SPH3D_REQUIRE(loss_part == nullptr || (loss_parts >= 0 && loss_sum != nullptr),
                  "train_metrics: loss_part needs loss_parts >= 0 and loss_sum");
    const long long R = (long long)B * N;
    long long blocks = (R + kMetricsBlock - 1) / kMetricsBlock;
    if (blocks > kMetricsMaxBlocks) blocks = kMetricsMaxBlocks;
    hipLaunchKernelGGL(train_metrics_kernel, dim3((unsigned)blocks), dim3(kMetricsBlock), 0, as_stream(stream), R, C, logits, label,
                       inner, loss_part, loss_parts, reinterpret_cast<unsigned long long*>(confusion),
                       reinterpret_cast<unsigned long long*>(counters), loss_sum);
    return check_launch("sph3d_train_metrics");
}
