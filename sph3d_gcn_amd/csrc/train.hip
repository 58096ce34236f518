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
