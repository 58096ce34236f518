// clseval.hip — the ModelNet40 classification evaluation on the device (modelnet40_cls/evaluate_modelnet.py:149-223): the whole-shape
// batch, the float64 vote sums and the per-class counters.  harness/clseval.py states all three in numpy; the integer outputs, the
// mask-0 coordinates and the float64 sums (ordered adds) equal that statement bit for bit.
//
//   clsfeed_assemble   objfeed.hip's batch with two more arguments.  order = 1: slot i reads row i of its shape, the stored order
//                      the reference evaluates in (FPS starts from row 0, so the graph depends on it); slots i >= n write zeros and
//                      index -1.  order = 0: the feed's draw (feed_sample_row).  swap_yz = 1 exchanges columns 1 and 2 of the row
//                      before any transform: `batch_xyz[:, :, [0, 2, 1]]` of evaluate_modelnet.py:173, train_modelnet.py:278,337.
//                      Recipe bits 1, 2, 4, 8 (TURN, TILT, SCALE, SHIFT) with objfeed.hip's purposes and counters; the kernel reads
//                      no other bit (the evaluation and the ModelNet training recipe have no jitter), and harness/clseval.py refuses
//                      a mask above 15 before it is uploaded.  A mask of 0 copies bit for bit.  No label output.
//                      Mapping as in objfeed.hip: grid (ceil(N / 256), B), one cloud per workgroup, the cloud's numbers wave-uniform.
//   cls_vote_accumulate  sums[b, c] = 0.0 + (double)logits[b, c] for vote 0 (np.zeros(...) += pred_val: a logit of -0.0 leaves
//                      +0.0), sums[b, c] += (double)logits[b, c] after it: one float64 add per vote in vote order,
//                      `batch_pred_sum += pred_val` of :180,196.  One thread per (b, c); no atomic.
//   cls_vote_finalize  one wave per cloud, one class per lane: a butterfly of (value, index) under numpy's arg-max rule (the first
//                      maximum; a NaN is a maximum), then lane 0 writes pred[shape id] and adds to the integer counters (:198-207).
// Every id and label is checked against its range before an address is formed.  No floating-point atomic, nothing allocated.
#include "feed_draws.hpp"

namespace sph3d {

enum : int { kClsTurn = 1, kClsTilt = 2, kClsScale = 4, kClsShift = 8 };

__global__ __launch_bounds__(256) void clsfeed_assemble_kernel(int N, int P, long long T, const float* __restrict__ rows,
                                                               const long long* __restrict__ offsets, const int* __restrict__ shape_ids,
                                                               unsigned long long seed, unsigned long long step,
                                                               const int* __restrict__ recipe, int order, int swap_yz,
                                                               float* __restrict__ points, int* __restrict__ index)
{
    const int b = blockIdx.y;                                          // (wave-uniform: one cloud per workgroup)
    const unsigned slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= (unsigned)N) return;
    const long long i = (long long)b * N + slot;
    float* out = points + i * 3;

    // the cloud's rows; a shape id or an offset pair that does not describe rows of the pool reads nothing (index -1, zeros), and
    // so does a slot past the last row of a shape that is read in stored order
    long long lo;
    const unsigned n = feed_pool_rows(shape_ids[b], P, T, offsets, lo);
    if (n == 0u || (order != 0 && slot >= n)) {
        out[0] = out[1] = out[2] = 0.f;
        if (index != nullptr) index[i] = -1;
        return;
    }
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    const int mask = uniform(recipe[b]);

    const unsigned r = order != 0 ? slot : feed_sample_row(ck, n, (unsigned)N, slot);
    const float4 a = *reinterpret_cast<const float4*>(rows + (lo + (long long)r) * 8);           // x y z (column 3 is not used)
    float x = a.x, y = swap_yz ? a.z : a.y, z = swap_yz ? a.y : a.z;

    // row vector times matrix, as utils/data_util.py writes it; the cloud's numbers are the same in every lane (objfeed.hip)
    if (mask & kClsTurn) {
        float st, ct;
        feed_turn(ck, st, ct);
        st = uniformf(st); ct = uniformf(ct);
        const float x1 = x * ct + y * st, y1 = y * ct - x * st;
        x = x1; y = y1;
    }
    if (mask & kClsTilt) {
        float m[9];
        feed_tilt(ck, m);
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = uniformf(m[k]);
        const float x1 = x * m[0] + y * m[3] + z * m[6];
        const float y1 = x * m[1] + y * m[4] + z * m[7];
        const float z1 = x * m[2] + y * m[5] + z * m[8];
        x = x1; y = y1; z = z1;
    }
    if (mask & kClsScale) {
        const float s = uniformf(0.8f + 0.45f * feed_uniform((unsigned)(feed_draw(ck, kFeedScale, 0u) >> 32)));
        x *= s; y *= s; z *= s;
    }
    if (mask & kClsShift) {
        x += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 0u) >> 32)));
        y += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 1u) >> 32)));
        z += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 2u) >> 32)));
    }
    out[0] = x; out[1] = y; out[2] = z;
    if (index != nullptr) index[i] = (int)r;
}

__global__ __launch_bounds__(256) void cls_vote_accumulate_kernel(int B, int C, const float* __restrict__ logits, int vote,
                                                                  int num_votes, double* __restrict__ sums,
                                                                  const int* __restrict__ shape_ids, float* __restrict__ votes_out,
                                                                  int P)
{
    const int k = blockIdx.x * 256 + threadIdx.x;                      // (B * C <= 65535 * 64 < 2^31)
    if (k >= B * C) return;
    const float l = logits[k];
    const double before = vote == 0 ? 0.0 : sums[k];
    sums[k] = before + (double)l;
    if (votes_out != nullptr) {
        const int b = k / C;
        const int id = shape_ids[b];
        if (id >= 0 && id < P) votes_out[((long long)id * num_votes + vote) * C + (k - b * C)] = l;
    }
}

// does (v, i) come before (w, j) in numpy's arg-max order: a NaN before every number, then the larger value, then the lower index
__device__ __forceinline__ bool cls_before(double v, int i, double w, int j)
{
    const bool vn = v != v, wn = w != w;
    if (vn != wn) return vn;
    if (!vn && v != w) return v > w;
    return i < j;
}

__global__ __launch_bounds__(256) void cls_vote_finalize_kernel(int B, int C, const double* __restrict__ sums,
                                                                const int* __restrict__ shape_ids, const int* __restrict__ category,
                                                                int P, int* __restrict__ pred, int* __restrict__ counters,
                                                                int* __restrict__ class_seen, int* __restrict__ class_correct)
{
    const int b = uniform((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));       // one wave per cloud
    if (b >= B) return;                                                        // (the whole wave leaves)
    const int lane = lane_id();
    const bool mine = lane < C;
    // a lane without a class holds (-inf, 64 + lane): it comes after every class, a class of -inf included
    double v = mine ? sums[(long long)b * C + lane] : -__builtin_inf();
    int arg = mine ? lane : 64 + lane;
    const bool bad = __any(mine && !(fabs(v) <= 1.7976931348623157e308));       // a NaN or an infinity among the C sums
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double w = __shfl_xor(v, d, 64);
        const int j = __shfl_xor(arg, d, 64);
        if (cls_before(w, j, v, arg)) {
            v = w;
            arg = j;
        }
    }
    if (lane != 0) return;
    const int id = shape_ids[b];
    if (id < 0 || id >= P) return;                                             // a shape outside the pool counts nothing
    pred[id] = arg;
    const int label = category[id];
    if (label < 0 || label >= C) {
        atomicAdd(&counters[3], 1);
        return;
    }
    atomicAdd(&counters[0], 1);
    atomicAdd(&class_seen[label], 1);
    if (bad) atomicAdd(&counters[2], 1);
    if (arg == label) {
        atomicAdd(&counters[1], 1);
        atomicAdd(&class_correct[label], 1);
    }
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_clsfeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows,
                                      const long long* offsets, const int* shape_ids, unsigned long long seed,
                                      unsigned long long step, const int* recipe, int order, int swap_yz, float* points, int* index,
                                      sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "clsfeed_assemble: batch 0<B<=65535 required, got %d", B);
    SPH3D_REQUIRE(num_point > 0, "clsfeed_assemble: num_point>0 required, got %d", num_point);
    SPH3D_REQUIRE(num_blocks > 0 && total_rows > 0, "clsfeed_assemble: empty pool (num_blocks=%d total_rows=%lld)", num_blocks,
                  total_rows);
    SPH3D_REQUIRE((order == 0 || order == 1) && (swap_yz == 0 || swap_yz == 1),
                  "clsfeed_assemble: order and swap_yz are 0 or 1, got %d and %d", order, swap_yz);
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && shape_ids != nullptr && recipe != nullptr,
                  "clsfeed_assemble: null input pointer");
    SPH3D_REQUIRE(points != nullptr, "clsfeed_assemble: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rows) & 15) == 0, "clsfeed_assemble: rows must be 16-byte aligned");
    const long long total = (long long)B * num_point;
    SPH3D_REQUIRE(total <= 0x7fffffffll, "clsfeed_assemble: B*num_point=%lld too large", total);
    hipLaunchKernelGGL(clsfeed_assemble_kernel, dim3((unsigned)((num_point + 255) / 256), (unsigned)B), dim3(256), 0, as_stream(stream),
                       num_point, num_blocks, total_rows, rows, offsets, shape_ids, seed, step, recipe, order, swap_yz, points, index);
    return check_launch("sph3d_clsfeed_assemble");
}

extern "C" int sph3d_cls_vote_accumulate(int B, int C, const float* logits, int vote, int num_votes, double* sums,
                                         const int* shape_ids, float* votes_out, int num_blocks, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "cls_vote_accumulate: batch 0<B<=65535 required, got %d", B);
    SPH3D_REQUIRE(C > 0 && C <= kVoteMaxClasses, "cls_vote_accumulate: 0<C<=%d classes required, got %d", kVoteMaxClasses, C);
    SPH3D_REQUIRE(num_votes > 0 && vote >= 0 && vote < num_votes, "cls_vote_accumulate: vote %d is not one of %d", vote, num_votes);
    SPH3D_REQUIRE(logits != nullptr && sums != nullptr, "cls_vote_accumulate: null logits or sums");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(sums) & 7) == 0, "cls_vote_accumulate: sums must be 8-byte aligned");
    SPH3D_REQUIRE(votes_out == nullptr || (shape_ids != nullptr && num_blocks > 0),
                  "cls_vote_accumulate: votes_out needs shape_ids and the pool's size");
    hipLaunchKernelGGL(cls_vote_accumulate_kernel, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, as_stream(stream), B, C, logits,
                       vote, num_votes, sums, shape_ids, votes_out, num_blocks);
    return check_launch("sph3d_cls_vote_accumulate");
}

extern "C" int sph3d_cls_vote_finalize(int B, int C, const double* sums, const int* shape_ids, const int* category, int num_blocks,
                                       int* pred, int* counters, int* class_seen, int* class_correct, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "cls_vote_finalize: batch 0<B<=65535 required, got %d", B);
    SPH3D_REQUIRE(C > 0 && C <= kVoteMaxClasses, "cls_vote_finalize: 0<C<=%d classes required, got %d", kVoteMaxClasses, C);
    SPH3D_REQUIRE(num_blocks > 0, "cls_vote_finalize: empty pool (num_blocks=%d)", num_blocks);
    SPH3D_REQUIRE(sums != nullptr && shape_ids != nullptr && category != nullptr, "cls_vote_finalize: null input pointer");
    SPH3D_REQUIRE(pred != nullptr && counters != nullptr && class_seen != nullptr && class_correct != nullptr,
                  "cls_vote_finalize: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(sums) & 7) == 0, "cls_vote_finalize: sums must be 8-byte aligned");
    hipLaunchKernelGGL(cls_vote_finalize_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, as_stream(stream), B, C, sums, shape_ids,
                       category, num_blocks, pred, counters, class_seen, class_correct);
    return check_launch("sph3d_cls_vote_finalize");
}
