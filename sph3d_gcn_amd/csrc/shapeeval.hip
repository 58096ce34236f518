// shapeeval.hip — the per-shape end of the ShapeNet part-segmentation evaluation on the device (shapenet_seg/evaluate_shapenet.py:
// 262-289 and evaluate_shapenet_onehot.py:283-314): arg-max of the vote sums inside the shape's own part range and the integer
// counts from which the host forms the part IoUs in float64.  It takes the place of vote.hip's finalize for a pool of shapes: the
// votes are the ones sph3d_vote_begin / sph3d_vote_accumulate left (rows [T,8] with the part label in column 6, votes indexed by
// pool row - row_base).  harness/shapeeval.py:shape_vote_reference states it in numpy; every output equals that statement.
//
//   per row      pred = part_lo[b] + first maximum of votes[row, part_lo[b] : part_lo[b] + part_n[b]] (a NaN counts as a maximum,
//                as np.argmax and vote.hip take it)
//   per shape    for the parts l of its range: inter[b, l] = rows with pred == l and gt == l, pred_cnt[b, l] = rows with pred == l,
//                gt_cnt[b, l] = rows with gt == l; correct[b] = rows with pred == gt.  A ground-truth label outside the range
//                matches no part.
// Mapping: grid (kShapeParts, B), a workgroup strides over the rows of ONE shape (so the shape's row range and part range are
// wave-uniform) with a thread per row, counts into 3 C + 2 LDS counters and flushes the non-zero ones with integer atomics.  Every
// address is checked against the pool and the batch's row range before it is formed (vote_cloud); a shape that does not fit, or
// whose part range is not inside [0, C), counts nothing and writes no prediction.  No floating-point atomic, nothing allocated.
#include "common.hpp"

namespace sph3d {

constexpr int kShapeParts = 8;                  // workgroups per shape (a ShapeNet shape has 2 000 - 3 000 rows)

__global__ __launch_bounds__(256) void shape_iou_kernel(int C, int P, long long T, const float* __restrict__ rows,
                                                        const long long* __restrict__ offsets, const int* __restrict__ shape_ids,
                                                        long long row_base, long long batch_rows, const float* __restrict__ votes,
                                                        const int* __restrict__ part_lo, const int* __restrict__ part_n,
                                                        int* __restrict__ pred, int* __restrict__ inter, int* __restrict__ pred_cnt,
                                                        int* __restrict__ gt_cnt, int* __restrict__ correct,
                                                        unsigned long long* __restrict__ nonfinite)
{
    __shared__ unsigned hist[3 * kVoteMaxClasses + 2];          // inter | pred_cnt | gt_cnt | correct, non-finite rows
    for (int k = threadIdx.x; k < 3 * kVoteMaxClasses + 2; k += 256) hist[k] = 0u;
    __syncthreads();
    const int b = blockIdx.y;
    long long lo;
    long long n = vote_cloud(b, P, T, offsets, shape_ids, row_base, batch_rows, lo);
    const int plo = part_lo[b], pn = part_n[b];
    if (plo < 0 || pn <= 0 || plo > C - pn) n = 0;               // (no range of the C sums: the shape takes no part)
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long long)gridDim.x * 256) {
        const long long row = lo - row_base + r;
        const float* v = votes + row * C;
        bool finite;
        const int arg = vote_argmax(v, plo, pn, C, finite);
        pred[row] = arg;
        if (!finite) atomicAdd(&hist[3 * kVoteMaxClasses + 1], 1u);
        const float lab = rows[(lo + r) * 8 + 6];
        atomicAdd(&hist[kVoteMaxClasses + arg], 1u);
        if (lab >= (float)plo && lab < (float)(plo + pn) && lab == (float)(int)lab)
            atomicAdd(&hist[2 * kVoteMaxClasses + (int)lab], 1u);
        if (lab == (float)arg) {
            atomicAdd(&hist[arg], 1u);
            atomicAdd(&hist[3 * kVoteMaxClasses], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * C; k += 256) {
        const int which = k / C, l = k - which * C;
        const unsigned h = hist[which * kVoteMaxClasses + l];
        if (h != 0u) atomicAdd((which == 0 ? inter : which == 1 ? pred_cnt : gt_cnt) + (long long)b * C + l, (int)h);
    }
    if (threadIdx.x == 0) {
        if (hist[3 * kVoteMaxClasses] != 0u) atomicAdd(&correct[b], (int)hist[3 * kVoteMaxClasses]);
        if (hist[3 * kVoteMaxClasses + 1] != 0u) atomicAdd(nonfinite, (unsigned long long)hist[3 * kVoteMaxClasses + 1]);
    }
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_shape_iou(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                               const int* shape_ids, long long row_base, long long batch_rows, const float* votes,
                               const int* part_lo, const int* part_n, int* pred, int* inter, int* pred_cnt, int* gt_cnt,
                               int* correct, long long* nonfinite, sph3d_stream_t stream)
{
    if (int rc = vote_check_args("shape_iou", B, C, num_blocks, total_rows, row_base, batch_rows)) return rc;
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && shape_ids != nullptr && votes != nullptr && part_lo != nullptr &&
                      part_n != nullptr,
                  "shape_iou: null input pointer");
    SPH3D_REQUIRE(pred != nullptr && inter != nullptr && pred_cnt != nullptr && gt_cnt != nullptr && correct != nullptr &&
                      nonfinite != nullptr,
                  "shape_iou: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(nonfinite) & 7) == 0, "shape_iou: nonfinite must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const size_t counts = (size_t)B * C * sizeof(int);
    if (int rc = zero_async(inter, counts, s, "shape_iou: inter")) return rc;
    if (int rc = zero_async(pred_cnt, counts, s, "shape_iou: pred_cnt")) return rc;
    if (int rc = zero_async(gt_cnt, counts, s, "shape_iou: gt_cnt")) return rc;
    if (int rc = zero_async(correct, (size_t)B * sizeof(int), s, "shape_iou: correct")) return rc;
    hipLaunchKernelGGL(shape_iou_kernel, dim3(kShapeParts, (unsigned)B), dim3(256), 0, s, C, num_blocks, total_rows, rows, offsets,
                       shape_ids, row_base, batch_rows, votes, part_lo, part_n, pred, inter, pred_cnt, gt_cnt, correct,
                       reinterpret_cast<unsigned long long*>(nonfinite));
    return check_launch("sph3d_shape_iou");
}
