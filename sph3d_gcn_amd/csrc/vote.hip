// vote.hip — the overlap-voting evaluation of the segmentation nets on the device (s3dis_seg/evaluate_s3dis_with_overlap.py:253-286
// the per-pass bookkeeping, :301-302 the vote, :314-325 arg-max and the per-class counts; its ScanNet twin differs in the coverage
// threshold only).  harness/evalvote.py:vote_reference states the same in numpy; every output here equals that statement bit for
// bit, the fp32 vote sums included: a row receives at most ONE fp32 add per pass and passes are ordered on the stream, so no sum
// depends on thread order.  No floating-point atomic anywhere; the integer ones are exact.
//
// A batch is b blocks of the pool; its rows are the range [row_base, row_base + batch_rows) of the pool's rows, and votes / count /
// pred / the stamps are indexed by (pool row - row_base).  Every kernel checks a block id, its offsets and the drawn row against
// the pool AND against that range before it forms an address: a cloud that does not fit votes nothing.
//
//   the duplicate rule   numpy's `a[idx] += v` with a repeated index keeps the LAST occurrence only, so slot j of a cloud votes iff
//                        no later slot of the same cloud drew the same row.  Phase 1 raises a 64-bit stamp (pass + 1) << 32 | slot
//                        per drawn row with an integer atomicMax; phase 2 lets the slot vote whose stamp stands.  The pass number
//                        in the high word makes stamps of earlier passes lose without a reset in between.
//   coverage             the winning slot's class-0 thread counts the row; an inner row whose count reaches min_votes adds one to
//                        its cloud's `covered`.  `remaining` = clouds with covered < inner_size, written by a one-wave kernel.
//   finalize             first-maximum arg-max per row as np.argmax (a NaN is a maximum), confusion[label, pred] of the inner rows
//                        through a per-workgroup LDS histogram flushed with 64-bit integer atomics.
// Traffic per pass at 16 x 8192 x 13: 6.8 MB of logits read coalesced (one thread per element), 2 x 6.8 MB of scattered 52-byte
// read-modify-writes on votes: microseconds; nothing here is tuned beyond that mapping.
#include "common.hpp"

namespace sph3d {

constexpr int kVoteFinalizeParts = 64;          // workgroups per cloud in the row-strided kernels

// inner_size[b] = rows of cloud b with inner == 1 (column 7 of the pool's rows)
__global__ __launch_bounds__(256) void vote_inner_size_kernel(int P, long long T, const float* __restrict__ rows,
                                                              const long long* __restrict__ offsets, const int* __restrict__ block_ids,
                                                              long long row_base, long long batch_rows, int* __restrict__ inner_size)
{
    const int b = blockIdx.y;
    long long lo;
    const long long n = vote_cloud(b, P, T, offsets, block_ids, row_base, batch_rows, lo);
    int mine = 0;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long long)gridDim.x * 256)
        mine += rows[(lo + r) * 8 + 7] == 1.0f ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if (lane_id() == 0 && mine != 0) atomicAdd(&inner_size[b], mine);
}

__global__ __launch_bounds__(64) void vote_remaining_kernel(int B, const int* __restrict__ covered, const int* __restrict__ inner_size,
                                                            int* __restrict__ remaining)
{
    int mine = 0;
    for (int b = threadIdx.x; b < B; b += 64) mine += covered[b] < inner_size[b] ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if (threadIdx.x == 0) remaining[0] = mine;
}

// phase 1: one thread per slot raises the stamp of the row it drew
__global__ __launch_bounds__(256) void vote_stamp_kernel(int B, int N, int P, long long T, const long long* __restrict__ offsets,
                                                         const int* __restrict__ block_ids, long long row_base, long long batch_rows,
                                                         unsigned pass, const int* __restrict__ index,
                                                         unsigned long long* __restrict__ stamp)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * N) return;
    const int b = (int)(i / N);
    const unsigned slot = (unsigned)(i - (long long)b * N);
    const int r = index[i];
    long long lo;
    const long long n = vote_cloud(b, P, T, offsets, block_ids, row_base, batch_rows, lo);
    if (r < 0 || r >= n) return;
    atomicMax(&stamp[lo - row_base + r], ((unsigned long long)(pass + 1u) << 32) | slot);
}

// phase 2: one thread per logit; the slot whose stamp stands adds its logits to the row's sums and counts the row
__global__ __launch_bounds__(256) void vote_add_kernel(int B, int N, int C, int P, long long T, const float* __restrict__ rows,
                                                       const long long* __restrict__ offsets, const int* __restrict__ block_ids,
                                                       long long row_base, long long batch_rows, unsigned pass,
                                                       const int* __restrict__ index, const float* __restrict__ logits, int min_votes,
                                                       const unsigned long long* __restrict__ stamp, float* __restrict__ votes,
                                                       int* __restrict__ count, int* __restrict__ covered)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * N * C) return;
    const long long i = e / C;
    const int c = (int)(e - i * C);
    const int b = (int)(i / N);
    const unsigned slot = (unsigned)(i - (long long)b * N);
    const int r = index[i];
    long long lo;
    const long long n = vote_cloud(b, P, T, offsets, block_ids, row_base, batch_rows, lo);
    if (r < 0 || r >= n) return;
    const long long row = lo - row_base + r;
    if (stamp[row] != (((unsigned long long)(pass + 1u) << 32) | slot)) return;
    votes[row * C + c] += logits[e];                        // the only writer of this element in this pass
    if (c == 0) {
        const int seen = count[row] + 1;                    // (likewise)
        count[row] = seen;
        if (seen == min_votes && rows[(lo + r) * 8 + 7] == 1.0f) atomicAdd(&covered[b], 1);
    }
}

// arg-max, confusion counts and the non-finite rows of cloud blockIdx.y; LDS: C * C counters
__global__ __launch_bounds__(256) void vote_finalize_kernel(int C, int P, long long T, const float* __restrict__ rows,
                                                            const long long* __restrict__ offsets, const int* __restrict__ block_ids,
                                                            long long row_base, long long batch_rows, const float* __restrict__ votes,
                                                            int* __restrict__ pred, unsigned long long* __restrict__ confusion,
                                                            unsigned long long* __restrict__ nonfinite)
{
    extern __shared__ unsigned hist[];
    __shared__ unsigned bad;
    for (int k = threadIdx.x; k < C * C; k += 256) hist[k] = 0u;
    if (threadIdx.x == 0) bad = 0u;
    __syncthreads();
    const int b = blockIdx.y;
    long long lo;
    const long long n = vote_cloud(b, P, T, offsets, block_ids, row_base, batch_rows, lo);
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long long)gridDim.x * 256) {
        const long long row = lo - row_base + r;
        const float* v = votes + row * C;
        bool finite;
        const int arg = vote_argmax(v, 0, C, C, finite);
        pred[row] = arg;
        if (!finite) atomicAdd(&bad, 1u);
        const float* src = rows + (lo + r) * 8;
        const float lab = src[6];
        if (src[7] == 1.0f && lab >= 0.0f && lab < (float)C) atomicAdd(&hist[(int)lab * C + arg], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C * C; k += 256)
        if (hist[k] != 0u) atomicAdd(&confusion[k], (unsigned long long)hist[k]);
    if (threadIdx.x == 0 && bad != 0u) atomicAdd(nonfinite, (unsigned long long)bad);
}

}  // namespace sph3d

using namespace sph3d;

extern "C" size_t sph3d_vote_workspace(long long batch_rows)
{
    return batch_rows > 0 ? (size_t)batch_rows * sizeof(unsigned long long) : 0;
}

extern "C" int sph3d_vote_begin(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                                const int* block_ids, long long row_base, long long batch_rows, float* votes, int* count,
                                int* covered, int* inner_size, int* remaining, void* workspace, size_t workspace_bytes,
                                sph3d_stream_t stream)
{
    if (int rc = vote_check_args("vote_begin", B, C, num_blocks, total_rows, row_base, batch_rows)) return rc;
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && block_ids != nullptr, "vote_begin: null input pointer");
    SPH3D_REQUIRE(votes != nullptr && count != nullptr && covered != nullptr && inner_size != nullptr && remaining != nullptr,
                  "vote_begin: null output pointer");
    SPH3D_REQUIRE(workspace != nullptr && workspace_bytes >= sph3d_vote_workspace(batch_rows) &&
                      (reinterpret_cast<size_t>(workspace) & 7) == 0,
                  "vote_begin: workspace of %zu bytes, 8-byte aligned, required (got %zu)", sph3d_vote_workspace(batch_rows),
                  workspace_bytes);
    hipStream_t s = as_stream(stream);
    if (int rc = zero_async(votes, (size_t)batch_rows * C * sizeof(float), s, "vote_begin: votes")) return rc;
    if (int rc = zero_async(count, (size_t)batch_rows * sizeof(int), s, "vote_begin: count")) return rc;
    if (int rc = zero_async(workspace, sph3d_vote_workspace(batch_rows), s, "vote_begin: stamps")) return rc;
    if (int rc = zero_async(covered, (size_t)B * sizeof(int), s, "vote_begin: covered")) return rc;
    if (int rc = zero_async(inner_size, (size_t)B * sizeof(int), s, "vote_begin: inner_size")) return rc;
    hipLaunchKernelGGL(vote_inner_size_kernel, dim3(kVoteFinalizeParts, (unsigned)B), dim3(256), 0, s, num_blocks, total_rows, rows,
                       offsets, block_ids, row_base, batch_rows, inner_size);
    hipLaunchKernelGGL(vote_remaining_kernel, dim3(1), dim3(64), 0, s, B, covered, inner_size, remaining);
    return check_launch("sph3d_vote_begin");
}

extern "C" int sph3d_vote_accumulate(int B, int num_point, int C, int num_blocks, long long total_rows, const float* rows,
                                     const long long* offsets, const int* block_ids, long long row_base, long long batch_rows,
                                     int pass, const int* index, const float* logits, int min_votes, float* votes, int* count,
                                     int* covered, const int* inner_size, int* remaining, void* workspace, size_t workspace_bytes,
                                     sph3d_stream_t stream)
{
    if (int rc = vote_check_args("vote_accumulate", B, C, num_blocks, total_rows, row_base, batch_rows)) return rc;
    SPH3D_REQUIRE(num_point > 0, "vote_accumulate: num_point>0 required, got %d", num_point);
    SPH3D_REQUIRE(min_votes >= 1, "vote_accumulate: min_votes>=1 required, got %d", min_votes);
    SPH3D_REQUIRE(pass >= 0 && pass < (1 << 20), "vote_accumulate: pass in [0, 2^20) required, got %d", pass);
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && block_ids != nullptr && index != nullptr && logits != nullptr &&
                      inner_size != nullptr,
                  "vote_accumulate: null input pointer");
    SPH3D_REQUIRE(votes != nullptr && count != nullptr && covered != nullptr && remaining != nullptr,
                  "vote_accumulate: null output pointer");
    SPH3D_REQUIRE(workspace != nullptr && workspace_bytes >= sph3d_vote_workspace(batch_rows) &&
                      (reinterpret_cast<size_t>(workspace) & 7) == 0,
                  "vote_accumulate: workspace of %zu bytes, 8-byte aligned, required (got %zu)", sph3d_vote_workspace(batch_rows),
                  workspace_bytes);
    const long long slots = (long long)B * num_point;
    SPH3D_REQUIRE(slots * C <= 0x7fffffffll * 128, "vote_accumulate: B*num_point*C=%lld too large", slots * C);
    hipStream_t s = as_stream(stream);
    unsigned long long* stamp = static_cast<unsigned long long*>(workspace);
    hipLaunchKernelGGL(vote_stamp_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, B, num_point, num_blocks, total_rows,
                       offsets, block_ids, row_base, batch_rows, (unsigned)pass, index, stamp);
    hipLaunchKernelGGL(vote_add_kernel, dim3((unsigned)((slots * C + 255) / 256)), dim3(256), 0, s, B, num_point, C, num_blocks,
                       total_rows, rows, offsets, block_ids, row_base, batch_rows, (unsigned)pass, index, logits, min_votes, stamp,
                       votes, count, covered);
    hipLaunchKernelGGL(vote_remaining_kernel, dim3(1), dim3(64), 0, s, B, covered, inner_size, remaining);
    return check_launch("sph3d_vote_accumulate");
}

extern "C" int sph3d_vote_finalize(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                                   const int* block_ids, long long row_base, long long batch_rows, const float* votes, int* pred,
                                   long long* confusion, long long* nonfinite, sph3d_stream_t stream)
{
    if (int rc = vote_check_args("vote_finalize", B, C, num_blocks, total_rows, row_base, batch_rows)) return rc;
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && block_ids != nullptr && votes != nullptr, "vote_finalize: null input pointer");
    SPH3D_REQUIRE(pred != nullptr && confusion != nullptr && nonfinite != nullptr, "vote_finalize: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(confusion) & 7) == 0 && (reinterpret_cast<size_t>(nonfinite) & 7) == 0,
                  "vote_finalize: confusion and nonfinite must be 8-byte aligned");
    hipLaunchKernelGGL(vote_finalize_kernel, dim3(kVoteFinalizeParts, (unsigned)B), dim3(256), (size_t)C * C * sizeof(unsigned),
                       as_stream(stream), C, num_blocks, total_rows, rows, offsets, block_ids, row_base, batch_rows, votes, pred,
                       reinterpret_cast<unsigned long long*>(confusion), reinterpret_cast<unsigned long long*>(nonfinite));
    return check_launch("sph3d_vote_finalize");
}
