// scene.hip — scene-level evaluation of the segmentation nets: what the reference does in MATLAB after the overlap-voting script
// (post-merging/s3dis_merge.m:42-82, scannet_merge.m:28-55): every block's summed logits are cut to a unit vector and soft-maxed
// per row, the inner rows' probabilities are added into a per-scene array through the record's index_label, the arg-max per scene
// point is the voxel-level prediction, and every point of the full-resolution cloud takes the prediction of its nearest voxel
// point (knnsearch).  harness/scenemerge.py states all of it in numpy; every output here equals that statement bit for bit, the
// fp32 probabilities included.  No floating-point atomic anywhere; every buffer is the caller's.
//
//   merge      ONE LAUNCH PER BLOCK, in the order of block_ids: the inner indices of a block are distinct (the pool refuses a
//              block where they are not), so inside a launch a scene row has one writer, and launches are ordered on the stream —
//              a scene row's adds happen in block order whatever the thread order.  A thread takes a row: s = sum of squares,
//              r = sqrt(s), z = sum of exp32(v / r), then merged[index] += exp32(v / r) / z.  Every operation is a separately
//              rounded fp32 one (contraction is off for this file; sqrt and division are the correctly rounded forms), and exp32
//              is the polynomial of include/sph3d_exp32.h that the numpy statement evaluates too.  At most 16 short launches per
//              batch beside the batch's forward passes; a stamp scheme as in vote.hip would save launches and cost a pass.
//   finalize   first-maximum arg-max per scene row (class 0 and `unseen` for a row without a hit), optional confusion counts.
//   nn1        nearest reference point of every query, exact in the fp32 predicate d2 = (dx*dx + dy*dy) + dz*dz, dx = q.x - r.x,
//              ties to the lowest index, d2 that is not finite never wins.
//              build   bounding box of the finite points (ordered-integer atomicMin / Max), a cell edge h such that the box holds
//                      about one cell per two points (at most kNn1MaxCells cells and kNn1MaxDim per axis), counting sort in
//                      global memory: count per cell, one-workgroup exclusive scan, fill of (x, y, z, index) in cell order.
//                      The fill's order inside a cell depends on the atomics' arrival; the search's result does not (the tie
//                      rule compares indices).  nn1_build (nn1grid.hpp) queues it; normals.hip's ball form calls it too, with
//                      a minimum cell edge (nn1 passes 0: the grid it always had).
//              search  a thread per query walks rings of cells (Chebyshev distance 0, 1, 2, ... from the query's cell; cells are
//                      z-fastest, so a column's share of a ring is one contiguous run of the sorted points).  After ring k every
//                      unvisited point differs from the query by more than (k - 4e-4) h along some axis: a point or a query lands
//                      in the wrong cell by at most 3 * 2^-24 * kNn1MaxDim = 1.8e-4 cells through the rounding of
//                      (v - lo) * invh.  The walk stops when best < (0.999 k h)^2 * 0.999: three orders of magnitude more margin
//                      than that and the 5 * 2^-24 relative rounding of the fp32 d2 need.  Queries are taken in the caller's
//                      order: neighbouring lanes diverge when neighbouring queries are far apart (tools/exp_scene.py measures
//                      the worst case, a shuffled cloud).
//              brute   256 queries per workgroup against tiles of 1024 reference points in LDS, ascending index, strict `<`.
//                      Runs when mode says so, or when the build raised the flag on the device: fewer than kNn1MinGrid finite
//                      points, a non-finite or zero extent.
//   lift       pred_full = pred_voxel[idx] (-1 where idx is -1), through label_map when given; optional confusion counts.
#pragma clang fp contract(off)
#include "common.hpp"
#include "nn1grid.hpp"
#include "../../include/sph3d_exp32.h"

namespace sph3d {

constexpr int kSceneMaxClasses = kVoteMaxClasses;
constexpr int kSceneParts = 64;             // workgroups of a merge launch (row-strided)
// (the grid's constants, its header and nn1_cell / finite3 / wave_sum: nn1grid.hpp, shared with normals.hip)

// ---- merge -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scene_merge_kernel(int b, int C, int P, long long T, const float* __restrict__ rows,
                                                          const long long* __restrict__ offsets, const int* __restrict__ index,
                                                          const int* __restrict__ block_ids, long long row_base,
                                                          long long batch_rows, const float* __restrict__ votes, long long V,
                                                          float* __restrict__ merged, int* __restrict__ hits,
                                                          unsigned long long* __restrict__ counters)
{
    long long lo;
    const long long n = vote_cloud(b, P, T, offsets, block_ids, row_base, batch_rows, lo);
    long long skipped = 0, outside = 0;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long long)gridDim.x * 256) {
        if (rows[(lo + r) * 8 + 7] != 1.0f) continue;
        const float* v = votes + (lo - row_base + r) * C;
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s = s + v[c] * v[c];
        if (!(s > 0.0f && s < INFINITY)) {           // all-zero, overflowing or non-finite sums (a NaN fails both)
            ++skipped;
            continue;
        }
        const float norm = sqrtf(s);                 // correctly rounded under the Makefile's flags (__fsqrt_rn is the bare v_sqrt_f32 here)
        float z = 0.0f;
        for (int c = 0; c < C; ++c) z = z + sph3d_exp32(v[c] / norm);
        const long long at = index[lo + r];
        if (at < 0 || at >= V) {
            ++outside;
            continue;
        }
        float* dst = merged + at * C;                // the only writer of this scene row in this launch
        for (int c = 0; c < C; ++c) dst[c] = dst[c] + sph3d_exp32(v[c] / norm) / z;
        hits[at] = hits[at] + 1;
    }
    skipped = wave_sum(skipped);
    outside = wave_sum(outside);
    if (lane_id() == 0) {
        if (skipped != 0) atomicAdd(&counters[0], (unsigned long long)skipped);
        if (outside != 0) atomicAdd(&counters[1], (unsigned long long)outside);
    }
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scene_finalize_kernel(int C, long long V, const float* __restrict__ merged,
                                                             const int* __restrict__ hits, const int* __restrict__ voxel_label,
                                                             int* __restrict__ pred, unsigned long long* __restrict__ unseen,
                                                             unsigned long long* __restrict__ confusion)
{
    extern __shared__ unsigned hist[];
    for (int k = threadIdx.x; k < C * C; k += 256) hist[k] = 0u;
    __syncthreads();
    long long mine = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        int arg = 0;
        bool finite;
        if (hits[i] > 0) arg = vote_argmax(merged + i * C, 0, C, C, finite);
        else ++mine;
        pred[i] = arg;
        if (voxel_label != nullptr) {
            const int lab = voxel_label[i];
            if (lab >= 0 && lab < C) atomicAdd(&hist[lab * C + arg], 1u);
        }
    }
    mine = wave_sum(mine);
    if (lane_id() == 0 && mine != 0) atomicAdd(unseen, (unsigned long long)mine);
    __syncthreads();
    if (confusion != nullptr)
        for (int k = threadIdx.x; k < C * C; k += 256)
            if (hist[k] != 0u) atomicAdd(&confusion[k], (unsigned long long)hist[k]);
}

// ---- lift ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scene_lift_kernel(int C, long long V, long long F, const int* __restrict__ pred_voxel,
                                                         const int* __restrict__ idx, const int* __restrict__ label_map,
                                                         const int* __restrict__ label_full, int* __restrict__ pred_full,
                                                         unsigned long long* __restrict__ confusion)
{
    extern __shared__ unsigned hist[];
    for (int k = threadIdx.x; k < C * C; k += 256) hist[k] = 0u;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < F; i += (long long)gridDim.x * 256) {
        const long long j = idx[i];
        int p = -1;
        if (j >= 0 && j < V) p = pred_voxel[j];
        const bool ok = p >= 0 && p < C;
        pred_full[i] = ok ? (label_map != nullptr ? label_map[p] : p) : -1;
        if (label_full != nullptr && ok) {
            const int lab = label_full[i];
            if (lab >= 0 && lab < C) atomicAdd(&hist[lab * C + p], 1u);
        }
    }
    __syncthreads();
    if (confusion != nullptr)
        for (int k = threadIdx.x; k < C * C; k += 256)
            if (hist[k] != 0u) atomicAdd(&confusion[k], (unsigned long long)hist[k]);
}

// ---- nn1: build ------------------------------------------------------------------------------------------------------------------
__global__ void nn1_init_kernel(Nn1Hdr* __restrict__ hdr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int a = 0; a < 3; a++) { hdr->lo[a] = 0xffffffffu; hdr->hi[a] = 0u; }
    hdr->nfin = 0; hdr->flag = 0;
    hdr->nx = hdr->ny = hdr->nz = hdr->ncell = 0;
}

__global__ __launch_bounds__(256) void nn1_bbox_kernel(long long V, const float* __restrict__ ref, Nn1Hdr* __restrict__ hdr)
{
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    int cnt = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const float x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
        if (!finite3(x, y, z)) continue;
        const unsigned o[3] = {f2ord(x), f2ord(y), f2ord(z)};
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], o[a]); hi[a] = max(hi[a], o[a]); }
        ++cnt;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = min(lo[a], (unsigned)__shfl_down((int)lo[a], off, 64));
            hi[a] = max(hi[a], (unsigned)__shfl_down((int)hi[a], off, 64));
        }
        cnt += __shfl_down(cnt, off, 64);
    }
    if (lane_id() == 0 && cnt != 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(&hdr->lo[a], lo[a]); atomicMax(&hdr->hi[a], hi[a]); }
        atomicAdd(&hdr->nfin, cnt);
    }
}

// the grid's shape, by one thread: the largest h (from the longest extent down in steps of 0.8) whose grid still has at most
// `target` cells and kNn1MaxDim - 1 steps per axis, and that is not below min_h (0 for sph3d_nn1: no such limit)
__global__ void nn1_setup_kernel(Nn1Hdr* __restrict__ hdr, float min_h)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int nfin = hdr->nfin;
    if (nfin < kNn1MinGrid) { hdr->flag = 1; return; }
    float lo[3], ext[3], maxext = 0.0f;
    for (int a = 0; a < 3; a++) {
        lo[a] = ord2f(hdr->lo[a]);
        ext[a] = ord2f(hdr->hi[a]) - lo[a];
        maxext = fmaxf(maxext, ext[a]);
    }
    if (!(maxext > 0.0f && maxext < INFINITY)) { hdr->flag = 1; return; }
    long long target = nfin / 2;
    target = target < kNn1MinCells ? kNn1MinCells : (target > kNn1MaxCells ? kNn1MaxCells : target);
    int n3[3] = {1, 1, 1};
    auto cells_at = [&](float h, int* n) -> long long {
        long long cells = 1;
        for (int a = 0; a < 3; a++) {
            const float e = ext[a] / h;
            if (!(e < (float)(kNn1MaxDim - 1))) return -1;
            n[a] = (int)e + 1;
            cells *= n[a];
        }
        return cells;
    };
    float h = maxext;
    for (int it = 0; it < 256; it++) {
        int t3[3];
        const float h2 = h * 0.8f;
        const long long c = cells_at(h2, t3);
        if (!(h2 > 0.0f) || h2 < min_h || c < 0 || c > target) break;
        h = h2;
    }
    const long long cells = cells_at(h, n3);
    const float invh = 1.0f / h;
    if (cells < 0 || cells > target || !(invh > 0.0f && invh < INFINITY)) { hdr->flag = 1; return; }
    hdr->minx = lo[0]; hdr->miny = lo[1]; hdr->minz = lo[2];
    hdr->h = h; hdr->invh = invh;
    hdr->nx = n3[0]; hdr->ny = n3[1]; hdr->nz = n3[2];
    hdr->ncell = (int)cells;
}

__device__ __forceinline__ int nn1_cell3(const Nn1Hdr& H, float x, float y, float z)
{
    return (nn1_cell(x, H.minx, H.invh, H.nx) * H.ny + nn1_cell(y, H.miny, H.invh, H.ny)) * H.nz + nn1_cell(z, H.minz, H.invh, H.nz);
}

// FILL = false: cell[c] += 1 per finite point.  FILL = true: cell[c] is the cell's cursor (its start after the scan); a point
// takes the next slot, and cell[c] ends as the END of cell c = the start of cell c + 1
template <bool FILL>
__global__ __launch_bounds__(256) void nn1_sort_kernel(long long V, const float* __restrict__ ref, const Nn1Hdr* __restrict__ hdr,
                                                       int* __restrict__ cell, float4* __restrict__ pts)
{
    const Nn1Hdr H = *hdr;
    if (H.flag != 0 || H.ncell <= 0) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const float x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
        if (!finite3(x, y, z)) continue;
        const int c = nn1_cell3(H, x, y, z);           // in [0, ncell): every axis is clamped
        const int pos = atomicAdd(&cell[c], 1);
        if (FILL && pos >= 0 && pos < V) pts[pos] = make_float4(x, y, z, __int_as_float((int)i));
    }
}

// exclusive scan of cell[0 .. ncell) in place, one workgroup of 1024 threads, a contiguous share per thread
__global__ __launch_bounds__(1024) void nn1_scan_kernel(const Nn1Hdr* __restrict__ hdr, int* __restrict__ cell)
{
    __shared__ int tmp[16];
    const int ncell = hdr->flag != 0 ? 0 : hdr->ncell;
    if (ncell <= 0) return;
    const int tid = (int)threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int per = (ncell + 1023) / 1024;
    const int c0 = tid * per;
    int local = 0;
    for (int k = 0; k < per; k++)
        if (c0 + k < ncell) local += cell[c0 + k];
    int incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) tmp[w] = incl;
    __syncthreads();
    int run = incl - local;
    for (int k = 0; k < w; k++) run += tmp[k];
    for (int k = 0; k < per; k++) {
        if (c0 + k < ncell) {
            const int c = cell[c0 + k];
            cell[c0 + k] = run;
            run += c;
        }
    }
}

// ---- nn1: search -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nn1_search_kernel(long long V, long long F, const float* __restrict__ query,
                                                         const Nn1Hdr* __restrict__ hdr, const int* __restrict__ cellEnd,
                                                         const float4* __restrict__ pts, int* __restrict__ idx)
{
    const Nn1Hdr H = *hdr;
    if (H.flag != 0 || H.ncell <= 0) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    const float qx = query[i * 3], qy = query[i * 3 + 1], qz = query[i * 3 + 2];
    if (!finite3(qx, qy, qz)) {
        idx[i] = -1;
        return;
    }
    const int nx = H.nx, ny = H.ny, nz = H.nz;
    const int cx = nn1_cell(qx, H.minx, H.invh, nx), cy = nn1_cell(qy, H.miny, H.invh, ny), cz = nn1_cell(qz, H.minz, H.invh, nz);
    float best = INFINITY;
    int arg = -1;
    // the points of cells [c0, c1] (consecutive cells are consecutive runs of pts)
    auto scan = [&](int c0, int c1) {
        int p = c0 > 0 ? cellEnd[c0 - 1] : 0;
        int e = cellEnd[c1];
        p = p < 0 ? 0 : p;
        e = e > V ? (int)V : e;
        for (; p < e; ++p) {
            const float4 r = pts[p];
            const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const int id = __float_as_int(r.w);
            if (d2 < best || (d2 == best && id < arg)) {
                best = d2;
                arg = id;
            }
        }
    };
    int maxr = max(max(cx, nx - 1 - cx), max(max(cy, ny - 1 - cy), max(cz, nz - 1 - cz)));
    for (int k = 0; k <= maxr; ++k) {
        const int x0 = max(cx - k, 0), x1 = min(cx + k, nx - 1), y0 = max(cy - k, 0), y1 = min(cy + k, ny - 1);
        const int z0 = max(cz - k, 0), z1 = min(cz + k, nz - 1);
        for (int X = x0; X <= x1; ++X) {
            const bool xedge = X == cx - k || X == cx + k;
            for (int Y = y0; Y <= y1; ++Y) {
                const int cb = (X * ny + Y) * nz;
                if (xedge || Y == cy - k || Y == cy + k) {
                    scan(cb + z0, cb + z1);
                } else {
                    if (cz - k >= 0) scan(cb + cz - k, cb + cz - k);
                    if (k > 0 && cz + k <= nz - 1) scan(cb + cz + k, cb + cz + k);
                }
            }
        }
        const float reach = (float)k * H.h * 0.999f;
        if (best < reach * reach * 0.999f) break;
    }
    idx[i] = arg;
}

__global__ __launch_bounds__(256) void nn1_brute_kernel(long long V, long long F, int force, const float* __restrict__ ref,
                                                        const float* __restrict__ query, const Nn1Hdr* __restrict__ hdr,
                                                        int* __restrict__ idx)
{
    __shared__ float4 tile[kNn1Tile];
    if (!force && hdr->flag == 0) return;              // uniform over the launch
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < F;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (live) { qx = query[i * 3]; qy = query[i * 3 + 1]; qz = query[i * 3 + 2]; }
    float best = INFINITY;
    int arg = -1;
    for (long long base = 0; base < V; base += kNn1Tile) {
        const int m = V - base < kNn1Tile ? (int)(V - base) : kNn1Tile;
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += 256) {
            const float* r = ref + (base + t) * 3;
            tile[t] = make_float4(r[0], r[1], r[2], 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < m; ++t) {
            const float4 r = tile[t];
            const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;      // a non-finite coordinate gives inf or NaN: never below `best`
            if (d2 < best) {
                best = d2;
                arg = (int)(base + t);
            }
        }
    }
    if (live) idx[i] = finite3(qx, qy, qz) ? arg : -1;
}

static unsigned strided_grid(long long n)
{
    long long blocks = (n + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
}

int nn1_build(long long V, const float* ref_xyz, float min_h, bool grid, const Nn1Ws& w, hipStream_t s)
{
    hipLaunchKernelGGL(nn1_init_kernel, dim3(1), dim3(64), 0, s, w.hdr);
    if (!grid) return SPH3D_OK;
    if (int rc = zero_async(w.cell, w.cellBytes, s, "nn1: cell counters")) return rc;
    hipLaunchKernelGGL(nn1_bbox_kernel, dim3(strided_grid(V)), dim3(256), 0, s, V, ref_xyz, w.hdr);
    hipLaunchKernelGGL(nn1_setup_kernel, dim3(1), dim3(64), 0, s, w.hdr, min_h);
    hipLaunchKernelGGL(nn1_sort_kernel<false>, dim3(strided_grid(V)), dim3(256), 0, s, V, ref_xyz, w.hdr, w.cell, w.pts);
    hipLaunchKernelGGL(nn1_scan_kernel, dim3(1), dim3(1024), 0, s, w.hdr, w.cell);
    hipLaunchKernelGGL(nn1_sort_kernel<true>, dim3(strided_grid(V)), dim3(256), 0, s, V, ref_xyz, w.hdr, w.cell, w.pts);
    return SPH3D_OK;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_scene_merge(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                                 const int* index, const int* block_ids, long long row_base, long long batch_rows,
                                 const float* votes, long long V, float* merged, int* hits, long long* counters,
                                 sph3d_stream_t stream)
{
    if (int rc = vote_check_args("scene_merge", B, C, num_blocks, total_rows, row_base, batch_rows)) return rc;
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll, "scene_merge: 0<V<2^31 scene rows required, got %lld", V);
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && index != nullptr && block_ids != nullptr && votes != nullptr,
                  "scene_merge: null input pointer");
    SPH3D_REQUIRE(merged != nullptr && hits != nullptr && counters != nullptr, "scene_merge: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(counters) & 7) == 0, "scene_merge: counters must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    for (int b = 0; b < B; ++b)
        hipLaunchKernelGGL(scene_merge_kernel, dim3(kSceneParts), dim3(256), 0, s, b, C, num_blocks, total_rows, rows, offsets, index,
                           block_ids, row_base, batch_rows, votes, V, merged, hits, reinterpret_cast<unsigned long long*>(counters));
    return check_launch("sph3d_scene_merge");
}

extern "C" int sph3d_scene_finalize(int C, long long V, const float* merged, const int* hits, const int* voxel_label,
                                    int* pred_voxel, long long* unseen_rows, long long* confusion, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(C > 0 && C <= kSceneMaxClasses, "scene_finalize: 0<C<=%d classes required, got %d", kSceneMaxClasses, C);
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll, "scene_finalize: 0<V<2^31 scene rows required, got %lld", V);
    SPH3D_REQUIRE(merged != nullptr && hits != nullptr, "scene_finalize: null input pointer");
    SPH3D_REQUIRE(pred_voxel != nullptr && unseen_rows != nullptr, "scene_finalize: null output pointer");
    SPH3D_REQUIRE((voxel_label == nullptr) == (confusion == nullptr), "scene_finalize: voxel_label and confusion come together");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(unseen_rows) & 7) == 0 && (reinterpret_cast<size_t>(confusion) & 7) == 0,
                  "scene_finalize: unseen_rows and confusion must be 8-byte aligned");
    hipLaunchKernelGGL(scene_finalize_kernel, dim3(strided_grid(V)), dim3(256), (size_t)C * C * sizeof(unsigned), as_stream(stream), C,
                       V, merged, hits, voxel_label, pred_voxel, reinterpret_cast<unsigned long long*>(unseen_rows),
                       reinterpret_cast<unsigned long long*>(confusion));
    return check_launch("sph3d_scene_finalize");
}

extern "C" int sph3d_scene_lift(int C, long long V, long long F, const int* pred_voxel, const int* idx, const int* label_map,
                                const int* label_full, int* pred_full, long long* confusion, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(C > 0 && C <= kSceneMaxClasses, "scene_lift: 0<C<=%d classes required, got %d", kSceneMaxClasses, C);
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll && F > 0 && F <= 0x7fffffffll, "scene_lift: 0<V,F<2^31 required, got %lld, %lld", V, F);
    SPH3D_REQUIRE(pred_voxel != nullptr && idx != nullptr && pred_full != nullptr, "scene_lift: null pointer");
    SPH3D_REQUIRE((label_full == nullptr) == (confusion == nullptr), "scene_lift: label_full and confusion come together");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(confusion) & 7) == 0, "scene_lift: confusion must be 8-byte aligned");
    hipLaunchKernelGGL(scene_lift_kernel, dim3(strided_grid(F)), dim3(256), (size_t)C * C * sizeof(unsigned), as_stream(stream), C, V,
                       F, pred_voxel, idx, label_map, label_full, pred_full, reinterpret_cast<unsigned long long*>(confusion));
    return check_launch("sph3d_scene_lift");
}

extern "C" size_t sph3d_nn1_workspace(long long V, long long F)
{
    if (V <= 0 || F <= 0 || V > 0x7fffffffll || F > 0x7fffffffll) return 0;
    return nn1_ws(nullptr, V).bytes;
}

extern "C" int sph3d_nn1(long long V, long long F, const float* ref_xyz, const float* query_xyz, int mode, int* idx,
                         void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll && F > 0 && F <= 0x7fffffffll, "nn1: 0<V,F<2^31 required, got %lld, %lld", V, F);
    SPH3D_REQUIRE(mode == SPH3D_NN1_GRID || mode == SPH3D_NN1_BRUTE, "nn1: mode %d is neither grid (0) nor brute (1)", mode);
    SPH3D_REQUIRE(ref_xyz != nullptr && query_xyz != nullptr && idx != nullptr, "nn1: null pointer");
    SPH3D_REQUIRE(workspace != nullptr && workspace_bytes >= sph3d_nn1_workspace(V, F) && (reinterpret_cast<size_t>(workspace) & 15) == 0,
                  "nn1: workspace of %zu bytes, 16-byte aligned, required (got %zu)", sph3d_nn1_workspace(V, F), workspace_bytes);
    hipStream_t s = as_stream(stream);
    const Nn1Ws w = nn1_ws(workspace, V);
    const unsigned qblocks = (unsigned)((F + 255) / 256);
    if (int rc = nn1_build(V, ref_xyz, 0.0f, mode == SPH3D_NN1_GRID, w, s)) return rc;
    if (mode == SPH3D_NN1_GRID)
        hipLaunchKernelGGL(nn1_search_kernel, dim3(qblocks), dim3(256), 0, s, V, F, query_xyz, w.hdr, w.cell, w.pts, idx);
    hipLaunchKernelGGL(nn1_brute_kernel, dim3(qblocks), dim3(256), 0, s, V, F, mode == SPH3D_NN1_BRUTE ? 1 : 0, ref_xyz, query_xyz,
                       w.hdr, idx);
    return check_launch("sph3d_nn1");
}
