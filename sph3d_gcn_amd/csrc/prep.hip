// prep.hip — scene preparation for the segmentation nets: what the reference does offline before any network runs, MATLAB's
// pcdownsample(..., 'gridAverage', 0.03) (preprocesing/s3dis_prepare_data.m:35-37, scannet_prepare_data.m:101-107) and the block
// writer (io/make_tfrecord_s3dis.py:113-242): full cloud -> voxel cloud -> blocks of a pool with a scene index.
// harness/sceneprep.py states all of it in numpy; every output here equals that statement bit for bit, the fp32 means included.
// No floating-point atomic anywhere; every buffer is the caller's.
//
//   voxel grid    bounding box of the KEPT points (all 3+A values finite and at most 2^17 in magnitude; ordered-integer
//                 atomicMin / Max), the grid's shape by one thread (n_a = floor((hi_a - lo_a) / h) + 1; more than max_cells cells
//                 raises the header's flag and every later kernel returns), a dense int32 table of the cells: zero, mark the
//                 occupied cells, exclusive scan of the occupancy flags — the voxel row of every occupied cell, in ascending key
//                 for free — and voxel_of_point.  The scan is three passes over chunks of 4096 cells (per-chunk sums, one
//                 workgroup over the sums, per-chunk write): a room's table is 1e7 cells, which nn1's one-workgroup scan (sized
//                 for 2^21) would walk with 1e4 serial loads per thread, and a single-pass look-back scan would spin on other
//                 workgroups' flags; three streaming passes over 40 MB need neither.
//   voxel reduce  q = rint(v * 2^20) as a 64-bit integer (the double product is exact), S[row, col] += q, count[row] += 1:
//                 INTEGER sums, so the order of the adds cannot show.  Two forms with the same bits: 64-bit integer atomics (a
//                 thread per point and column: the lanes of a point add to 8 (3+A) contiguous bytes), or a counting sort of the
//                 points by row and a per-row sum.  finalize: mean = f32(f64(S) / f64(count) * 2^-20), and the box of the means.
//   normalise     c = (lo + hi) / 2 with c_z = lo_z, xyz' = xyz - c, rgb' = (2 rgb) / 255 - 1, separately rounded fp32 operations.
//   rect count    R rectangles (already rounded bounds, inclusive) in LDS tiles of 2048, a thread per point, wave ballot +
//                 popcount, one LDS integer atomic per rectangle and wave, one global one per rectangle and workgroup.
//   block fill    ordered compaction: per block and chunk of 64 points (one wave) the count inside the padded rectangle, an
//                 exclusive scan along the chunks of a block, and the fill of rows [T, 8] and index [T] at
//                 offsets[p] + chunk start + rank inside the wave — ascending voxel index by construction.
#pragma clang fp contract(off)
#include "common.hpp"

namespace sph3d {

constexpr int kPrepMaxAttr = 13;                 // 3 + A <= 16 columns
constexpr long long kPrepMaxCells = 1ll << 30;   // cell keys are int32
constexpr int kPrepChunk = 4096;                 // cells per workgroup of the scan: 256 threads x 16
constexpr int kPrepHdrWords = 16;                // the public header (sph3d.h)
constexpr size_t kPrepWsHdrBytes = 256;          // the private one: ordered-integer extrema and the kept count
constexpr int kPrepRectTile = 2048;              // rectangles per LDS tile
constexpr double kPrepQScale = 1048576.0;        // 2^20
constexpr float kPrepMaxValue = 131072.0f;       // 2^17

struct PrepBox {
    unsigned lo[3], hi[3];
    int kept, pad;
};

__device__ __forceinline__ bool prep_ok(float v) { return fabsf(v) <= kPrepMaxValue; }      // false for NaN and infinities

__device__ __forceinline__ bool prep_kept(long long i, int A, const float* __restrict__ xyz, const float* __restrict__ attr)
{
    bool ok = prep_ok(xyz[i * 3]) && prep_ok(xyz[i * 3 + 1]) && prep_ok(xyz[i * 3 + 2]);
    for (int a = 0; a < A; ++a) ok = ok && prep_ok(attr[i * A + a]);
    return ok;
}

// the cell of a kept point: i_a = floor((v_a - lo_a) / h), each operation rounded to fp32 once (contraction is off, `/` is the
// correctly rounded division); in [0, n_a) by the monotonicity of both roundings, clamped all the same
__device__ __forceinline__ int prep_axis(float v, float lo, float h, int n)
{
    const float t = floorf((v - lo) / h);
    return t >= 0.0f ? (t < (float)n ? (int)t : n - 1) : 0;
}
__device__ __forceinline__ int prep_key(const int* __restrict__ header, float h, float x, float y, float z)
{
    const int ny = header[4], nz = header[5];
    const int ix = prep_axis(x, __int_as_float(header[6]), h, header[3]);
    const int iy = prep_axis(y, __int_as_float(header[7]), h, ny);
    const int iz = prep_axis(z, __int_as_float(header[8]), h, nz);
    return (ix * ny + iy) * nz + iz;
}

static unsigned prep_grid(long long n, int per = 256, long long cap = 4096)
{
    long long blocks = (n + per - 1) / per;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// exclusive scan of one value per thread over a workgroup of 256 (four waves); -> the thread's prefix, total = the workgroup's sum
__device__ __forceinline__ int prep_block_scan(int v, int* tmp, int& total)
{
    const int lane = lane_id(), w = (int)threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    __syncthreads();                                   // (tmp may still be read from the previous use)
    if (lane == 63) tmp[w] = incl;
    __syncthreads();
    int run = incl - v;
    for (int k = 0; k < w; ++k) run += tmp[k];
    total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
    return run;
}

// ---- voxel grid ------------------------------------------------------------------------------------------------------------
// header: the public header of the voxel grid, or null (sph3d_prep_box)
__global__ void prep_grid_init_kernel(PrepBox* __restrict__ box, int* __restrict__ header)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int a = 0; a < 3; ++a) { box->lo[a] = 0xffffffffu; box->hi[a] = 0u; }
    box->kept = 0;
    box->pad = 0;
    if (header != nullptr)
        for (int k = 0; k < kPrepHdrWords; ++k) header[k] = 0;
}

// A < 0: the box of the FINITE points of xyz alone (sph3d_prep_box)
__global__ __launch_bounds__(256) void prep_bbox_kernel(long long F, int A, const float* __restrict__ xyz,
                                                        const float* __restrict__ attr, PrepBox* __restrict__ box)
{
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    int cnt = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < F; i += (long long)gridDim.x * 256) {
        const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
        if (A >= 0 ? !prep_kept(i, A, xyz, attr) : !(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY)) continue;
        const unsigned o[3] = {f2ord(x), f2ord(y), f2ord(z)};
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], o[a]); hi[a] = max(hi[a], o[a]); }
        ++cnt;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], (unsigned)__shfl_down((int)lo[a], off, 64));
            hi[a] = max(hi[a], (unsigned)__shfl_down((int)hi[a], off, 64));
        }
        cnt += __shfl_down(cnt, off, 64);
    }
    if (lane_id() == 0 && cnt != 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(&box->lo[a], lo[a]); atomicMax(&box->hi[a], hi[a]); }
        atomicAdd(&box->kept, cnt);
    }
}

__global__ void prep_grid_setup_kernel(long long F, float h, long long max_cells, const PrepBox* __restrict__ box,
                                       int* __restrict__ header)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int kept = box->kept;
    header[1] = (int)(F - kept);
    if (kept <= 0) { header[2] = 2; return; }
    int n[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = ord2f(box->lo[a]), hi = ord2f(box->hi[a]);
        header[6 + a] = __float_as_int(lo);
        header[9 + a] = __float_as_int(hi);
        const float t = floorf((hi - lo) / h);
        if (!(t >= 0.0f && t < (float)max_cells)) { header[2] = 1; return; }      // (also an overflowing quotient)
        n[a] = (int)t + 1;
    }
    long long cells = (long long)n[0] * n[1];
    if (cells <= max_cells) cells *= n[2];
    header[3] = n[0]; header[4] = n[1]; header[5] = n[2];
    if (cells > max_cells) { header[2] = 1; return; }
    header[12] = (int)cells;
}

__global__ __launch_bounds__(256) void prep_grid_zero_kernel(const int* __restrict__ header, int* __restrict__ cell)
{
    const long long n = header[2] != 0 ? 0 : header[12];
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long long)gridDim.x * 256) cell[k] = 0;
}

// MARK: cell[key] = 1 for every kept point (equal values from all writers).  else: voxel_of_point = the cell's row, -1 if dropped
template <bool MARK>
__global__ __launch_bounds__(256) void prep_grid_points_kernel(long long F, int A, float h, const float* __restrict__ xyz,
                                                               const float* __restrict__ attr, const int* __restrict__ header,
                                                               int* __restrict__ cell, int* __restrict__ voxel_of_point)
{
    const bool live = header[2] == 0;
    const int ncell = header[12];
    if (MARK && !live) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < F; i += (long long)gridDim.x * 256) {
        int row = -1;
        if (live && prep_kept(i, A, xyz, attr)) {
            const int key = prep_key(header, h, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]);
            if (key >= 0 && key < ncell) {
                if (MARK) cell[key] = 1;
                else row = cell[key];
            }
        }
        if (!MARK) voxel_of_point[i] = row;
    }
}

// ---- the three-pass exclusive scan over n ints (n on the device when n_dev is given).  FLAGS: the scanned value of an entry is
// (entry != 0) and an entry that is 0 becomes -1 (the cell table: row of an occupied cell); else the entries themselves.
__device__ __forceinline__ long long prep_scan_n(const int* n_dev, const int* flag_dev, long long n_host)
{
    if (flag_dev != nullptr && *flag_dev != 0) return 0;
    return n_dev != nullptr ? (long long)*n_dev : n_host;
}

template <bool FLAGS>
__global__ __launch_bounds__(256) void prep_scan_sum_kernel(const int* n_dev, const int* flag_dev, long long n_host,
                                                            const int* __restrict__ in, int* __restrict__ partial)
{
    __shared__ int tmp[4];
    const long long n = prep_scan_n(n_dev, flag_dev, n_host);
    const long long chunks = (n + kPrepChunk - 1) / kPrepChunk;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long k0 = c * kPrepChunk + (long long)threadIdx.x * 16;
        int s = 0;
        for (int k = 0; k < 16; ++k)
            if (k0 + k < n) s += FLAGS ? (in[k0 + k] != 0 ? 1 : 0) : in[k0 + k];
        int total;
        prep_block_scan(s, tmp, total);
        if (threadIdx.x == 0) partial[c] = total;
    }
}

// one workgroup of 1024: exclusive scan of the chunk sums in place; *total = the sum of all
__global__ __launch_bounds__(1024) void prep_scan_partial_kernel(const int* n_dev, const int* flag_dev, long long n_host,
                                                                 int* __restrict__ partial, int* __restrict__ total)
{
    __shared__ int tmp[16];
    const long long n = prep_scan_n(n_dev, flag_dev, n_host);
    const int chunks = (int)((n + kPrepChunk - 1) / kPrepChunk);
    const int tid = (int)threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int per = (chunks + 1023) / 1024;
    const int c0 = tid * per;
    int local = 0;
    for (int k = 0; k < per; ++k)
        if (c0 + k < chunks) local += partial[c0 + k];
    int incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) tmp[w] = incl;
    __syncthreads();
    int run = incl - local;
    for (int k = 0; k < w; ++k) run += tmp[k];
    for (int k = 0; k < per; ++k) {
        if (c0 + k < chunks) {
            const int v = partial[c0 + k];
            partial[c0 + k] = run;
            run += v;
        }
    }
    if (tid == 1023 && total != nullptr) *total = run;
}

template <bool FLAGS>
__global__ __launch_bounds__(256) void prep_scan_write_kernel(const int* n_dev, const int* flag_dev, long long n_host,
                                                              const int* in, const int* __restrict__ partial, int* out)
{
    __shared__ int tmp[4];
    const long long n = prep_scan_n(n_dev, flag_dev, n_host);
    const long long chunks = (n + kPrepChunk - 1) / kPrepChunk;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long k0 = c * kPrepChunk + (long long)threadIdx.x * 16;
        int v[16], s = 0;
        for (int k = 0; k < 16; ++k) {
            v[k] = k0 + k < n ? (FLAGS ? (in[k0 + k] != 0 ? 1 : 0) : in[k0 + k]) : 0;
            s += v[k];
        }
        int total;
        int run = partial[c] + prep_block_scan(s, tmp, total);
        for (int k = 0; k < 16; ++k) {
            if (k0 + k < n) out[k0 + k] = FLAGS ? (v[k] != 0 ? run : -1) : run;
            run += v[k];
        }
    }
}

template <bool FLAGS>
static void prep_scan(const int* n_dev, const int* flag_dev, long long n_host, long long n_max, const int* in, int* partial, int* out,
                      int* total, hipStream_t s)
{
    const unsigned blocks = prep_grid(n_max, kPrepChunk, 2048);
    hipLaunchKernelGGL(prep_scan_sum_kernel<FLAGS>, dim3(blocks), dim3(256), 0, s, n_dev, flag_dev, n_host, in, partial);
    hipLaunchKernelGGL(prep_scan_partial_kernel, dim3(1), dim3(1024), 0, s, n_dev, flag_dev, n_host, partial, total);
    hipLaunchKernelGGL(prep_scan_write_kernel<FLAGS>, dim3(blocks), dim3(256), 0, s, n_dev, flag_dev, n_host, in, partial, out);
}

static size_t prep_partial_bytes(long long n_max)
{
    return ((size_t)((n_max + kPrepChunk - 1) / kPrepChunk + 1) * sizeof(int) + 255) & ~(size_t)255;
}

// ---- voxel reduce ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long prep_q(float v) { return __double2ll_rn((double)v * kPrepQScale); }

__device__ __forceinline__ float prep_value(long long i, int col, int A, const float* __restrict__ xyz, const float* __restrict__ attr)
{
    return col < 3 ? xyz[i * 3 + col] : attr[i * A + (col - 3)];
}

// a thread per (point, column): the lanes of one point add to 8 (3 + A) contiguous bytes of its row
__global__ __launch_bounds__(256) void prep_reduce_atomic_kernel(long long F, int A, long long V, const float* __restrict__ xyz,
                                                                 const float* __restrict__ attr, const int* __restrict__ vop,
                                                                 unsigned long long* __restrict__ sums, int* __restrict__ count)
{
    const int D = 3 + A;
    const long long n = F * D;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const long long i = t / D;
        const int col = (int)(t - i * D);
        const long long row = vop[i];
        if (row < 0 || row >= V) continue;
        atomicAdd(&sums[row * D + col], (unsigned long long)prep_q(prep_value(i, col, A, xyz, attr)));
        if (col == 0) atomicAdd(&count[row], 1);
    }
}

// the sorted form.  COUNT: count[row] += 1.  else: order[cursor[row]++] = point (cursor = the rows' starts after the scan)
template <bool COUNT>
__global__ __launch_bounds__(256) void prep_reduce_sort_kernel(long long F, long long V, const int* __restrict__ vop,
                                                               int* __restrict__ counter, int* __restrict__ order)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < F; i += (long long)gridDim.x * 256) {
        const long long row = vop[i];
        if (row < 0 || row >= V) continue;
        const int pos = atomicAdd(&counter[row], 1);
        if (!COUNT && pos >= 0 && pos < F) order[pos] = (int)i;
    }
}

// a thread per (row, column): the row's points are order[end - count, end), end = the row's cursor after the fill
__global__ __launch_bounds__(256) void prep_reduce_rows_kernel(long long F, int A, long long V, const float* __restrict__ xyz,
                                                               const float* __restrict__ attr, const int* __restrict__ count,
                                                               const int* __restrict__ cursor, const int* __restrict__ order,
                                                               long long* __restrict__ sums)
{
    const int D = 3 + A;
    const long long n = V * D;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const long long row = t / D;
        const int col = (int)(t - row * D);
        const long long end = cursor[row];
        long long p = end - count[row];
        unsigned long long s = 0;
        if (p < 0 || end > F) p = end;
        for (; p < end; ++p) {
            const long long i = order[p];
            if (i >= 0 && i < F) s += (unsigned long long)prep_q(prep_value(i, col, A, xyz, attr));
        }
        sums[t] = (long long)s;
    }
}

__global__ __launch_bounds__(256) void prep_finalize_kernel(long long V, int A, const long long* __restrict__ sums,
                                                            const int* __restrict__ count, float* __restrict__ vxyz,
                                                            float* __restrict__ vattr)
{
    const int D = 3 + A;
    const long long n = V * D;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const long long row = t / D;
        const int col = (int)(t - row * D);
        const float mean = (float)(((double)sums[t] / (double)count[row]) * (1.0 / kPrepQScale));
        if (col < 3) vxyz[row * 3 + col] = mean;
        else vattr[row * A + (col - 3)] = mean;
    }
}

// ---- normalise ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_normalise_kernel(long long V, const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                             const PrepBox* __restrict__ box, float* __restrict__ out_xyz,
                                                             float* __restrict__ out_rgb)
{
    float c[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = ord2f(box->lo[a]), hi = ord2f(box->hi[a]);
        c[a] = a == 2 ? lo : (lo + hi) / 2.0f;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out_xyz[i * 3 + a] = xyz[i * 3 + a] - c[a];
            out_rgb[i * 3 + a] = (rgb[i * 3 + a] * 2.0f) / 255.0f - 1.0f;
        }
    }
}

// ---- rectangle counts --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool prep_inside(float x, float y, float x0, float x1, float y0, float y1)
{
    return x >= x0 && x <= x1 && y >= y0 && y <= y1;
}

__global__ __launch_bounds__(256) void prep_rect_count_kernel(long long V, int R, const float* __restrict__ xyz,
                                                              const float4* __restrict__ rects, int* __restrict__ counts)
{
    __shared__ float4 rs[kPrepRectTile];
    __shared__ int cs[kPrepRectTile];
    const int r0 = (int)blockIdx.y * kPrepRectTile;
    const int m = R - r0 < kPrepRectTile ? R - r0 : kPrepRectTile;
    for (int r = threadIdx.x; r < m; r += 256) { rs[r] = rects[r0 + r]; cs[r] = 0; }
    __syncthreads();
    const int lane = lane_id();
    for (long long base = (long long)blockIdx.x * 256; base < V; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        const bool live = i < V;
        const float x = live ? xyz[i * 3] : 0.0f, y = live ? xyz[i * 3 + 1] : 0.0f;
        for (int r = 0; r < m; ++r) {
            const float4 q = rs[r];
            const unsigned long long mask = __ballot(live && prep_inside(x, y, q.x, q.y, q.z, q.w));
            if (lane == 0 && mask != 0ull) atomicAdd(&cs[r], __popcll(mask));
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < m; r += 256)
        if (cs[r] != 0) atomicAdd(&counts[r0 + r], cs[r]);
}

// ---- block fill ----------------------------------------------------------------------------------------------------------------
// rects [P, 8]: the padded rectangle (x_lo, x_hi, y_lo, y_hi), then the plain one.  A wave takes chunks of 64 consecutive points.
// WRITE = false: cnt[p * chunks + c] = points of chunk c inside block p's padded rectangle.  WRITE = true: cnt holds the
// exclusive scan along c, and the points go to rows / index at offsets[p] + cnt + rank inside the wave.
template <bool WRITE>
__global__ __launch_bounds__(256) void prep_fill_kernel(long long V, int P, long long T, const float* __restrict__ xyz,
                                                        const float* __restrict__ rgb, const int* __restrict__ label,
                                                        const float* __restrict__ rects, const long long* __restrict__ offsets,
                                                        int* __restrict__ cnt, float* __restrict__ rows, int* __restrict__ index)
{
    const long long chunks = (V + 63) / 64;
    const int lane = lane_id();
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (long long)gridDim.x * 4;
    for (long long c = wave; c < chunks; c += waves) {
        const long long i = c * 64 + lane;
        const bool live = i < V;
        float x = 0.0f, y = 0.0f;
        if (live) { x = xyz[i * 3]; y = xyz[i * 3 + 1]; }
        for (int p = 0; p < P; ++p) {
            const float* r = rects + (size_t)p * 8;
            const bool in = live && prep_inside(x, y, r[0], r[1], r[2], r[3]);
            const unsigned long long mask = __ballot(in);
            if (!WRITE) {
                if (lane == 0) cnt[(size_t)p * chunks + c] = __popcll(mask);
                continue;
            }
            if (!in) continue;
            const long long lo = offsets[p], hi = offsets[p + 1];
            const long long at = lo + cnt[(size_t)p * chunks + c] + prefix_popc(mask);
            if (at < lo || at >= hi || at < 0 || at >= T) continue;          // (never, unless the cloud changed since the counts)
            const float inner = prep_inside(x, y, r[4], r[5], r[6], r[7]) ? 1.0f : 0.0f;
            float4* dst = reinterpret_cast<float4*>(rows + at * 8);
            dst[0] = make_float4(x, y, xyz[i * 3 + 2], rgb[i * 3]);
            dst[1] = make_float4(rgb[i * 3 + 1], rgb[i * 3 + 2], (float)label[i], inner);
            index[at] = (int)i;
        }
    }
}

// one workgroup per block: exclusive scan of the block's chunk counts in place; a total that is not the block's size counts in
// *mismatch
__global__ __launch_bounds__(256) void prep_fill_scan_kernel(long long V, int P, const long long* __restrict__ offsets,
                                                             int* __restrict__ cnt, int* __restrict__ mismatch)
{
    __shared__ int tmp[4];
    const long long chunks = (V + 63) / 64;
    const int p = (int)blockIdx.x;
    int* mine = cnt + (size_t)p * chunks;
    const long long per = (chunks + 255) / 256;
    const long long c0 = (long long)threadIdx.x * per;
    int s = 0;
    for (long long k = 0; k < per; ++k)
        if (c0 + k < chunks) s += mine[c0 + k];
    int total;
    int run = prep_block_scan(s, tmp, total);
    for (long long k = 0; k < per; ++k) {
        if (c0 + k < chunks) {
            const int v = mine[c0 + k];
            mine[c0 + k] = run;
            run += v;
        }
    }
    if (threadIdx.x == 0 && (long long)total != offsets[p + 1] - offsets[p]) atomicAdd(mismatch, 1);
}

}  // namespace sph3d

using namespace sph3d;

static bool prep_cloud_ok(long long F, int A) { return F > 0 && F <= 0x7fffffffll && A >= 0 && A <= kPrepMaxAttr; }

extern "C" size_t sph3d_prep_voxel_grid_workspace(long long F, long long max_cells)
{
    if (F <= 0 || F > 0x7fffffffll || max_cells < 1 || max_cells > kPrepMaxCells) return 0;
    return kPrepWsHdrBytes + prep_partial_bytes(max_cells) + (size_t)max_cells * sizeof(int);
}

extern "C" int sph3d_prep_voxel_grid(long long F, int A, const float* xyz, const float* attr, float h, long long max_cells,
                                     int* voxel_of_point, int* header, void* workspace, size_t workspace_bytes,
                                     sph3d_stream_t stream)
{
    SPH3D_REQUIRE(prep_cloud_ok(F, A), "prep_voxel_grid: 0<F<2^31 points and 0<=A<=%d attributes required, got %lld, %d", kPrepMaxAttr,
                  F, A);
    SPH3D_REQUIRE(h > 0.0f && h < INFINITY, "prep_voxel_grid: cell edge h>0 required, got %g", (double)h);
    SPH3D_REQUIRE(max_cells >= 1 && max_cells <= kPrepMaxCells, "prep_voxel_grid: 1<=max_cells<=2^30 required, got %lld", max_cells);
    SPH3D_REQUIRE(xyz != nullptr && (A == 0 || attr != nullptr), "prep_voxel_grid: null input pointer");
    SPH3D_REQUIRE(voxel_of_point != nullptr && header != nullptr, "prep_voxel_grid: null output pointer");
    const size_t need = sph3d_prep_voxel_grid_workspace(F, max_cells);
    SPH3D_REQUIRE(workspace != nullptr && workspace_bytes >= need && (reinterpret_cast<size_t>(workspace) & 15) == 0,
                  "prep_voxel_grid: workspace of %zu bytes, 16-byte aligned, required (got %zu)", need, workspace_bytes);
    hipStream_t s = as_stream(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    PrepBox* box = reinterpret_cast<PrepBox*>(ws);
    int* partial = reinterpret_cast<int*>(ws + kPrepWsHdrBytes);
    int* cell = reinterpret_cast<int*>(ws + kPrepWsHdrBytes + prep_partial_bytes(max_cells));
    const unsigned pblocks = prep_grid(F);
    hipLaunchKernelGGL(prep_grid_init_kernel, dim3(1), dim3(64), 0, s, box, header);
    hipLaunchKernelGGL(prep_bbox_kernel, dim3(pblocks), dim3(256), 0, s, F, A, xyz, attr, box);
    hipLaunchKernelGGL(prep_grid_setup_kernel, dim3(1), dim3(64), 0, s, F, h, max_cells, box, header);
    hipLaunchKernelGGL(prep_grid_zero_kernel, dim3(prep_grid(max_cells, 256, 8192)), dim3(256), 0, s, header, cell);
    hipLaunchKernelGGL(prep_grid_points_kernel<true>, dim3(pblocks), dim3(256), 0, s, F, A, h, xyz, attr, header, cell, voxel_of_point);
    prep_scan<true>(header + 12, header + 2, 0, max_cells, cell, partial, cell, header, s);
    hipLaunchKernelGGL(prep_grid_points_kernel<false>, dim3(pblocks), dim3(256), 0, s, F, A, h, xyz, attr, header, cell, voxel_of_point);
    return check_launch("sph3d_prep_voxel_grid");
}

extern "C" size_t sph3d_prep_voxel_reduce_workspace(long long F, long long V, int mode)
{
    if (F <= 0 || F > 0x7fffffffll || V <= 0 || V > F || mode != SPH3D_PREP_REDUCE_SORTED) return 0;
    const size_t rows = ((size_t)V * sizeof(int) + 255) & ~(size_t)255;
    return prep_partial_bytes(V) + rows + (size_t)F * sizeof(int);
}

extern "C" int sph3d_prep_voxel_reduce(long long F, int A, long long V, const float* xyz, const float* attr, const int* voxel_of_point,
                                       int mode, long long* sums, int* count, void* workspace, size_t workspace_bytes,
                                       sph3d_stream_t stream)
{
    SPH3D_REQUIRE(prep_cloud_ok(F, A), "prep_voxel_reduce: 0<F<2^31 points and 0<=A<=%d attributes required, got %lld, %d",
                  kPrepMaxAttr, F, A);
    SPH3D_REQUIRE(V > 0 && V <= F, "prep_voxel_reduce: 0<V<=F voxel rows required, got %lld", V);
    SPH3D_REQUIRE(mode == SPH3D_PREP_REDUCE_ATOMIC || mode == SPH3D_PREP_REDUCE_SORTED,
                  "prep_voxel_reduce: mode %d is neither atomic (0) nor sorted (1)", mode);
    SPH3D_REQUIRE(xyz != nullptr && (A == 0 || attr != nullptr) && voxel_of_point != nullptr, "prep_voxel_reduce: null input pointer");
    SPH3D_REQUIRE(sums != nullptr && count != nullptr && (reinterpret_cast<size_t>(sums) & 7) == 0,
                  "prep_voxel_reduce: sums (8-byte aligned) and count required");
    const size_t need = sph3d_prep_voxel_reduce_workspace(F, V, mode);
    SPH3D_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need && (reinterpret_cast<size_t>(workspace) & 15) == 0),
                  "prep_voxel_reduce: workspace of %zu bytes, 16-byte aligned, required (got %zu)", need, workspace_bytes);
    hipStream_t s = as_stream(stream);
    const int D = 3 + A;
    if (int rc = zero_async(count, (size_t)V * sizeof(int), s, "prep_voxel_reduce: count")) return rc;
    if (mode == SPH3D_PREP_REDUCE_ATOMIC) {
        if (int rc = zero_async(sums, (size_t)V * D * sizeof(long long), s, "prep_voxel_reduce: sums")) return rc;
        hipLaunchKernelGGL(prep_reduce_atomic_kernel, dim3(prep_grid(F * D, 256, 1 << 20)), dim3(256), 0, s, F, A, V, xyz, attr,
                           voxel_of_point, reinterpret_cast<unsigned long long*>(sums), count);
    } else {
        unsigned char* ws = static_cast<unsigned char*>(workspace);
        int* partial = reinterpret_cast<int*>(ws);
        int* cursor = reinterpret_cast<int*>(ws + prep_partial_bytes(V));
        int* order = reinterpret_cast<int*>(ws + prep_partial_bytes(V) + (((size_t)V * sizeof(int) + 255) & ~(size_t)255));
        hipLaunchKernelGGL(prep_reduce_sort_kernel<true>, dim3(prep_grid(F)), dim3(256), 0, s, F, V, voxel_of_point, count, order);
        prep_scan<false>(nullptr, nullptr, V, V, count, partial, cursor, nullptr, s);
        hipLaunchKernelGGL(prep_reduce_sort_kernel<false>, dim3(prep_grid(F)), dim3(256), 0, s, F, V, voxel_of_point, cursor, order);
        hipLaunchKernelGGL(prep_reduce_rows_kernel, dim3(prep_grid(V * D)), dim3(256), 0, s, F, A, V, xyz, attr, count, cursor, order,
                           sums);
    }
    return check_launch("sph3d_prep_voxel_reduce");
}

extern "C" int sph3d_prep_box(long long V, const float* xyz, int* box, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll, "prep_box: 0<V<2^31 points required, got %lld", V);
    SPH3D_REQUIRE(xyz != nullptr && box != nullptr, "prep_box: null pointer");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(prep_grid_init_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<PrepBox*>(box), static_cast<int*>(nullptr));
    hipLaunchKernelGGL(prep_bbox_kernel, dim3(prep_grid(V)), dim3(256), 0, s, V, -1, xyz, static_cast<const float*>(nullptr),
                       reinterpret_cast<PrepBox*>(box));
    return check_launch("sph3d_prep_box");
}

extern "C" int sph3d_prep_voxel_finalize(long long V, int A, const long long* sums, const int* count, float* voxel_xyz,
                                         float* voxel_attr, int* box, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll && A >= 0 && A <= kPrepMaxAttr,
                  "prep_voxel_finalize: 0<V<2^31 rows and 0<=A<=%d attributes required, got %lld, %d", kPrepMaxAttr, V, A);
    SPH3D_REQUIRE(sums != nullptr && count != nullptr, "prep_voxel_finalize: null input pointer");
    SPH3D_REQUIRE(voxel_xyz != nullptr && (A == 0 || voxel_attr != nullptr) && box != nullptr, "prep_voxel_finalize: null output pointer");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(prep_finalize_kernel, dim3(prep_grid(V * (3 + A))), dim3(256), 0, s, V, A, sums, count, voxel_xyz, voxel_attr);
    if (int rc = sph3d_prep_box(V, voxel_xyz, box, stream)) return rc;
    return check_launch("sph3d_prep_voxel_finalize");
}

extern "C" int sph3d_prep_normalise(long long V, const float* voxel_xyz, const float* voxel_rgb, const int* box, float* out_xyz,
                                    float* out_rgb, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll, "prep_normalise: 0<V<2^31 points required, got %lld", V);
    SPH3D_REQUIRE(voxel_xyz != nullptr && voxel_rgb != nullptr && box != nullptr && out_xyz != nullptr && out_rgb != nullptr,
                  "prep_normalise: null pointer");
    hipLaunchKernelGGL(prep_normalise_kernel, dim3(prep_grid(V)), dim3(256), 0, as_stream(stream), V, voxel_xyz, voxel_rgb,
                       reinterpret_cast<const PrepBox*>(box), out_xyz, out_rgb);
    return check_launch("sph3d_prep_normalise");
}

extern "C" int sph3d_prep_rect_count(long long V, int R, const float* xyz, const float* rects, int* counts, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll, "prep_rect_count: 0<V<2^31 points required, got %lld", V);
    SPH3D_REQUIRE(R > 0 && R <= kPrepRectTile * 65535, "prep_rect_count: 0<R<=%d rectangles required, got %d", kPrepRectTile * 65535, R);
    SPH3D_REQUIRE(xyz != nullptr && rects != nullptr && counts != nullptr, "prep_rect_count: null pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rects) & 15) == 0, "prep_rect_count: rects must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    if (int rc = zero_async(counts, (size_t)R * sizeof(int), s, "prep_rect_count: counts")) return rc;
    const unsigned tiles = (unsigned)((R + kPrepRectTile - 1) / kPrepRectTile);
    hipLaunchKernelGGL(prep_rect_count_kernel, dim3(prep_grid(V, 256, 1024), tiles), dim3(256), 0, s, V, R, xyz,
                       reinterpret_cast<const float4*>(rects), counts);
    return check_launch("sph3d_prep_rect_count");
}

extern "C" size_t sph3d_prep_block_fill_workspace(long long V, int P)
{
    if (V <= 0 || V > 0x7fffffffll || P <= 0) return 0;
    return (size_t)P * (size_t)((V + 63) / 64) * sizeof(int);
}

extern "C" int sph3d_prep_block_fill(long long V, int P, long long T, const float* xyz, const float* rgb, const int* label,
                                     const float* rects, const long long* offsets, float* rows, int* index, int* mismatch,
                                     void* workspace, size_t workspace_bytes, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(V > 0 && V <= 0x7fffffffll, "prep_block_fill: 0<V<2^31 points required, got %lld", V);
    SPH3D_REQUIRE(P > 0 && P <= 65535 && T > 0, "prep_block_fill: 0<P<=65535 blocks and T>0 rows required, got %d, %lld", P, T);
    SPH3D_REQUIRE(xyz != nullptr && rgb != nullptr && label != nullptr && rects != nullptr && offsets != nullptr,
                  "prep_block_fill: null input pointer");
    SPH3D_REQUIRE(rows != nullptr && index != nullptr && mismatch != nullptr, "prep_block_fill: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rows) & 15) == 0, "prep_block_fill: rows must be 16-byte aligned");
    const size_t need = sph3d_prep_block_fill_workspace(V, P);
    SPH3D_REQUIRE(workspace != nullptr && workspace_bytes >= need && (reinterpret_cast<size_t>(workspace) & 15) == 0,
                  "prep_block_fill: workspace of %zu bytes, 16-byte aligned, required (got %zu)", need, workspace_bytes);
    hipStream_t s = as_stream(stream);
    int* cnt = static_cast<int*>(workspace);
    const unsigned blocks = prep_grid((V + 63) / 64, 4, 4096);
    hipLaunchKernelGGL(prep_fill_kernel<false>, dim3(blocks), dim3(256), 0, s, V, P, T, xyz, rgb, label, rects, offsets, cnt, rows, index);
    hipLaunchKernelGGL(prep_fill_scan_kernel, dim3(P), dim3(256), 0, s, V, P, offsets, cnt, mismatch);
    hipLaunchKernelGGL(prep_fill_kernel<true>, dim3(blocks), dim3(256), 0, s, V, P, T, xyz, rgb, label, rects, offsets, cnt, rows, index);
    return check_launch("sph3d_prep_block_fill");
}
