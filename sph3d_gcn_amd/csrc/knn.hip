// knn.hip — exact k nearest neighbours of every query of a batch of clouds, in the searches' output format (nn_index, nn_count,
// nn_dist).  Not in the reference, whose searches are range searches that keep the first nn_sample points in index order.
// harness/knn.py states the op in numpy (knn_reference); every output here equals that statement bit for bit at every launch form.
//
//   predicate  dx = q.x - p.x, d2 = (dx*dx + dy*dy) + dz*dz in fp32, one rounding per operation (contraction is off for this
//              library): sph3d_nn1's d2.  A candidate is admitted iff d2 is finite and d2 < R2, R2 = radius * radius in fp32;
//              radius = +inf is "no radius".  This predicate is the op's own and deliberately simple: it is NOT the reference
//              kernel's fabs(dist - radius) > 1e-6 test, and no radius grows.  A row lists the admitted candidates in ascending
//              (d2, index) order, cut at k; unused slots hold index 0 and distance 0.
//   list       one wave per query.  The query's best k <= 64 candidates live one per lane, ascending, as 64-bit keys
//              (bits(d2) << 32) | index: for non-negative finite floats the bit order is the value order, so one unsigned compare
//              is the statement's order, ties included, and keys are distinct.  A step offers up to 64 candidates, one per lane;
//              a ballot of key < (current k-th key) discards most, the survivors are inserted one by one with a ballot (the
//              position), one shift up by a lane and a broadcast of the new k-th key.  No LDS traffic per candidate.
//   scan       4 queries per workgroup, a wave each (kKnnPerWave = 1: more per wave measured slower, knn_plan.hpp); the cloud is
//              staged in LDS as x, y, z planes, 1024 points per tile, once per workgroup; every wave walks the tile 64 points
//              per step.  Any N, no workspace.
//   grid       per cloud a counting-sorted cell grid in the caller's workspace: nn1grid.hpp's header, cell ends and points
//              (x, y, z, index bits) in cell order, cells z-fastest, about two points per cell — scene.hip's build, batched over
//              the clouds (the same passes as separate launches: header reset, bounding box of the finite points, shape, count,
//              scan, fill; no workgroup waits for another).  The fill's order inside a cell depends on the atomics' arrival; the
//              search's result does not (the keys order the list).
//              The search walks cube shells of cells (Chebyshev distance r = 0, 1, 2, ... from the query's cell; a query outside
//              the box starts from the clamped cell): a lane takes a column (X, Y) of the shell's square — its share of the shell
//              is one contiguous run of the sorted points, or the two end cells — and the lanes step through their runs together,
//              one candidate per lane and step.  After shell r every unvisited point differs from the query by more than
//              (r - 4e-4) h along some axis: a point or a query lands in the wrong cell by at most 3 * 2^-24 * kNn1MaxDim =
//              1.8e-4 cells through the rounding of (v - lo) * invh (nn1grid.hpp), and a query outside the box is farther still.
//              So every unvisited point has a true d2 above ((r - 4e-4) h)^2 and an fp32 d2 above that less 5 * 2^-24 relative;
//              the walk stops when the list is full and its k-th d2 < (0.999 r h)^2 * 0.999, or when R2 <= that bound (nothing
//              unvisited is admitted): three orders of magnitude more margin than both roundings need, as in scene.hip.  Without
//              a radius the list always fills: the grid takes only clouds of at least kNn1MinGrid = 64 >= k finite points.
//   fallback   a cloud the grid cannot index (fewer than 64 finite points, a zero or non-finite extent) has its header's flag
//              raised by the shape pass; the search skips it, and the scan kernel, queued behind the search, takes exactly the
//              flagged clouds.  The host reads nothing.
//   bounds     every loop is bounded by the grid's extent or by N; cell ends are clamped into [0, N] before they are used.
// The launch choice is knn_plan.hpp's: knn_plan().
#include "nn1grid.hpp"
#include "knn_plan.hpp"
#include <stddef.h>
#include <string.h>

namespace sph3d {

static_assert(kKnnMinCells == kNn1MinCells && kKnnMaxCells == kNn1MaxCells && kKnnHdrBytes == (long long)kNn1HdrBytes &&
                  kKnnTile == kNn1Tile && kKnnMaxK <= kNn1MinGrid && sizeof(Nn1Hdr) <= kNn1HdrBytes,
              "knn_plan.hpp restates nn1grid.hpp's layout");

constexpr unsigned long long kKnnKeyInf = ~0ull;

struct KnnWs {              // the grid form's workspace as the kernels see it
    unsigned char* hdr;
    unsigned char* cells;
    unsigned char* pts;
    long long cell_stride, point_stride;
};
__device__ __forceinline__ Nn1Hdr* knn_hdr(const KnnWs& w, long long b) { return reinterpret_cast<Nn1Hdr*>(w.hdr + b * (long long)kNn1HdrBytes); }
__device__ __forceinline__ int* knn_cells(const KnnWs& w, long long b) { return reinterpret_cast<int*>(w.cells + b * w.cell_stride); }
__device__ __forceinline__ float4* knn_pts(const KnnWs& w, long long b) { return reinterpret_cast<float4*>(w.pts + b * w.point_stride); }

// ---- the running list ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long knn_bcast(unsigned long long v, int src)        // src: uniform over the wave
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long knn_key(float d2, unsigned index, float R2)
{
    return d2 < R2 ? ((unsigned long long)(unsigned)__float_as_int(d2) << 32) | index : kKnnKeyInf;         // (NaN, inf: not admitted)
}

// `list`: lane l holds the l-th smallest key so far (kKnnKeyInf: none); `kth`: the key of lane k - 1, uniform.  `cand`: this lane's
// candidate or kKnnKeyInf.  At most 64 insertions.
__device__ __forceinline__ void knn_merge(unsigned long long& list, unsigned long long& kth, unsigned long long cand, int k, int lane)
{
    unsigned long long live = __ballot(cand < kth);
    while (live != 0) {
        const int j = __ffsll((long long)live) - 1;
        live &= live - 1;
        const unsigned long long x = knn_bcast(cand, j);
        if (x < kth) {                  // (uniform: an earlier insertion may have lowered kth below x)
            const int pos = __popcll(__ballot(list < x));               // the list is ascending: a prefix
            const unsigned long long up = __shfl_up(list, 1, 64);
            list = lane < pos ? list : (lane == pos ? x : up);
            kth = knn_bcast(list, k - 1);
        }
    }
}

__device__ __forceinline__ void knn_write(unsigned long long list, int k, int lane, int dist, long long row, int* __restrict__ nn_index,
                                          int* __restrict__ nn_count, float* __restrict__ nn_dist)
{
    const bool valid = lane < k && list != kKnnKeyInf;
    const int cnt = __popcll(__ballot(valid));
    if (lane < k) {
        const float d2 = valid ? __int_as_float((int)(unsigned)(list >> 32)) : 0.0f;
        nn_index[row * k + lane] = valid ? (int)(unsigned)list : 0;
        nn_dist[row * k + lane] = dist == SPH3D_KNN_DIST_SQUARED ? d2 : sqrtf(sqrtf(d2));
    }
    if (lane == 0) nn_count[row] = cnt;
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------
// work item = (cloud, group of kKnnQueries queries); gate != nullptr: only clouds whose header's flag is up (the grid's fallback)
__global__ __launch_bounds__(kKnnBlock) void knn_scan_kernel(int N, int M, int k, float R2, int dist, long long groups, long long items,
                                                             const float* __restrict__ database, const float* __restrict__ query,
                                                             const unsigned char* __restrict__ gate, int* __restrict__ nn_index,
                                                             int* __restrict__ nn_count, float* __restrict__ nn_dist)
{
    __shared__ float tx[kKnnTile], ty[kKnnTile], tz[kKnnTile];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long b = it / groups, g = it % groups;
        if (gate != nullptr && reinterpret_cast<const Nn1Hdr*>(gate + b * (long long)kNn1HdrBytes)->flag == 0) continue;       // uniform
        // this wave's queries m0 .. m0 + kKnnPerWave - 1: they share every step's points
        const long long m0 = g * kKnnQueries + (long long)wave * kKnnPerWave;
        float qx[kKnnPerWave], qy[kKnnPerWave], qz[kKnnPerWave];
        unsigned long long list[kKnnPerWave], kth[kKnnPerWave];
#pragma unroll
        for (int j = 0; j < kKnnPerWave; j++) {
            qx[j] = qy[j] = qz[j] = 0.0f;
            if (m0 + j < M) {
                const float* q = query + (b * M + m0 + j) * 3;
                qx[j] = q[0]; qy[j] = q[1]; qz[j] = q[2];
            }
            list[j] = kth[j] = kKnnKeyInf;
        }
        const float* P = database + b * N * 3;
        for (int base = 0; base < N; base += kKnnTile) {
            const int n = N - base < kKnnTile ? N - base : kKnnTile;
            __syncthreads();
            // (a point per thread, three strided loads: reading consecutive floats and sorting them into the planes by t / 3 and
            // t % 3 measured slower — 16 x 2048 -> 8192, k = 3: 380 against 313 us)
            for (int t = (int)threadIdx.x; t < n; t += kKnnBlock) {
                const float* r = P + (long long)(base + t) * 3;
                tx[t] = r[0]; ty[t] = r[1]; tz[t] = r[2];
            }
            __syncthreads();
            if (m0 < M) {
                for (int t0 = 0; t0 < n; t0 += 64) {
                    const int t = t0 + lane;
                    const bool in = t < n;
                    const float px = in ? tx[t] : 0.0f, py = in ? ty[t] : 0.0f, pz = in ? tz[t] : 0.0f;
#pragma unroll
                    for (int j = 0; j < kKnnPerWave; j++) {
                        if (m0 + j < M) {               // uniform over the wave
                            const float dx = qx[j] - px, dy = qy[j] - py, dz = qz[j] - pz;
                            const float d2 = (dx * dx + dy * dy) + dz * dz;
                            knn_merge(list[j], kth[j], in ? knn_key(d2, (unsigned)(base + t), R2) : kKnnKeyInf, k, lane);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kKnnPerWave; j++)
            if (m0 + j < M) knn_write(list[j], k, lane, dist, b * M + m0 + j, nn_index, nn_count, nn_dist);
    }
}

// ---- grid: build (scene.hip's nn1 build, a cloud per work item) -------------------------------------------------------------------
__global__ __launch_bounds__(kKnnBuildBlock) void knn_init_kernel(long long B, KnnWs w)
{
    for (long long b = (long long)blockIdx.x * kKnnBuildBlock + threadIdx.x; b < B; b += (long long)gridDim.x * kKnnBuildBlock) {
        Nn1Hdr* hdr = knn_hdr(w, b);
        for (int a = 0; a < 3; a++) { hdr->lo[a] = 0xffffffffu; hdr->hi[a] = 0u; }
        hdr->nfin = 0; hdr->flag = 0;
        hdr->minx = hdr->miny = hdr->minz = 0.0f; hdr->invh = hdr->h = 0.0f;
        hdr->nx = hdr->ny = hdr->nz = hdr->ncell = 0;
    }
}

__global__ __launch_bounds__(kKnnBuildBlock) void knn_bbox_kernel(long long items, int parts, int N, const float* __restrict__ database, KnnWs w)
{
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long b = it / parts;
        const int part = (int)(it % parts);
        const float* ref = database + b * N * 3;
        unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
        int cnt = 0;
        for (long long i = (long long)part * kKnnBuildBlock + threadIdx.x; i < N; i += (long long)parts * kKnnBuildBlock) {
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
            Nn1Hdr* hdr = knn_hdr(w, b);
#pragma unroll
            for (int a = 0; a < 3; a++) { atomicMin(&hdr->lo[a], lo[a]); atomicMax(&hdr->hi[a], hi[a]); }
            atomicAdd(&hdr->nfin, cnt);
        }
    }
}

// the grid's shape, a thread per cloud: nn1_setup_kernel's rule without a minimum cell edge — the largest h (from the longest
// extent down in steps of 0.8) whose grid still has at most nfin / 2 cells (held to [kNn1MinCells, kNn1MaxCells]) and
// kNn1MaxDim - 1 steps per axis
__global__ __launch_bounds__(kKnnBuildBlock) void knn_setup_kernel(long long B, KnnWs w)
{
    for (long long b = (long long)blockIdx.x * kKnnBuildBlock + threadIdx.x; b < B; b += (long long)gridDim.x * kKnnBuildBlock) {
        Nn1Hdr* hdr = knn_hdr(w, b);
        const int nfin = hdr->nfin;
        if (nfin < kNn1MinGrid) { hdr->flag = 1; continue; }
        float lo[3], ext[3], maxext = 0.0f;
        for (int a = 0; a < 3; a++) {
            lo[a] = ord2f(hdr->lo[a]);
            ext[a] = ord2f(hdr->hi[a]) - lo[a];
            maxext = fmaxf(maxext, ext[a]);
        }
        if (!(maxext > 0.0f && maxext < INFINITY)) { hdr->flag = 1; continue; }
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
            if (!(h2 > 0.0f) || c < 0 || c > target) break;
            h = h2;
        }
        const long long cells = cells_at(h, n3);
        const float invh = 1.0f / h;
        if (cells < 0 || cells > target || !(invh > 0.0f && invh < INFINITY)) { hdr->flag = 1; continue; }
        hdr->minx = lo[0]; hdr->miny = lo[1]; hdr->minz = lo[2];
        hdr->h = h; hdr->invh = invh;
        hdr->nx = n3[0]; hdr->ny = n3[1]; hdr->nz = n3[2];
        hdr->ncell = (int)cells;
    }
}

// FILL = false: cell[c] += 1 per finite point.  FILL = true: cell[c] is the cell's cursor (its start after the scan); a point
// takes the next slot, and cell[c] ends as the END of cell c.  ncell <= the plan's cells: target <= N / 2 held to the same range
template <bool FILL>
__global__ __launch_bounds__(kKnnBuildBlock) void knn_sort_kernel(long long items, int parts, int N, const float* __restrict__ database, KnnWs w)
{
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long b = it / parts;
        const int part = (int)(it % parts);
        const Nn1Hdr H = *knn_hdr(w, b);
        if (H.flag != 0 || H.ncell <= 0) continue;
        const float* ref = database + b * N * 3;
        int* cell = knn_cells(w, b);
        float4* pts = knn_pts(w, b);
        for (long long i = (long long)part * kKnnBuildBlock + threadIdx.x; i < N; i += (long long)parts * kKnnBuildBlock) {
            const float x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
            if (!finite3(x, y, z)) continue;
            const int c = (nn1_cell(x, H.minx, H.invh, H.nx) * H.ny + nn1_cell(y, H.miny, H.invh, H.ny)) * H.nz +
                          nn1_cell(z, H.minz, H.invh, H.nz);            // in [0, ncell): every axis is clamped
            const int pos = atomicAdd(&cell[c], 1);
            if (FILL && pos >= 0 && pos < N) pts[pos] = make_float4(x, y, z, __int_as_float((int)i));
        }
    }
}

// exclusive scan of a cloud's cell[0 .. ncell) in place, one workgroup of 1024 threads, a contiguous share per thread
__global__ __launch_bounds__(kKnnPrefixBlock) void knn_prefix_kernel(long long B, KnnWs w)
{
    __shared__ int tmp[16];
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const Nn1Hdr* hdr = knn_hdr(w, b);
        const int ncell = hdr->flag != 0 ? 0 : hdr->ncell;
        if (ncell <= 0) continue;           // uniform
        int* cell = knn_cells(w, b);
        const int per = (ncell + kKnnPrefixBlock - 1) / kKnnPrefixBlock;
        const int c0 = tid * per;
        int local = 0;
        for (int j = 0; j < per; j++)
            if (c0 + j < ncell) local += cell[c0 + j];
        int incl = local;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        __syncthreads();                    // (the previous cloud's readers of tmp are done)
        if (lane == 63) tmp[wv] = incl;
        __syncthreads();
        int run = incl - local;
        for (int j = 0; j < wv; j++) run += tmp[j];
        for (int j = 0; j < per; j++) {
            if (c0 + j < ncell) {
                const int c = cell[c0 + j];
                cell[c0 + j] = run;
                run += c;
            }
        }
    }
}

// ---- grid: search ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKnnBlock) void knn_grid_kernel(int N, int M, int k, float R2, int dist, long long groups, long long items,
                                                             const float* __restrict__ query, KnnWs w, int* __restrict__ nn_index,
                                                             int* __restrict__ nn_count, float* __restrict__ nn_dist)
{
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long b = it / groups;
        const Nn1Hdr H = *knn_hdr(w, b);
        if (H.flag != 0 || H.ncell <= 0) continue;              // the scan behind this launch takes the cloud
        for (int j = 0; j < kKnnPerWave; ++j) {                 // this wave's queries (kKnnPerWave = 1)
            const long long m = (it % groups) * kKnnQueries + (long long)wave * kKnnPerWave + j;
            if (m >= M) break;
            const float* q = query + (b * M + m) * 3;
            const float qx = q[0], qy = q[1], qz = q[2];
            unsigned long long list = kKnnKeyInf, kth = kKnnKeyInf;
            if (finite3(qx, qy, qz)) {
                const int* __restrict__ cellEnd = knn_cells(w, b);
                const float4* __restrict__ pts = knn_pts(w, b);
                const int nx = H.nx, ny = H.ny, nz = H.nz;
                const int cx = nn1_cell(qx, H.minx, H.invh, nx), cy = nn1_cell(qy, H.miny, H.invh, ny), cz = nn1_cell(qz, H.minz, H.invh, nz);
                // the points of cells [c0, c1] (consecutive cells are consecutive runs of pts), clamped into the cloud
                auto run = [&](int c0, int c1, int& p, int& e) {
                    p = c0 > 0 ? cellEnd[c0 - 1] : 0;
                    e = cellEnd[c1];
                    p = p < 0 ? 0 : p;
                    e = e > N ? N : e;
                };
                const int maxr = max(max(cx, nx - 1 - cx), max(max(cy, ny - 1 - cy), max(cz, nz - 1 - cz)));
                for (int r = 0; r <= maxr; ++r) {
                    const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
                    const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
                    const int wy = y1 - y0 + 1, ncol = (x1 - x0 + 1) * wy;
                    for (int t0 = 0; t0 < ncol; t0 += 64) {
                        const int t = t0 + lane;
                        int pa = 0, ea = 0, pb = 0, eb = 0;
                        if (t < ncol) {
                            const int X = x0 + t / wy, Y = y0 + t % wy;
                            const int cb = (X * ny + Y) * nz;
                            if (X == cx - r || X == cx + r || Y == cy - r || Y == cy + r) {
                                run(cb + z0, cb + z1, pa, ea);
                            } else {
                                if (cz - r >= 0) run(cb + cz - r, cb + cz - r, pa, ea);
                                if (cz + r <= nz - 1) run(cb + cz + r, cb + cz + r, pb, eb);        // (r > 0 here: r == 0 is an edge column)
                            }
                        }
                        // every trip takes a point off each unfinished lane's runs: at most N trips
                        while (__ballot(pa < ea || pb < eb) != 0) {
                            int p = -1;
                            if (pa < ea) p = pa++;
                            else if (pb < eb) p = pb++;
                            unsigned long long key = kKnnKeyInf;
                            if (p >= 0) {
                                const float4 rr = pts[p];
                                const float dx = qx - rr.x, dy = qy - rr.y, dz = qz - rr.z;
                                const float d2 = (dx * dx + dy * dy) + dz * dz;
                                key = knn_key(d2, (unsigned)__float_as_int(rr.w), R2);
                            }
                            knn_merge(list, kth, key, k, lane);
                        }
                    }
                    const float reach = (float)r * H.h * 0.999f;
                    const float bound = reach * reach * 0.999f;
                    if ((kth != kKnnKeyInf && __int_as_float((int)(unsigned)(kth >> 32)) < bound) || R2 <= bound) break;
                }
            }
            knn_write(list, k, lane, dist, b * M + m, nn_index, nn_count, nn_dist);
        }
    }
}

}  // namespace sph3d

using namespace sph3d;

// The plan of a call, or the status and message of the arguments it rejects (the entry and the plan query answer alike)
static int knn_checked_plan(KnnPlan* p, int B, int N, int M, int k, float radius, int mode)
{
    *p = knn_plan(B, N, M, k, radius, mode);
    SPH3D_REQUIRE(p->bad != kKnnBadK, "build_nearest_neighbor: k>=1 required, got %d", k);
    if (p->bad == kKnnBigK) {
        set_error("build_nearest_neighbor: k<=%d supported, got %d", kKnnMaxK, k);
        return SPH3D_EUNSUPPORTED;
    }
    SPH3D_REQUIRE(p->bad != kKnnBadRadius, "build_nearest_neighbor: radius>0 required (+inf: none)");
    SPH3D_REQUIRE(p->bad != kKnnBadDims, "build_nearest_neighbor: bad dims B=%d N=%d M=%d", B, N, M);
    SPH3D_REQUIRE(p->bad != kKnnBadSize, "build_nearest_neighbor: bad dims B=%d N=%d M=%d (B N and B M <= 2^40)", B, N, M);
    SPH3D_REQUIRE(p->bad != kKnnBadMode, "build_nearest_neighbor: mode %d is none of auto (0), scan (1), grid (2)", mode);
    return SPH3D_OK;
}

// 0 for arguments the entry rejects
extern "C" size_t sph3d_build_nearest_neighbor_workspace(int B, int N, int M, int k, int mode)
{
    return (size_t)knn_plan(B, N, M, k, INFINITY, mode).workspace_bytes;
}

extern "C" int sph3d_build_nearest_neighbor_plan(int B, int N, int M, int k, float radius, int mode, long long* out)
{
    KnnPlan p;
    int rc = knn_checked_plan(&p, B, N, M, k, radius, mode);
    if (rc) return rc;
    SPH3D_REQUIRE(out != nullptr, "sph3d_build_nearest_neighbor_plan: out is NULL");
    static_assert(offsetof(KnnPlan, bad) == SPH3D_KNN_PLAN_FIELDS * sizeof(long long), "the plan starts with the documented fields, in their order");
    static_assert(kKnnNone == SPH3D_KNN_FORM_NONE && kKnnScan == SPH3D_KNN_FORM_SCAN && kKnnGrid == SPH3D_KNN_FORM_GRID &&
                      kKnnModeAuto == SPH3D_KNN_AUTO && kKnnModeScan == SPH3D_KNN_SCAN && kKnnModeGrid == SPH3D_KNN_GRID,
                  "the forms and modes as the header numbers them");
    memcpy(out, &p, SPH3D_KNN_PLAN_FIELDS * sizeof(long long));
    return SPH3D_OK;
}

extern "C" int sph3d_build_nearest_neighbor(int B, int N, int M, int k, float radius, int mode, int dist, const float* database,
                                            const float* query, int* nn_index, int* nn_count, float* nn_dist, void* workspace,
                                            size_t workspace_bytes, sph3d_stream_t stream)
{
    KnnPlan p;
    int rc = knn_checked_plan(&p, B, N, M, k, radius, mode);
    if (rc) return rc;
    SPH3D_REQUIRE(dist == SPH3D_KNN_DIST_ROOT || dist == SPH3D_KNN_DIST_SQUARED, "build_nearest_neighbor: dist %d is neither root (0) nor squared (1)", dist);
    if (p.form == kKnnNone) return SPH3D_OK;
    SPH3D_REQUIRE(database != nullptr && query != nullptr && nn_index != nullptr && nn_count != nullptr && nn_dist != nullptr,
                  "build_nearest_neighbor: null pointer");
    if (p.workspace_bytes != 0 && (workspace == nullptr || workspace_bytes < (size_t)p.workspace_bytes || (reinterpret_cast<size_t>(workspace) & 15) != 0)) {
        set_error("build_nearest_neighbor: workspace of %zu bytes, 16-byte aligned, required (got %zu)", (size_t)p.workspace_bytes, workspace_bytes);
        return SPH3D_EWORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    const float R2 = radius * radius;
    const long long items = (long long)B * p.groups;
    const dim3 block((unsigned)p.block);
    if (p.form == kKnnScan) {
        hipLaunchKernelGGL(knn_scan_kernel, dim3((unsigned)p.scan_grid), block, 0, s, N, M, k, R2, dist, p.groups, items, database, query,
                           (const unsigned char*)nullptr, nn_index, nn_count, nn_dist);
        return check_launch("sph3d_build_nearest_neighbor");
    }
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const KnnWs w = {ws + p.off_hdr, ws + p.off_cells, ws + p.off_points, p.cell_stride, p.point_stride};
    const long long bitems = (long long)B * p.build_parts;
    const int parts = (int)p.build_parts;
    const dim3 bblock((unsigned)p.build_block), bgrid((unsigned)p.build_grid), sgrid((unsigned)p.setup_grid);
    hipLaunchKernelGGL(knn_init_kernel, sgrid, bblock, 0, s, (long long)B, w);
    if ((rc = zero_async(w.cells, (size_t)(B * p.cell_stride), s, "build_nearest_neighbor: cell counters"))) return rc;
    hipLaunchKernelGGL(knn_bbox_kernel, bgrid, bblock, 0, s, bitems, parts, N, database, w);
    hipLaunchKernelGGL(knn_setup_kernel, sgrid, bblock, 0, s, (long long)B, w);
    hipLaunchKernelGGL(knn_sort_kernel<false>, bgrid, bblock, 0, s, bitems, parts, N, database, w);
    hipLaunchKernelGGL(knn_prefix_kernel, dim3((unsigned)p.prefix_grid), dim3((unsigned)p.prefix_block), 0, s, (long long)B, w);
    hipLaunchKernelGGL(knn_sort_kernel<true>, bgrid, bblock, 0, s, bitems, parts, N, database, w);
    hipLaunchKernelGGL(knn_grid_kernel, dim3((unsigned)p.search_grid), block, 0, s, N, M, k, R2, dist, p.groups, items, query, w, nn_index,
                       nn_count, nn_dist);
    // the fallback: returns at once per cloud unless the build raised its flag
    hipLaunchKernelGGL(knn_scan_kernel, dim3((unsigned)p.scan_grid), block, 0, s, N, M, k, R2, dist, p.groups, items, database, query,
                       (const unsigned char*)w.hdr, nn_index, nn_count, nn_dist);
    return check_launch("sph3d_build_nearest_neighbor");
}
