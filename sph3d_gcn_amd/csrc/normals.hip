// normals.hip — surface normals from order-free integer ball moments.  harness/normals.py states all of it in numpy; the ten
// integer moments and the count of every row equal that statement bit for bit, the normal and the variation are held to the
// per-element bounds of tests/_normal_ref.py.  include/sph3d.h carries the statement; in short:
//
//   offsets    d = p - q per axis (one fp32 subtraction), t = rint((double)d * Q), Q = 2^18 / radius; a neighbour counts when
//              |(double)d * Q| <= 2^21 on all three axes (a non-finite offset fails), else it is skipped.
//   moments    n, S1_a = sum t_a, S2_ab = sum t_a t_b as signed 64-bit integers (v_mad_i64_i32: |t| fits 32 bits).  Integer sums
//              are order-free, so the lane mapping, the fill order of the cell grid and the path (grid or brute force) cannot show.
//   finish     ONE device function for both forms: float64 covariance c_ab = S2_ab / n - m_a m_b (contraction is off), cyclic
//              Jacobi on the 3x3 matrix, the eigenvector of the smallest eigenvalue, the sign rule, one rounding to fp32.
//              Jacobi never divides by an eigenvalue gap: an exact plane (a zero row and column) and coinciding eigenvalues
//              end in orthonormal vectors like any other matrix.
//
//   graph form 256 rows per workgroup.  Pass 1: a quarter wave per row reads the row's index words 16 at a time (one 64-byte
//              segment), gathers the points, and folds its ten sums with four xor shuffles; lane 0 leaves them in LDS
//              (20 KB).  Pass 2: a thread per row takes its sums from LDS and finishes, so the float64 solve runs with every
//              lane busy instead of one in sixteen.  No workspace; the one atomic is the skipped-neighbour counter, one add per wave.
//   ball form  scene.hip's counting-sorted grid (nn1_build) with a minimum cell edge of `radius`.  A thread per SORTED point:
//              neighbouring lanes sit in the same or adjacent cells and walk the same runs of points, and a query needs no
//              cross-lane reduction.  The walk covers the cells [floor(f - r/h - slack), floor(f + r/h + slack)] per axis
//              (three cells when h >= radius; the whole grid for a radius beyond the cloud) and takes a column's cells as one
//              run (cells are z-fastest).  Clouds the grid cannot index (the build's flag) go through the tiled brute-force
//              kernel, which returns at once otherwise.  Both apply the same fp32 predicate (dx*dx + dy*dy) + dz*dz < r2.
#pragma clang fp contract(off)
#include "common.hpp"
#include "nn1grid.hpp"

namespace sph3d {

constexpr int kNrmRows = 256;               // rows per workgroup of the graph form
constexpr long long kNrmMaxBall = 1ll << 26;
constexpr double kNrmLimit = 2097152.0;     // 2^21: largest |t| of a valid neighbour
// walk margin in cells: point and query each land in the wrong cell by at most 1.8e-4 (nn1grid.hpp); r * invh, f - r and f + r
// round by at most 2^-24 * kNn1MaxDim = 6e-5 each; |dx| <= r (1 + 2^-22) for a point the fp32 predicate accepts
constexpr float kNrmCellSlack = 1e-3f;

struct Moments {
    long long v[10];                        // n, S1 x y z, S2 xx xy xz yy yz zz
};

__device__ __forceinline__ void moments_zero(Moments& m)
{
#pragma unroll
    for (int j = 0; j < 10; ++j) m.v[j] = 0;
}

// one neighbour: -> true when it counted
__device__ __forceinline__ bool moments_add(Moments& m, float dx, float dy, float dz, double Q)
{
    const double ux = (double)dx * Q, uy = (double)dy * Q, uz = (double)dz * Q;
    if (!(fabs(ux) <= kNrmLimit && fabs(uy) <= kNrmLimit && fabs(uz) <= kNrmLimit)) return false;      // (a NaN fails)
    const int tx = (int)rint(ux), ty = (int)rint(uy), tz = (int)rint(uz);
    m.v[0] += 1;
    m.v[1] += tx; m.v[2] += ty; m.v[3] += tz;
    m.v[4] += (long long)tx * tx; m.v[5] += (long long)tx * ty; m.v[6] += (long long)tx * tz;
    m.v[7] += (long long)ty * ty; m.v[8] += (long long)ty * tz; m.v[9] += (long long)tz * tz;
    return true;
}

// one Jacobi rotation that annihilates a[P][Q] (Rutishauser's update: the rotation is applied as corrections to the entries)
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3], int sweep)
{
    constexpr int R = 3 - P - Q;
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double g = 100.0 * fabs(apq);
    if (sweep > 3 && fabs(a[P][P]) + g == fabs(a[P][P]) && fabs(a[Q][Q]) + g == fabs(a[Q][Q])) {
        a[P][Q] = 0.0;
        return;
    }
    double h = a[Q][Q] - a[P][P], t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
    h = t * apq;
    a[P][P] -= h;
    a[Q][Q] += h;
    a[P][Q] = 0.0;
    // the third row / column: entries (R, P) and (R, Q), kept in the upper triangle
    double& arp = R < P ? a[R][P] : a[P][R];
    double& arq = R < Q ? a[R][Q] : a[Q][R];
    const double gp = arp, hq = arq;
    arp = gp - s * (hq + gp * tau);
    arq = hq + s * (gp - hq * tau);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vg = v[k][P], vh = v[k][Q];
        v[k][P] = vg - s * (vh + vg * tau);
        v[k][Q] = vh + s * (vg - vh * tau);
    }
}

// ten integers -> the row's outputs.  q: the query; toward: the point normals face (null: canonical sign only)
__device__ __forceinline__ void normals_finish(const Moments& m, float qx, float qy, float qz, const float* __restrict__ toward,
                                               int min_count, long long row, float* __restrict__ normals,
                                               float* __restrict__ variation, int* __restrict__ count,
                                               long long* __restrict__ moments)
{
    if (count != nullptr) count[row] = (int)m.v[0];
    if (moments != nullptr) {
#pragma unroll
        for (int j = 0; j < 10; ++j) moments[row * 10 + j] = m.v[j];
    }
    float out[3] = {0.0f, 0.0f, 0.0f}, var = 0.0f;
    const long long n = m.v[0];
    if (n >= min_count) {
        const double dn = (double)n;
        const double mx = (double)m.v[1] / dn, my = (double)m.v[2] / dn, mz = (double)m.v[3] / dn;
        double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        a[0][0] = (double)m.v[4] / dn - mx * mx;
        a[0][1] = (double)m.v[5] / dn - mx * my;
        a[0][2] = (double)m.v[6] / dn - mx * mz;
        a[1][1] = (double)m.v[7] / dn - my * my;
        a[1][2] = (double)m.v[8] / dn - my * mz;
        a[2][2] = (double)m.v[9] / dn - mz * mz;
        a[1][0] = a[2][0] = a[2][1] = 0.0;              // (only the upper triangle is used)
        const double trace = (a[0][0] + a[1][1]) + a[2][2];
        if (trace > 0.0) {
            for (int sweep = 0; sweep < 24; ++sweep) {
                const double off = (fabs(a[0][1]) + fabs(a[0][2])) + fabs(a[1][2]);
                if (off <= 0x1p-70 * ((fabs(a[0][0]) + fabs(a[1][1])) + fabs(a[2][2]))) break;
                jacobi_rotate<0, 1>(a, v, sweep);
                jacobi_rotate<0, 2>(a, v, sweep);
                jacobi_rotate<1, 2>(a, v, sweep);
            }
            const double w0 = a[0][0], w1 = a[1][1], w2 = a[2][2];
            // the smallest eigenvalue's column, ties to the lowest column
            const int k = (w0 <= w1 && w0 <= w2) ? 0 : (w1 <= w2 ? 1 : 2);
            double nx = k == 0 ? v[0][0] : (k == 1 ? v[0][1] : v[0][2]);
            double ny = k == 0 ? v[1][0] : (k == 1 ? v[1][1] : v[1][2]);
            double nz = k == 0 ? v[2][0] : (k == 1 ? v[2][1] : v[2][2]);
            const double l0 = k == 0 ? w0 : (k == 1 ? w1 : w2);
            const double hi = fmax(w0, fmax(w1, w2));
            const double mid = fmax(fmin(w0, w1), fmin(fmax(w0, w1), w2));
            const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
            const double lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
            bool flip = lead < 0.0;
            if (toward != nullptr) {
                const double tx = (double)toward[0] - (double)qx, ty = (double)toward[1] - (double)qy,
                             tz = (double)toward[2] - (double)qz;
                const double s = flip ? -1.0 : 1.0;
                const double dot = ((s * nx) * tx + (s * ny) * ty) + (s * nz) * tz;
                if (dot < 0.0) flip = !flip;
            }
            if (flip) { nx = -nx; ny = -ny; nz = -nz; }
            out[0] = (float)nx; out[1] = (float)ny; out[2] = (float)nz;
            if (l0 > 0.0) var = (float)(l0 / ((l0 + mid) + hi));
        }
    }
    normals[row * 3] = out[0]; normals[row * 3 + 1] = out[1]; normals[row * 3 + 2] = out[2];
    if (variation != nullptr) variation[row] = var;
}

// ---- graph form --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void graph_normals_kernel(long long rows, int N, int M, int K, double Q, int min_count,
                                                            const float* __restrict__ database, const float* __restrict__ query,
                                                            const int* __restrict__ nn_index, const int* __restrict__ nn_count,
                                                            const float* __restrict__ toward, float* __restrict__ normals,
                                                            float* __restrict__ variation, int* __restrict__ count,
                                                            long long* __restrict__ moments,
                                                            unsigned long long* __restrict__ counters)
{
    __shared__ long long sums[10][kNrmRows];
    const long long base = (long long)blockIdx.x * kNrmRows;
    const int g = (int)threadIdx.x >> 4, l = (int)threadIdx.x & 15;
    long long skipped = 0;
    for (int r = 0; r < kNrmRows / 16; ++r) {
        const int slot = r * 16 + g;
        const long long row = base + slot;
        Moments m;
        moments_zero(m);
        if (row < rows) {
            const long long b = row / M;
            const float qx = query[row * 3], qy = query[row * 3 + 1], qz = query[row * 3 + 2];
            int cnt = nn_count[row];
            cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
            const int* list = nn_index + row * K;
            const float* cloud = database + b * N * 3;
            for (int j = l; j < cnt; j += 16) {
                const int i = list[j];
                bool ok = i >= 0 && i < N;
                if (ok) {
                    const float* p = cloud + (long long)i * 3;
                    ok = moments_add(m, p[0] - qx, p[1] - qy, p[2] - qz, Q);
                }
                if (!ok) ++skipped;
            }
        }
#pragma unroll
        for (int j = 0; j < 10; ++j) {
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) m.v[j] += __shfl_xor(m.v[j], off, 16);
        }
        if (l == 0) {
#pragma unroll
            for (int j = 0; j < 10; ++j) sums[j][slot] = m.v[j];
        }
    }
    __syncthreads();
    const long long row = base + threadIdx.x;
    if (row < rows) {
        Moments m;
#pragma unroll
        for (int j = 0; j < 10; ++j) m.v[j] = sums[j][threadIdx.x];
        normals_finish(m, query[row * 3], query[row * 3 + 1], query[row * 3 + 2],
                       toward != nullptr ? toward + (row / M) * 3 : nullptr, min_count, row, normals, variation, count, moments);
    }
    if (counters != nullptr) {
        skipped = wave_sum(skipped);
        if (lane_id() == 0 && skipped != 0) atomicAdd(&counters[0], (unsigned long long)skipped);
    }
}

// ---- ball form ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ball_normals_grid_kernel(long long V, float radius, float r2, double Q, int min_count,
                                                                const float* __restrict__ xyz, const float* __restrict__ toward,
                                                                const Nn1Hdr* __restrict__ hdr, const int* __restrict__ cellEnd,
                                                                const float4* __restrict__ pts, float* __restrict__ normals,
                                                                float* __restrict__ variation, int* __restrict__ count,
                                                                long long* __restrict__ moments)
{
    const Nn1Hdr H = *hdr;
    if (H.flag != 0 || H.ncell <= 0) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    Moments m;
    moments_zero(m);
    {   // a row with a non-finite coordinate is not in the grid: it has no neighbour
        const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
        if (!finite3(x, y, z)) normals_finish(m, x, y, z, toward, min_count, i, normals, variation, count, moments);
    }
    if (i >= H.nfin) return;
    const float4 me = pts[i];
    const long long id = __float_as_int(me.w);
    if (id < 0 || id >= V) return;
    const float qx = me.x, qy = me.y, qz = me.z;
    const int nx = H.nx, ny = H.ny, nz = H.nz;
    const float rr = radius * H.invh + kNrmCellSlack;
    // first and last cell of an axis that can hold a point of the ball (clamped as nn1_cell clamps)
    auto span = [&](float q, float lo, int n, int& c0, int& c1) {
        const float f = (q - lo) * H.invh;
        const float a = floorf(f - rr), b = floorf(f + rr);
        c0 = a >= 0.0f ? (a < (float)n ? (int)a : n - 1) : 0;
        c1 = b >= 0.0f ? (b < (float)n ? (int)b : n - 1) : 0;
    };
    int x0, x1, y0, y1, z0, z1;
    span(qx, H.minx, nx, x0, x1);
    span(qy, H.miny, ny, y0, y1);
    span(qz, H.minz, nz, z0, z1);
    for (int X = x0; X <= x1; ++X) {
        for (int Y = y0; Y <= y1; ++Y) {
            const int cb = (X * ny + Y) * nz;
            int p = cb + z0 > 0 ? cellEnd[cb + z0 - 1] : 0;
            int e = cellEnd[cb + z1];
            p = p < 0 ? 0 : p;
            e = e > V ? (int)V : e;
            for (; p < e; ++p) {
                const float4 c = pts[p];
                const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < r2) moments_add(m, dx, dy, dz, Q);
            }
        }
    }
    normals_finish(m, qx, qy, qz, toward, min_count, id, normals, variation, count, moments);
}

__global__ __launch_bounds__(256) void ball_normals_brute_kernel(long long V, float r2, double Q, int min_count,
                                                                 const float* __restrict__ xyz, const float* __restrict__ toward,
                                                                 const Nn1Hdr* __restrict__ hdr, float* __restrict__ normals,
                                                                 float* __restrict__ variation, int* __restrict__ count,
                                                                 long long* __restrict__ moments)
{
    __shared__ float4 tile[kNn1Tile];
    if (hdr->flag == 0) return;                        // uniform over the launch
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < V;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (live) { qx = xyz[i * 3]; qy = xyz[i * 3 + 1]; qz = xyz[i * 3 + 2]; }
    Moments m;
    moments_zero(m);
    for (long long base = 0; base < V; base += kNn1Tile) {
        const int cnt = V - base < kNn1Tile ? (int)(V - base) : kNn1Tile;
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) {
            const float* r = xyz + (base + t) * 3;
            tile[t] = make_float4(r[0], r[1], r[2], 0.0f);
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const float4 c = tile[t];
            const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;       // a non-finite coordinate gives inf or NaN: never below r2
            if (d2 < r2) moments_add(m, dx, dy, dz, Q);
        }
    }
    if (live) normals_finish(m, qx, qy, qz, toward, min_count, i, normals, variation, count, moments);
}

static int normals_check_common(const char* what, float radius, int min_count)
{
    SPH3D_REQUIRE(radius > 0.0f && radius < INFINITY, "%s: finite radius>0 required, got %g", what, (double)radius);
    SPH3D_REQUIRE(min_count >= 3, "%s: min_count>=3 required, got %d", what, min_count);
    return SPH3D_OK;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_graph_normals(int B, int N, int M, int K, float radius, int min_count, const float* database,
                                   const float* query, const int* nn_index, const int* nn_count, const float* toward,
                                   float* normals, float* variation, int* count, long long* moments, long long* counters,
                                   sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B >= 0 && N >= 0 && M >= 0, "graph_normals: B, N, M >= 0 required, got %d, %d, %d", B, N, M);
    SPH3D_REQUIRE(K > 0 && K <= 65535, "graph_normals: 0<K<2^16 required, got %d", K);
    if (int rc = normals_check_common("graph_normals", radius, min_count)) return rc;
    const long long rows = (long long)B * M;
    if (rows == 0) return SPH3D_OK;
    SPH3D_REQUIRE(query != nullptr && nn_index != nullptr && nn_count != nullptr && normals != nullptr && (N == 0 || database != nullptr),
                  "graph_normals: null pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(moments) & 7) == 0 && (reinterpret_cast<size_t>(counters) & 7) == 0,
                  "graph_normals: moments and counters must be 8-byte aligned");
    const long long blocks = (rows + kNrmRows - 1) / kNrmRows;
    SPH3D_REQUIRE(blocks <= 0x7fffffffll, "graph_normals: too many rows");
    const double Q = 262144.0 / (double)radius;
    hipLaunchKernelGGL(graph_normals_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), rows, N, M, K, Q, min_count,
                       database, query, nn_index, nn_count, toward, normals, variation, count, moments,
                       reinterpret_cast<unsigned long long*>(counters));
    return check_launch("sph3d_graph_normals");
}

extern "C" size_t sph3d_ball_normals_workspace(long long V)
{
    if (V <= 0 || V > kNrmMaxBall) return 0;
    return nn1_ws(nullptr, V).bytes;
}

extern "C" int sph3d_ball_normals(long long V, float radius, int min_count, const float* xyz, const float* toward, float* normals,
                                  float* variation, int* count, long long* moments, void* workspace, size_t workspace_bytes,
                                  sph3d_stream_t stream)
{
    SPH3D_REQUIRE(V >= 0 && V <= kNrmMaxBall, "ball_normals: 0<=V<=2^26 rows required, got %lld", V);
    if (int rc = normals_check_common("ball_normals", radius, min_count)) return rc;
    if (V == 0) return SPH3D_OK;
    SPH3D_REQUIRE(xyz != nullptr && normals != nullptr && count != nullptr, "ball_normals: null pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(moments) & 7) == 0, "ball_normals: moments must be 8-byte aligned");
    SPH3D_REQUIRE(workspace != nullptr && workspace_bytes >= sph3d_ball_normals_workspace(V) && (reinterpret_cast<size_t>(workspace) & 15) == 0,
                  "ball_normals: workspace of %zu bytes, 16-byte aligned, required (got %zu)", sph3d_ball_normals_workspace(V),
                  workspace_bytes);
    hipStream_t s = as_stream(stream);
    const Nn1Ws w = nn1_ws(workspace, V);
    const float r2 = radius * radius;
    const double Q = 262144.0 / (double)radius;
    const unsigned blocks = (unsigned)((V + 255) / 256);
    if (int rc = nn1_build(V, xyz, radius, true, w, s)) return rc;
    hipLaunchKernelGGL(ball_normals_grid_kernel, dim3(blocks), dim3(256), 0, s, V, radius, r2, Q, min_count, xyz, toward, w.hdr, w.cell,
                       w.pts, normals, variation, count, moments);
    hipLaunchKernelGGL(ball_normals_brute_kernel, dim3(blocks), dim3(256), 0, s, V, r2, Q, min_count, xyz, toward, w.hdr, normals,
                       variation, count, moments);
    return check_launch("sph3d_ball_normals");
}
