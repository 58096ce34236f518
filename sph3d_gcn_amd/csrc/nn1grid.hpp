// nn1grid.hpp — the counting-sorted cell grid of scene.hip (sph3d_nn1's build) as its other users see it: the header the build
// leaves in the workspace, the workspace's layout, the cell coordinate of a value, and the host call that queues the build.
// The build's kernels stay in scene.hip; normals.hip walks the grid they leave.
#pragma once
#include "common.hpp"

namespace sph3d {

constexpr int kNn1MinGrid = 64;             // fewer finite reference points: brute force
constexpr int kNn1MinCells = 64;
constexpr int kNn1MaxCells = 1 << 21;       // 8 MB of cell ends
constexpr int kNn1MaxDim = 1024;            // cells per axis: bounds the rounding of the cell coordinate (scene.hip, head comment)
constexpr int kNn1Tile = 1024;              // reference points per LDS tile of the brute-force kernels
// (a point or a query lands in the wrong cell by at most 3 * 2^-24 * kNn1MaxDim = 1.8e-4 cells through the rounding of
// (v - lo) * invh: every walk of the grid allows for it)

struct Nn1Hdr {
    unsigned lo[3], hi[3];                  // bounding box as ordered integers
    int nfin, flag;                         // finite reference points; 1: the grid cannot index this cloud
    float minx, miny, minz, invh, h;
    int nx, ny, nz, ncell;
};
constexpr size_t kNn1HdrBytes = 256;

static inline long long nn1_cell_cap(long long V)
{
    const long long c = V / 2;
    return c < kNn1MinCells ? kNn1MinCells : (c > kNn1MaxCells ? kNn1MaxCells : c);
}

// the workspace of a build over V reference points: header, cell ends (cell[c] = END of cell c after the build), sorted points
// (x, y, z, index bits) in cell order, cells z-fastest
struct Nn1Ws {
    Nn1Hdr* hdr; int* cell; float4* pts; size_t cellBytes, bytes;
};
static inline Nn1Ws nn1_ws(void* workspace, long long V)
{
    Nn1Ws w;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    w.cellBytes = (((size_t)nn1_cell_cap(V) + 1) * sizeof(int) + 255) & ~(size_t)255;
    w.hdr = reinterpret_cast<Nn1Hdr*>(ws);
    w.cell = reinterpret_cast<int*>(ws + kNn1HdrBytes);
    w.pts = reinterpret_cast<float4*>(ws + kNn1HdrBytes + w.cellBytes);
    w.bytes = kNn1HdrBytes + w.cellBytes + (size_t)V * sizeof(float4);
    return w;
}

// scene.hip: queues the header's reset and, with `grid`, the build (zero fill, bounding box, shape, count, scan, fill) on
// `stream`.  min_h: the cell edge is not refined below it (0: none — sph3d_nn1's own grid); a cloud whose longest extent is
// smaller keeps that extent as its edge.  -> SPH3D_OK or the zero fill's error; the caller ends with check_launch()
int nn1_build(long long V, const float* ref_xyz, float min_h, bool grid, const Nn1Ws& w, hipStream_t stream);

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}
// cell coordinate along one axis, clamped into the grid (a query outside the box takes the nearest cell)
__device__ __forceinline__ int nn1_cell(float v, float lo, float invh, int n)
{
    const float t = floorf((v - lo) * invh);
    return t >= 0.0f ? (t < (float)n ? (int)t : n - 1) : 0;
}
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

}  // namespace sph3d
