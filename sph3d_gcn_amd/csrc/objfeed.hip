// objfeed.hip — a batch of the object datasets (ShapeNet parts, ModelNet40) assembled on the device from a resident pool of shapes:
// the per-step work of shapenet_seg/train_shapenet.py:121-152, modelnet40_cls/train_modelnet.py:95-115 and of the evaluation's
// two-pass draw (shapenet_seg/evaluate_shapenet.py:86-94,228-247) in ONE launch, one thread per output point.  The pool is
// feed.hip's: rows [T,8] with xyz in columns 0:3 and the label in column 6.  The sample draws are feed.hip's, unchanged
// (feed_draws.hpp), so `index` is a pure function of (seed, step, b, n, N) and does not depend on the recipe; harness/objfeed.py:
// assemble_reference states everything in numpy, integer outputs bit for bit.
//
//   recipe[b]   a bit mask, applied in the reference's order (utils/data_util.py:47-61,140-204):
//     1  TURN    . Rz(2 pi u)                                                      purpose 3, counter 0
//     2  TILT    . (Rz Ry Rx)(three clipped normal angles, sigma 0.06, clip 0.18)  purpose 4, counters 0, 1
//     4  SCALE   * (0.8 + 0.45 u)                                                  purpose 6, counter 0
//     8  SHIFT   + (-0.1 + 0.2 u) per axis                                         purpose 7, counters 0..2
//    16  JITTER  + clipped normal noise per point (sigma 0.01, clip 0.02)          purpose 5, counters 2 slot, 2 slot + 1
//   A mask of 0 copies xyz bit for bit.
// Mapping: grid (ceil(N / 256), B): a workgroup serves ONE cloud, so the cloud's key, its row range, the nine matrix entries, scale
// and shift are wave-uniform (formed once per wave and pinned to scalar registers); only the sample walk, the row read and the
// jitter are per lane.  Traffic: one 16-byte load (xyz) and one 4-byte load (label) of a random 32-byte row, 12 + 4 (+ 4) bytes
// stored per point — bound by the launch and the row reads.
#include "feed_draws.hpp"

namespace sph3d {

enum : int { kObjTurn = 1, kObjTilt = 2, kObjScale = 4, kObjShift = 8, kObjJitter = 16, kObjAll = 31 };

__global__ __launch_bounds__(256) void objfeed_assemble_kernel(int N, int P, long long T, const float* __restrict__ rows,
                                                               const long long* __restrict__ offsets, const int* __restrict__ shape_ids,
                                                               unsigned long long seed, unsigned long long step,
                                                               const int* __restrict__ recipe, float* __restrict__ points,
                                                               int* __restrict__ label, int* __restrict__ index)
{
    const int b = blockIdx.y;                                          // (wave-uniform: one cloud per workgroup)
    const unsigned slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= (unsigned)N) return;
    const long long i = (long long)b * N + slot;
    float* out = points + i * 3;

    // the cloud's rows; a shape id or an offset pair that does not describe rows of the pool reads nothing (index -1, zeros)
    long long lo;
    const unsigned n = feed_pool_rows(shape_ids[b], P, T, offsets, lo);
    if (n == 0u) {
        out[0] = out[1] = out[2] = 0.f;
        label[i] = 0;
        if (index != nullptr) index[i] = -1;
        return;
    }
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    const int mask = uniform(recipe[b]) & kObjAll;

    const unsigned r = feed_sample_row(ck, n, (unsigned)N, slot);
    const float* src = rows + (lo + (long long)r) * 8;
    const float4 a = *reinterpret_cast<const float4*>(src);           // x y z (column 3 is not used)
    const float lab = src[6];
    float x = a.x, y = a.y, z = a.z;

    // row vector times matrix, as utils/data_util.py writes it; the cloud's numbers are the same in every lane
    if (mask & kObjTurn) {
        float st, ct;
        feed_turn(ck, st, ct);
        st = uniformf(st); ct = uniformf(ct);
        const float x1 = x * ct + y * st, y1 = y * ct - x * st;
        x = x1; y = y1;
    }
    if (mask & kObjTilt) {
        float m[9];
        feed_tilt(ck, m);
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = uniformf(m[k]);
        const float x1 = x * m[0] + y * m[3] + z * m[6];
        const float y1 = x * m[1] + y * m[4] + z * m[7];
        const float z1 = x * m[2] + y * m[5] + z * m[8];
        x = x1; y = y1; z = z1;
    }
    if (mask & kObjScale) {
        const float s = uniformf(0.8f + 0.45f * feed_uniform((unsigned)(feed_draw(ck, kFeedScale, 0u) >> 32)));
        x *= s; y *= s; z *= s;
    }
    if (mask & kObjShift) {
        x += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 0u) >> 32)));
        y += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 1u) >> 32)));
        z += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 2u) >> 32)));
    }
    if (mask & kObjJitter) {
        float j0, j1, j2;
        feed_jitter(ck, slot, j0, j1, j2);
        x += j0; y += j1; z += j2;
    }
    out[0] = x; out[1] = y; out[2] = z;
    label[i] = (int)lab;
    if (index != nullptr) index[i] = (int)r;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_objfeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows,
                                      const long long* offsets, const int* shape_ids, unsigned long long seed,
                                      unsigned long long step, const int* recipe, float* points, int* label, int* index,
                                      sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "objfeed_assemble: batch 0<B<=65535 required, got %d", B);
    SPH3D_REQUIRE(num_point > 0, "objfeed_assemble: num_point>0 required, got %d", num_point);
    SPH3D_REQUIRE(num_blocks > 0 && total_rows > 0, "objfeed_assemble: empty pool (num_blocks=%d total_rows=%lld)", num_blocks,
                  total_rows);
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && shape_ids != nullptr && recipe != nullptr,
                  "objfeed_assemble: null input pointer");
    SPH3D_REQUIRE(points != nullptr && label != nullptr, "objfeed_assemble: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rows) & 15) == 0, "objfeed_assemble: rows must be 16-byte aligned");
    const long long total = (long long)B * num_point;
    SPH3D_REQUIRE(total <= 0x7fffffffll, "objfeed_assemble: B*num_point=%lld too large", total);
    hipLaunchKernelGGL(objfeed_assemble_kernel, dim3((unsigned)((num_point + 255) / 256), (unsigned)B), dim3(256), 0, as_stream(stream),
                       num_point, num_blocks, total_rows, rows, offsets, shape_ids, seed, step, recipe, points, label, index);
    return check_launch("sph3d_objfeed_assemble");
}
