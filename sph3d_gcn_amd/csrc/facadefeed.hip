// facadefeed.hip — a batch of RueMonge2014 facade clouds assembled on the device from a resident pool of facade splits: the per-step
// work of ruemonge2014_seg/train_ruemonge2014.py:98-138 and of the evaluation's augmented pass
// (ruemonge2014_seg/evaluate_ruemonge2014.py:180-305) in ONE launch, one thread per output point.  The pool is feed.hip's — rows
// [T,8]: xyz, rgb, label, inner — plus normals [T,4]: nx ny nz 0, so that a row's normal is one aligned 16-byte load.  The sample
// draws are feed.hip's, unchanged (feed_draws.hpp), so `index` is a pure function of (seed, step, b, n, N) and does not depend on
// the recipe; the recipe's bits, purposes and counters are objfeed.hip's, unchanged.  harness/facadefeed.py: assemble_reference
// and apply_reference state everything in numpy, integer outputs and every copied channel bit for bit.
//
//   recipe[b]   TURN 1 and TILT 2 multiply xyz AND the normal by the same matrix entries (utils/data_util.py:64-105);
//               SCALE 4, SHIFT 8 and JITTER 16 touch xyz only; rgb and the label are always copied.
//   A mask of 0 copies all nine channels bit for bit; a mask without TURN and TILT copies the normal bit for bit.
// Output channels are the reference's (train_ruemonge2014.py:159): xyz, normal, rgb.
// Mapping: grid (ceil(N / 256), B): a workgroup serves ONE cloud, so the cloud's key, its row range, the matrix entries, scale and
// shift are wave-uniform (formed once per wave and pinned to scalar registers); the sample walk, the row reads and the jitter are
// per lane.  Traffic per point: 48 bytes read (two 16-byte loads of a random 32-byte row, one of its 16-byte normal), 36 + 4 (+ 4)
// bytes stored; the nine floats of a point are consecutive, 4-byte aligned, and leave the lane as three 12-byte stores, not
// through LDS (DESIGN 4.14 has the ISA).
#include "feed_draws.hpp"

namespace sph3d {

enum : int { kFacTurn = 1, kFacTilt = 2, kFacScale = 4, kFacShift = 8, kFacJitter = 16, kFacAll = 31 };

__global__ __launch_bounds__(256) void facadefeed_assemble_kernel(int N, int P, long long T, const float* __restrict__ rows,
                                                                  const float* __restrict__ normals,
                                                                  const long long* __restrict__ offsets, const int* __restrict__ ids,
                                                                  unsigned long long seed, unsigned long long step,
                                                                  const int* __restrict__ recipe, float* __restrict__ points,
                                                                  int* __restrict__ label, int* __restrict__ index)
{
    const int b = blockIdx.y;                                          // (wave-uniform: one cloud per workgroup)
    const unsigned slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= (unsigned)N) return;
    const long long i = (long long)b * N + slot;
    float* out = points + i * 9;

    // the cloud's rows; an id or an offset pair that does not describe rows of the pool reads nothing (index -1, zeros)
    long long lo;
    const unsigned n = feed_pool_rows(ids[b], P, T, offsets, lo);
    if (n == 0u) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = 0.f;
        label[i] = 0;
        if (index != nullptr) index[i] = -1;
        return;
    }
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    const int mask = uniform(recipe[b]) & kFacAll;

    const unsigned r = feed_sample_row(ck, n, (unsigned)N, slot);
    const long long row = lo + (long long)r;
    const float4 a = *reinterpret_cast<const float4*>(rows + row * 8);         // x y z red
    const float4 c = *reinterpret_cast<const float4*>(rows + row * 8 + 4);     // green blue label inner
    const float4 nm = *reinterpret_cast<const float4*>(normals + row * 4);     // nx ny nz (column 3 is padding, never written out)
    float x = a.x, y = a.y, z = a.z;
    float nx = nm.x, ny = nm.y, nz = nm.z;

    // row vector times matrix, as utils/data_util.py writes it; the cloud's numbers are the same in every lane
    if (mask & kFacTurn) {
        float st, ct;
        feed_turn(ck, st, ct);
        st = uniformf(st); ct = uniformf(ct);
        const float x1 = x * ct + y * st, y1 = y * ct - x * st;
        const float nx1 = nx * ct + ny * st, ny1 = ny * ct - nx * st;
        x = x1; y = y1;
        nx = nx1; ny = ny1;
    }
    if (mask & kFacTilt) {
        float m[9];
        feed_tilt(ck, m);
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = uniformf(m[k]);
        const float x1 = x * m[0] + y * m[3] + z * m[6];
        const float y1 = x * m[1] + y * m[4] + z * m[7];
        const float z1 = x * m[2] + y * m[5] + z * m[8];
        const float nx1 = nx * m[0] + ny * m[3] + nz * m[6];
        const float ny1 = nx * m[1] + ny * m[4] + nz * m[7];
        const float nz1 = nx * m[2] + ny * m[5] + nz * m[8];
        x = x1; y = y1; z = z1;
        nx = nx1; ny = ny1; nz = nz1;
    }
    if (mask & kFacScale) {
        const float s = uniformf(0.8f + 0.45f * feed_uniform((unsigned)(feed_draw(ck, kFeedScale, 0u) >> 32)));
        x *= s; y *= s; z *= s;
    }
    if (mask & kFacShift) {
        x += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 0u) >> 32)));
        y += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 1u) >> 32)));
        z += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(ck, kFeedShift, 2u) >> 32)));
    }
    if (mask & kFacJitter) {
        float j0, j1, j2;
        feed_jitter(ck, slot, j0, j1, j2);
        x += j0; y += j1; z += j2;
    }
    out[0] = x; out[1] = y; out[2] = z;
    out[3] = nx; out[4] = ny; out[5] = nz;
    out[6] = a.w; out[7] = c.x; out[8] = c.y;
    label[i] = (int)c.z;
    if (index != nullptr) index[i] = (int)r;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_facadefeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows,
                                         const float* normals, const long long* offsets, const int* ids, unsigned long long seed,
                                         unsigned long long step, const int* recipe, float* points, int* label, int* index,
                                         sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "facadefeed_assemble: batch 0<B<=65535 required, got %d", B);
    SPH3D_REQUIRE(num_point > 0, "facadefeed_assemble: num_point>0 required, got %d", num_point);
    SPH3D_REQUIRE(num_blocks > 0 && total_rows > 0, "facadefeed_assemble: empty pool (num_blocks=%d total_rows=%lld)", num_blocks,
                  total_rows);
    SPH3D_REQUIRE(rows != nullptr && normals != nullptr && offsets != nullptr && ids != nullptr && recipe != nullptr,
                  "facadefeed_assemble: null input pointer");
    SPH3D_REQUIRE(points != nullptr && label != nullptr, "facadefeed_assemble: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rows) & 15) == 0, "facadefeed_assemble: rows must be 16-byte aligned");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(normals) & 15) == 0, "facadefeed_assemble: normals must be 16-byte aligned");
    const long long total = (long long)B * num_point;
    SPH3D_REQUIRE(total <= 0x7fffffffll, "facadefeed_assemble: B*num_point=%lld too large", total);
    hipLaunchKernelGGL(facadefeed_assemble_kernel, dim3((unsigned)((num_point + 255) / 256), (unsigned)B), dim3(256), 0,
                       as_stream(stream), num_point, num_blocks, total_rows, rows, normals, offsets, ids, seed, step, recipe, points,
                       label, index);
    return check_launch("sph3d_facadefeed_assemble");
}
