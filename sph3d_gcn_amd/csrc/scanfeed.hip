// scanfeed.hip — a ScanNet batch assembled on the device from a resident pool of parsed blocks (feed.hip's pool: rows [T,8] with
// xyz, rgb, label, inner): the per-step work of scannet_seg/train_scannet.py:112-127 and the three chained views of one evaluation
// draw (scannet_seg/evaluate_scannet_withoverlap.py:94-116,282-286) in ONE launch, one thread per output point and ALL views.
// The sample draws are feed.hip's, unchanged (feed_draws.hpp), so index, label and inner are a pure function of
// (seed, step, b, n, N), whatever the recipes, and equal sph3d_feed_assemble(..., augment = 0) bit for bit;
// harness/scannet.py:assemble_reference states everything in numpy, integer outputs bit for bit.
//
//   recipe[v][b]  objfeed.hip's bit mask (1 TURN, 2 TILT, 4 SCALE, 8 SHIFT, 16 JITTER, applied in that order, same purposes and
//                 counters), applied to the fp32 xyz of view v - 1; view -1 is the pool row.  The reference augments its float32
//                 batch in place, view after view: the coordinates stay in registers between views, which is the same arithmetic.
//   keys          view v takes its transform draws from feed_view_key(ck, v); view 0's key is ck, so a one-view launch draws
//                 exactly what sph3d_objfeed_assemble draws.
//   A mask of 0 copies the previous view bit for bit; rgb is copied into every view.
// Mapping: grid (ceil(N / 256), B): a workgroup serves ONE cloud, so per view the cloud's key, angles, matrix, scale and shift are
// wave-uniform (formed once per wave and pinned to scalar registers); only the sample walk, the row read and the jitter are per
// lane.  Traffic: the random 32-byte row is read once (two 16-byte loads) for all views; 24 bytes stored per point and view, 8
// (+ 4) per point — bound by the launch and the row reads.
#include "feed_draws.hpp"

namespace sph3d {

enum : int { kScanTurn = 1, kScanTilt = 2, kScanScale = 4, kScanShift = 8, kScanJitter = 16, kScanAll = 31, kScanMaxViews = 4 };

__global__ __launch_bounds__(256) void blockfeed_assemble_kernel(int B, int N, int P, long long T, const float* __restrict__ rows,
                                                                 const long long* __restrict__ offsets,
                                                                 const int* __restrict__ block_ids, unsigned long long seed,
                                                                 unsigned long long step, int views, const int* __restrict__ recipe,
                                                                 float* __restrict__ points, int* __restrict__ label,
                                                                 int* __restrict__ inner, int* __restrict__ index)
{
    const int b = blockIdx.y;                                          // (wave-uniform: one cloud per workgroup)
    const unsigned slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= (unsigned)N) return;
    const long long i = (long long)b * N + slot;
    const long long view_stride = (long long)B * N * 6;
    float2* out = reinterpret_cast<float2*>(points + i * 6);          // view v: out + v * view_stride / 2

    // the cloud's rows; a block id or an offset pair that does not describe rows of the pool reads nothing (index -1, zeros)
    long long lo;
    const unsigned n = feed_pool_rows(block_ids[b], P, T, offsets, lo);
    if (n == 0u) {
        for (int v = 0; v < views; ++v) {
            float2* o = out + v * (view_stride / 2);
            o[0] = o[1] = o[2] = make_float2(0.f, 0.f);
        }
        label[i] = 0;
        inner[i] = 0;
        if (index != nullptr) index[i] = -1;
        return;
    }
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    const unsigned r = feed_sample_row(ck, n, (unsigned)N, slot);

    const float4* src = reinterpret_cast<const float4*>(rows + (lo + (long long)r) * 8);
    const float4 a = src[0], c = src[1];            // x y z r | g b label inner
    float x = a.x, y = a.y, z = a.z;

    for (int v = 0; v < views; ++v) {
        const int mask = uniform(recipe[v * B + b]) & kScanAll;
        const unsigned long long vk = feed_view_key(ck, (unsigned)v);
        // row vector times matrix, as utils/data_util.py writes it; the cloud's numbers are the same in every lane
        if (mask & kScanTurn) {
            float st, ct;
            feed_turn(vk, st, ct);
            st = uniformf(st); ct = uniformf(ct);
            const float x1 = x * ct + y * st, y1 = y * ct - x * st;
            x = x1; y = y1;
        }
        if (mask & kScanTilt) {
            float m[9];
            feed_tilt(vk, m);
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = uniformf(m[k]);
            const float x1 = x * m[0] + y * m[3] + z * m[6];
            const float y1 = x * m[1] + y * m[4] + z * m[7];
            const float z1 = x * m[2] + y * m[5] + z * m[8];
            x = x1; y = y1; z = z1;
        }
        if (mask & kScanScale) {
            const float s = uniformf(0.8f + 0.45f * feed_uniform((unsigned)(feed_draw(vk, kFeedScale, 0u) >> 32)));
            x *= s; y *= s; z *= s;
        }
        if (mask & kScanShift) {
            x += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(vk, kFeedShift, 0u) >> 32)));
            y += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(vk, kFeedShift, 1u) >> 32)));
            z += uniformf(-0.1f + 0.2f * feed_uniform((unsigned)(feed_draw(vk, kFeedShift, 2u) >> 32)));
        }
        if (mask & kScanJitter) {
            float j0, j1, j2;
            feed_jitter(vk, slot, j0, j1, j2);
            x += j0; y += j1; z += j2;
        }
        float2* o = out + v * (view_stride / 2);
        o[0] = make_float2(x, y);
        o[1] = make_float2(z, a.w);
        o[2] = make_float2(c.x, c.y);
    }
    label[i] = (int)c.z;
    inner[i] = (int)c.w;
    if (index != nullptr) index[i] = (int)r;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_blockfeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows,
                                        const long long* offsets, const int* block_ids, unsigned long long seed,
                                        unsigned long long step, int views, const int* recipe, float* points, int* label, int* inner,
                                        int* index, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "blockfeed_assemble: batch 0<B<=65535 required, got %d", B);
    SPH3D_REQUIRE(num_point > 0, "blockfeed_assemble: num_point>0 required, got %d", num_point);
    SPH3D_REQUIRE(views >= 1 && views <= kScanMaxViews, "blockfeed_assemble: 1<=views<=%d required, got %d", (int)kScanMaxViews, views);
    SPH3D_REQUIRE(num_blocks > 0 && total_rows > 0, "blockfeed_assemble: empty pool (num_blocks=%d total_rows=%lld)", num_blocks,
                  total_rows);
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && block_ids != nullptr && recipe != nullptr,
                  "blockfeed_assemble: null input pointer");
    SPH3D_REQUIRE(points != nullptr && label != nullptr && inner != nullptr, "blockfeed_assemble: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rows) & 15) == 0 && (reinterpret_cast<size_t>(points) & 7) == 0,
                  "blockfeed_assemble: rows must be 16-byte and points 8-byte aligned");
    const long long total = (long long)views * B * num_point;
    SPH3D_REQUIRE(total <= 0x7fffffffll, "blockfeed_assemble: views*B*num_point=%lld too large", total);
    hipLaunchKernelGGL(blockfeed_assemble_kernel, dim3((unsigned)((num_point + 255) / 256), (unsigned)B), dim3(256), 0,
                       as_stream(stream), B, num_point, num_blocks, total_rows, rows, offsets, block_ids, seed, step, views, recipe,
                       points, label, inner, index);
    return check_launch("sph3d_blockfeed_assemble");
}
