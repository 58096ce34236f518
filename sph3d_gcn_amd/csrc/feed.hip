// feed.hip — a training batch assembled on the device from a resident pool of parsed S3DIS blocks: the per-step work of the
// reference's input loop (train_s3dis.py:114-142,343-347; host statement: harness/blockio.py sample_points / augment_batch) in ONE
// launch, one thread per output point.  The draws are counter-based — pure functions of (seed, step, cloud, slot, purpose) — and
// harness/feed.py:assemble_reference states them in numpy; the integer outputs equal that statement bit for bit.
//
//   cloud key   ck = mix(mix(mix(seed + G) + step + G) + b + G)           mix = the splitmix64 finaliser, G = 0x9e3779b97f4a7c15
//   a draw      w(purpose, counter) = mix(ck ^ (purpose << 56 | counter))    64 bits; "bits" = its high word
//   n >= N      slot j takes pi(j): a 6-round balanced Feistel network over 2 * ceil(k / 2) bits (2^k >= n > 2^(k-1)), walked
//               until it lands below n (a bijection of the domain, so the walk returns to [0, n): 2^(2 ceil(k/2)) < 4 n,
//               fewer than 4 steps expected).  N distinct rows in an exchangeable order, no sort, no cross-thread traffic.
//   n <  N      slot j takes mulhi(bits, n)
//   augment     third = B / 3: clouds [0, third) are turned by Rz(theta) * (Rz Ry Rx)(three clipped normal angles), clouds
//               [third, 2 third) get clipped normal noise per coordinate.  Uniforms are (bits >> 8) * 2^-24, normals Box-Muller
//               in fp32 with u1 = ((hi >> 8) + 1) * 2^-24 (never 0) and u2 from the low word of the same draw.
// Traffic: two 16-byte loads of a random 32-byte row and 36 bytes of stores per point — bound by the launch and the row reads.
#include "feed_draws.hpp"

namespace sph3d {

__global__ __launch_bounds__(256) void feed_assemble_kernel(int B, int N, int P, long long T, const float* __restrict__ rows,
                                                            const long long* __restrict__ offsets, const int* __restrict__ block_ids,
                                                            unsigned long long seed, unsigned long long step, int augment,
                                                            float* __restrict__ points, int* __restrict__ label,
                                                            int* __restrict__ inner, int* __restrict__ index)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * N) return;
    const int b = (int)(i / N);
    const unsigned slot = (unsigned)(i - (long long)b * N);
    float2* out = reinterpret_cast<float2*>(points + i * 6);

    // the cloud's rows; a block id or an offset pair that does not describe rows of the pool reads nothing (index -1, zeros)
    long long lo;
    const unsigned n = feed_pool_rows(block_ids[b], P, T, offsets, lo);
    if (n == 0u) {
        out[0] = out[1] = out[2] = make_float2(0.f, 0.f);
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
    const int third = B / 3;
    if (augment && b < third) {
        // xyz . Rz(theta) . (Rz(az) Ry(ay) Rx(ax)), row vector times matrix (utils/data_util.py:47-61,140-163); the eleven
        // numbers are the same for every point of the cloud: each thread recomputes them (4 sincos)
        float st, ct, m[9];
        feed_turn(ck, st, ct);
        feed_tilt(ck, m);
        const float x1 = x * ct + y * st, y1 = y * ct - x * st;
        x = x1 * m[0] + y1 * m[3] + a.z * m[6];
        y = x1 * m[1] + y1 * m[4] + a.z * m[7];
        z = x1 * m[2] + y1 * m[5] + a.z * m[8];
    } else if (augment && b < 2 * third) {
        float j0, j1, j2;
        feed_jitter(ck, slot, j0, j1, j2);
        x += j0; y += j1; z += j2;
    }
    out[0] = make_float2(x, y);
    out[1] = make_float2(z, a.w);
    out[2] = make_float2(c.x, c.y);
    label[i] = (int)c.z;
    inner[i] = (int)c.w;
    if (index != nullptr) index[i] = (int)r;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_feed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows,
                                   const long long* offsets, const int* block_ids, unsigned long long seed, unsigned long long step,
                                   int augment, float* points, int* label, int* inner, int* index, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0, "feed_assemble: batch B>0 required, got %d", B);
    SPH3D_REQUIRE(num_point > 0, "feed_assemble: num_point>0 required, got %d", num_point);
    SPH3D_REQUIRE(num_blocks > 0 && total_rows > 0, "feed_assemble: empty pool (num_blocks=%d total_rows=%lld)", num_blocks, total_rows);
    SPH3D_REQUIRE(augment == 0 || augment == 1, "feed_assemble: augment must be 0 or 1, got %d", augment);
    SPH3D_REQUIRE(rows != nullptr && offsets != nullptr && block_ids != nullptr, "feed_assemble: null input pointer");
    SPH3D_REQUIRE(points != nullptr && label != nullptr && inner != nullptr, "feed_assemble: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rows) & 15) == 0 && (reinterpret_cast<size_t>(points) & 7) == 0,
                  "feed_assemble: rows must be 16-byte and points 8-byte aligned");
    const long long total = (long long)B * num_point;
    SPH3D_REQUIRE(total <= 0x7fffffffll, "feed_assemble: B*num_point=%lld too large", total);
    hipLaunchKernelGGL(feed_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), B, num_point,
                       num_blocks, total_rows, rows, offsets, block_ids, seed, step, augment, points, label, inner, index);
    return check_launch("sph3d_feed_assemble");
}
