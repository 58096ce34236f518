// cropfeed.hip — a batch of training crops cut out of whole scenes on the device, in ONE launch: what the later indoor-segmentation
// recipes do per step (keep the room resident, crop around a random point) in place of the offline block writer.  The pool is a
// set of COLUMN-SORTED scenes (harness/cropfeed.py: column_sort_reference; include/sph3d.h: sph3d_cropfeed_assemble): a scene's rows
// are sorted by col = ix n_y + iy of an xy cell grid, so the rows of cells (ix, y0 .. y1) are the contiguous range
// [col_start[ix n_y + y0], col_start[ix n_y + y1 + 1]) — a "strip" — and a square window of cells is at most 2 outer_half + 1 strips.
// harness/cropfeed.py: crop_reference states everything in numpy; the integer outputs equal it bit for bit.
//
//   attempt a   centre row = mulhi(hi32(draw(ck, kFeedCrop, a)), n); (cx, cy) = divmod(column[centre], n_y); the window is
//               ix in [max(0, cx - outer_half), min(n_x - 1, cx + outer_half)], iy likewise; T_a = the sum of its strips' lengths
//   the choice  the first attempt with T_a >= min_points, else the largest T_a (lowest a on a tie)
//   slot j      member t = feed_sample_row(ck, T, N, j) of the chosen window (the strips in ascending ix, rows in stored order);
//               inner iff |ix - cx| <= inner_half and |iy - cy| <= inner_half of the row's own column
//   augment     feed.hip's rule by thirds of B, feed.hip's arithmetic
// Mapping: grid (ceil(N / 256), B), a workgroup of 4 waves serves one cloud and 256 of its slots.
//   Phase A (integers only) is done by EVERY WAVE on its own — no workgroup and no wave waits for another to learn the choice: per
//   attempt the lanes load the two col_start words of their strips (4 chunks of 64 cover the at most 255 strips), an inclusive wave
//   scan with a carry gives the strips' prefix sums and T_a.  Wave w keeps chunk w's sums of the best attempt so far and, after
//   the choice, writes them to LDS: prefix [257] and the strips' first rows [256].  One barrier.
//   Phase B, one thread per slot: the sample, a binary search of the member in the LDS prefix (8 steps), two 16-byte loads of the
//   row and one 4-byte load of its column, the transform, feed.hip's stores.
// No atomics, no workspace, nothing allocated; every output bit is a pure function of the arguments.
// Robustness: a scene_tab row is checked against the pool before an address is formed; a strip whose two words are not
// 0 <= first <= end <= n counts as empty and a column word outside the grid is clamped, so a damaged pool yields wrong crops or
// none (crop -1), never a read outside rows / column / col_start.
#include "feed_draws.hpp"

namespace sph3d {

constexpr int kCropThreads = 256;
constexpr int kCropChunks = kCropThreads / kWave;        // 4 chunks of 64 strips: 2 outer_half + 1 <= 256
constexpr int kCropMaxAttempts = 8;

__global__ __launch_bounds__(kCropThreads) void cropfeed_assemble_kernel(
    int B, int N, int S, long long T, long long C, const float* __restrict__ rows, const int* __restrict__ column,
    const int* __restrict__ col_start, const long long* __restrict__ scene_tab, const int* __restrict__ scene_ids,
    unsigned long long seed, unsigned long long step, int augment, int inner_half, int outer_half, int attempts, int min_points,
    float* __restrict__ points, int* __restrict__ label, int* __restrict__ inner, int* __restrict__ index, int* __restrict__ crop)
{
    __shared__ unsigned s_prefix[kCropThreads + 1];      // s_prefix[s] = members before strip s; [256] = T
    __shared__ unsigned s_first[kCropThreads];           // the first row (within the scene) of strip s

    const int b = blockIdx.y;                            // (wave-uniform: one cloud per workgroup)
    const unsigned slot = blockIdx.x * (unsigned)kCropThreads + threadIdx.x;
    const bool live = slot < (unsigned)N;
    const long long i = (long long)b * N + slot;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);

    // ---- the scene: a scene id or a table row that does not describe rows of the pool reads nothing
    const int sid = scene_ids[b];
    long long row0 = 0, cs0 = 0, nx = 0, ny = 0, n64 = 0;
    if (sid >= 0 && sid < S) {
        const long long* t = scene_tab + (long long)sid * 5;
        row0 = t[0]; cs0 = t[1]; nx = t[2]; ny = t[3]; n64 = t[4];
    }
    bool ok = n64 > 0 && n64 <= 0x7fffffffll && row0 >= 0 && row0 + n64 <= T && nx > 0 && ny > 0 && nx <= 0x7fffffffll &&
              ny <= 0x7fffffffll && nx * ny <= 0x7fffffffll && cs0 >= 0 && cs0 + nx * ny + 1 <= C;

    // ---- Phase A: every wave on its own, all to the same result
    const unsigned long long ck = feed_cloud_key(seed, step, (unsigned)b);
    unsigned best = 0u, my_prefix = 0u, my_first = 0u;
    int best_a = -1, best_row = 0, best_cx = 0, best_cy = 0;
    if (ok) {
        const unsigned n = (unsigned)n64;
        const int inx = (int)nx, iny = (int)ny;
        const int* cs = col_start + cs0;
        for (int a = 0; a < attempts; ++a) {
            const unsigned centre = __umulhi((unsigned)(feed_draw(ck, kFeedCrop, (unsigned)a) >> 32), n);
            int col = column[row0 + centre];
            col = min(max(col, 0), inx * iny - 1);
            const int cx = col / iny, cy = col - cx * iny;
            const int x0 = max(0, cx - outer_half), x1 = min(inx - 1, cx + outer_half);
            const int y0 = max(0, cy - outer_half), y1 = min(iny - 1, cy + outer_half);
            const int W = x1 - x0 + 1;                   // <= 2 outer_half + 1 <= 255
            unsigned carry = 0u, keep_prefix = 0u, keep_first = 0u;
#pragma unroll
            for (int c = 0; c < kCropChunks; ++c) {
                const int s = c * kWave + lane;
                unsigned first = 0u, len = 0u;
                if (s < W) {
                    const long long at = (long long)(x0 + s) * iny;
                    const int f = cs[at + y0], e = cs[at + y1 + 1];
                    if (f >= 0 && f <= e && (unsigned)e <= n) { first = (unsigned)f; len = (unsigned)(e - f); }
                }
                unsigned incl = len;
#pragma unroll
                for (int o = 1; o < kWave; o <<= 1) {
                    const unsigned v = __shfl_up(incl, o);
                    if (lane >= o) incl += v;
                }
                incl += carry;
                carry = __shfl(incl, kWave - 1);
                if (c == wave) { keep_prefix = incl; keep_first = first; }
            }
            if (carry > best) {                          // (strictly: the lowest attempt wins a tie)
                best = carry; best_a = a; best_row = (int)centre; best_cx = cx; best_cy = cy;
                my_prefix = keep_prefix; my_first = keep_first;
            }
            if (carry >= (unsigned)min_points) break;    // (then carry > every earlier T_a, so it is `best`)
        }
        ok = best > 0u && best <= n;
    }
    if (!ok) {                                           // (workgroup-uniform: nobody waits at the barrier below)
        if (live) {
            float2* out = reinterpret_cast<float2*>(points + i * 6);
            out[0] = out[1] = out[2] = make_float2(0.f, 0.f);
            label[i] = 0;
            inner[i] = 0;
            if (index != nullptr) index[i] = -1;
        }
        if (blockIdx.x == 0 && threadIdx.x < 4) crop[b * 4 + threadIdx.x] = -1;
        return;
    }
    if (threadIdx.x == 0) s_prefix[0] = 0u;
    s_prefix[threadIdx.x + 1] = my_prefix;               // (thread wave * 64 + lane holds strip wave * 64 + lane)
    s_first[threadIdx.x] = my_first;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        crop[b * 4 + 0] = sid; crop[b * 4 + 1] = best_row; crop[b * 4 + 2] = best_a; crop[b * 4 + 3] = (int)best;
    }
    __syncthreads();
    if (!live) return;

    // ---- Phase B: one thread per slot
    const unsigned t = feed_sample_row(ck, best, (unsigned)N, slot);        // member t of the crop, t < best = s_prefix[256]
    int s = 0;
#pragma unroll
    for (int w = kCropThreads / 2; w > 0; w >>= 1)
        if (s_prefix[s + w] <= t) s += w;                // the last strip with s_prefix[s] <= t: it holds member t
    const unsigned r = min(s_first[s] + (t - s_prefix[s]), (unsigned)n64 - 1u);        // (the min: a damaged pool only)

    const float4* src = reinterpret_cast<const float4*>(rows + (row0 + (long long)r) * 8);
    const float4 a = src[0], c = src[1];                 // x y z r | g b label (unused)
    const int iny = (int)ny;
    const int col = column[row0 + r];
    const int ix = col / iny, iy = col - ix * iny;
    const int in = (abs(ix - best_cx) <= inner_half && abs(iy - best_cy) <= inner_half) ? 1 : 0;

    float x = a.x, y = a.y, z = a.z;
    const int third = B / 3;
    if (augment && b < third) {
        // xyz . Rz(theta) . (Rz(az) Ry(ay) Rx(ax)), as feed.hip writes it
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
    float2* out = reinterpret_cast<float2*>(points + i * 6);
    out[0] = make_float2(x, y);
    out[1] = make_float2(z, a.w);
    out[2] = make_float2(c.x, c.y);
    label[i] = (int)c.z;
    inner[i] = in;
    if (index != nullptr) index[i] = (int)r;
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_cropfeed_assemble(int B, int num_point, int num_scenes, long long total_rows, long long total_cols,
                                       const float* rows, const int* column, const int* col_start, const long long* scene_tab,
                                       const int* scene_ids, unsigned long long seed, unsigned long long step, int augment,
                                       int inner_half, int outer_half, int attempts, int min_points, float* points, int* label,
                                       int* inner, int* index, int* crop, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B > 0 && B <= 65535, "cropfeed_assemble: batch 0<B<=65535 required, got %d", B);
    SPH3D_REQUIRE(num_point > 0, "cropfeed_assemble: num_point>0 required, got %d", num_point);
    SPH3D_REQUIRE(num_scenes > 0 && total_rows > 0 && total_cols > 0,
                  "cropfeed_assemble: empty pool (num_scenes=%d total_rows=%lld total_cols=%lld)", num_scenes, total_rows, total_cols);
    SPH3D_REQUIRE(augment == 0 || augment == 1, "cropfeed_assemble: augment must be 0 or 1, got %d", augment);
    SPH3D_REQUIRE(outer_half >= 0 && 2 * (long long)outer_half + 1 <= kCropThreads,
                  "cropfeed_assemble: 2*outer_half+1 <= %d required, got outer_half=%d", kCropThreads, outer_half);
    SPH3D_REQUIRE(inner_half >= 0 && inner_half <= outer_half, "cropfeed_assemble: 0 <= inner_half <= outer_half required, got %d, %d",
                  inner_half, outer_half);
    SPH3D_REQUIRE(attempts >= 1 && attempts <= kCropMaxAttempts, "cropfeed_assemble: 1 <= attempts <= %d required, got %d",
                  kCropMaxAttempts, attempts);
    SPH3D_REQUIRE(min_points >= 1, "cropfeed_assemble: min_points>=1 required, got %d", min_points);
    SPH3D_REQUIRE(rows != nullptr && column != nullptr && col_start != nullptr && scene_tab != nullptr && scene_ids != nullptr,
                  "cropfeed_assemble: null input pointer");
    SPH3D_REQUIRE(points != nullptr && label != nullptr && inner != nullptr && crop != nullptr,
                  "cropfeed_assemble: null output pointer");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(rows) & 15) == 0 && (reinterpret_cast<size_t>(points) & 7) == 0,
                  "cropfeed_assemble: rows must be 16-byte and points 8-byte aligned");
    SPH3D_REQUIRE((reinterpret_cast<size_t>(scene_tab) & 7) == 0, "cropfeed_assemble: scene_tab must be 8-byte aligned");
    SPH3D_REQUIRE(((reinterpret_cast<size_t>(column) | reinterpret_cast<size_t>(col_start) | reinterpret_cast<size_t>(scene_ids) |
                    reinterpret_cast<size_t>(label) | reinterpret_cast<size_t>(inner) | reinterpret_cast<size_t>(index) |
                    reinterpret_cast<size_t>(crop)) & 3) == 0,
                  "cropfeed_assemble: int32 arrays must be 4-byte aligned");
    const long long total = (long long)B * num_point;
    SPH3D_REQUIRE(total <= 0x7fffffffll, "cropfeed_assemble: B*num_point=%lld too large", total);
    hipLaunchKernelGGL(cropfeed_assemble_kernel, dim3((unsigned)((num_point + kCropThreads - 1) / kCropThreads), (unsigned)B),
                       dim3(kCropThreads), 0, as_stream(stream), B, num_point, num_scenes, total_rows, total_cols, rows, column,
                       col_start, scene_tab, scene_ids, seed, step, augment, inner_half, outer_half, attempts, min_points, points,
                       label, inner, index, crop);
    return check_launch("sph3d_cropfeed_assemble");
}
