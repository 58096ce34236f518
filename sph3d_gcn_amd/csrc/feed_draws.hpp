// feed_draws.hpp — the counter-based draws the feed kernels share (feed.hip, objfeed.hip, scanfeed.hip, cropfeed.hip); harness/feed.py states
// them in numpy.
//
//   cloud key   ck = mix(mix(mix(seed + G) + step + G) + b + G)           mix = the splitmix64 finaliser, G = 0x9e3779b97f4a7c15
//   view key    vk(ck, 0) = ck,  vk(ck, v) = mix(ck + v + G) for v >= 1   (harness/scannet.py: view_key)
//   a draw      w(purpose, counter) = mix(ck ^ (purpose << 56 | counter))    64 bits; "bits" = its high word
//   n >= N      slot j takes pi(j): a 6-round balanced Feistel network over 2 * ceil(k / 2) bits (2^k >= n > 2^(k-1)), walked
//               until it lands below n;  n < N: slot j takes mulhi(bits, n)
//   uniforms    (bits >> 8) * 2^-24; normals Box-Muller in fp32 with u1 = ((hi >> 8) + 1) * 2^-24 (never 0), u2 from the low word
#pragma once
#include "common.hpp"

namespace sph3d {

constexpr unsigned long long kFeedGold = 0x9e3779b97f4a7c15ull;
constexpr int kFeedRounds = 6;
enum : unsigned long long { kFeedPerm = 1, kFeedRepl = 2, kFeedTurn = 3, kFeedTilt = 4, kFeedJitter = 5, kFeedScale = 6,
                            kFeedShift = 7, kFeedIds = 8 /* + level, 0 <= level < 8: idsample.hip */,
                            kFeedDropout = 16 /* + layer, 0 <= layer < kFeedDropoutLayers: dropout.hip */,
                            // the augmentation stage (augment.hip; harness/augment.py states the counters)
                            kFeedAugGate = 32 /* counter = the gate's bit */, kFeedAugScale = 33 /* counter = axis */,
                            kFeedAugField = 34 /* + pass, 0 <= pass < 2; counter = the packed node */,
                            kFeedAugContrast = 36, kFeedAugCtrans = 37 /* counter = channel */,
                            kFeedAugCnoise = 38 /* counters 2 slot, 2 slot + 1 */,
                            kFeedCrop = 40 /* counter = the attempt: cropfeed.hip */ };
constexpr int kFeedDropoutLayers = 16;

__host__ __device__ __forceinline__ unsigned long long feed_mix(unsigned long long z)
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ unsigned long long feed_cloud_key(unsigned long long seed, unsigned long long step, unsigned b)
{
    return feed_mix(feed_mix(feed_mix(seed + kFeedGold) + step + kFeedGold) + b + kFeedGold);
}
// the key view v of a cloud takes its TRANSFORM draws from (scanfeed.hip: several views of one sample): view 0 is the cloud's own
// key, so a one-view launch draws what objfeed.hip draws; a later view is one more round over (ck, v).  The sample draws
// (kFeedPerm, kFeedRepl) always use ck itself.
__host__ __device__ __forceinline__ unsigned long long feed_view_key(unsigned long long ck, unsigned v)
{
    return v == 0u ? ck : feed_mix(ck + v + kFeedGold);
}
__device__ __forceinline__ unsigned long long feed_draw(unsigned long long ck, unsigned long long purpose, unsigned counter)
{
    return feed_mix(ck ^ (purpose << 56 | counter));
}
__device__ __forceinline__ unsigned feed_fmix32(unsigned x)
{
    x ^= x >> 16; x *= 0x85ebca6bu;
    x ^= x >> 13; x *= 0xc2b2ae35u;
    return x ^ (x >> 16);
}
__device__ __forceinline__ float feed_uniform(unsigned bits) { return (float)(bits >> 8) * 0x1p-24f; }

// two independent N(0,1) from one 64-bit draw
__device__ __forceinline__ void feed_normal_pair(unsigned long long w, float& z0, float& z1)
{
    const float u1 = (float)(((unsigned)(w >> 32) >> 8) + 1u) * 0x1p-24f;
    const float u2 = feed_uniform((unsigned)w);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    z0 = r * c;
    z1 = r * s;
}
__device__ __forceinline__ float feed_clip(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// the row of its cloud (n rows, n >= 1) that slot `slot` of a num_point sample takes: distinct rows for n >= num_point
__device__ __forceinline__ unsigned feed_sample_row(unsigned long long ck, unsigned n, unsigned num_point, unsigned slot)
{
    if (n < num_point) return __umulhi((unsigned)(feed_draw(ck, kFeedRepl, slot) >> 32), n);
    const int k = n > 1 ? 32 - __builtin_clz(n - 1) : 0;        // 2^k >= n > 2^(k-1)
    const int half = (k + 1) >> 1;
    const unsigned mask = (1u << half) - 1u;                       // (half <= 16)
    unsigned rk[kFeedRounds];
#pragma unroll
    for (int t = 0; t < kFeedRounds; ++t) rk[t] = (unsigned)(feed_draw(ck, kFeedPerm, (unsigned)t) >> 32);
    unsigned r = slot;
    do {
        unsigned L = r >> half, R = r & mask;
#pragma unroll
        for (int t = 0; t < kFeedRounds; ++t) {
            const unsigned f = feed_fmix32(R ^ rk[t]) & mask;
            const unsigned nl = R;
            R = L ^ f;
            L = nl;
        }
        r = (L << half) | R;
    } while (r >= n);
    return r;
}

// the rows of pool block `id`: -> n (0 for an id or an offset pair that does not describe rows of the pool), lo = its first row
__device__ __forceinline__ unsigned feed_pool_rows(int id, int P, long long T, const long long* __restrict__ offsets, long long& lo)
{
    long long n64 = 0;
    lo = 0;
    if (id >= 0 && id < P) {
        lo = offsets[id];
        n64 = offsets[id + 1] - lo;
    }
    return (n64 <= 0 || n64 > 0x7fffffffll || lo < 0 || lo + n64 > T) ? 0u : (unsigned)n64;
}

// The cloud-level numbers below are computed per lane: feed.hip's flat mapping lets one wave span two clouds, so only a caller
// whose workgroup serves one cloud (objfeed.hip) may pin what they return with uniformf().

// sin / cos of the turn: xyz . Rz(theta) = [[c,-s,0],[s,c,0],[0,0,1]] is  x' = x c + y s,  y' = y c - x s
__device__ __forceinline__ void feed_turn(unsigned long long ck, float& st, float& ct)
{
    sincosf(6.283185307179586f * feed_uniform((unsigned)(feed_draw(ck, kFeedTurn, 0u) >> 32)), &st, &ct);
}

// m = Rz(az) Ry(ay) Rx(ax), row-major, of three clipped normal angles (utils/data_util.py:140-163); xyz . m is the tilt
__device__ __forceinline__ void feed_tilt(unsigned long long ck, float (&m)[9])
{
    float ax, ay, az, unused;
    feed_normal_pair(feed_draw(ck, kFeedTilt, 0u), ax, ay);
    feed_normal_pair(feed_draw(ck, kFeedTilt, 1u), az, unused);
    ax = feed_clip(0.06f * ax, 0.18f); ay = feed_clip(0.06f * ay, 0.18f); az = feed_clip(0.06f * az, 0.18f);
    float sx, cx, sy, cy, sz, cz;
    sincosf(ax, &sx, &cx); sincosf(ay, &sy, &cy); sincosf(az, &sz, &cz);
    m[0] = cz * cy; m[1] = cz * sy * sx - sz * cx; m[2] = cz * sy * cx + sz * sx;
    m[3] = sz * cy; m[4] = sz * sy * sx + cz * cx; m[5] = sz * sy * cx - cz * sx;
    m[6] = -sy;     m[7] = cy * sx;                m[8] = cy * cx;
}

// the clipped normal noise of slot `slot`, one number per coordinate
__device__ __forceinline__ void feed_jitter(unsigned long long ck, unsigned slot, float& j0, float& j1, float& j2)
{
    float unused;
    feed_normal_pair(feed_draw(ck, kFeedJitter, 2u * slot), j0, j1);
    feed_normal_pair(feed_draw(ck, kFeedJitter, 2u * slot + 1u), j2, unused);
    j0 = feed_clip(0.01f * j0, 0.02f); j1 = feed_clip(0.01f * j1, 0.02f); j2 = feed_clip(0.01f * j2, 0.02f);
}

}  // namespace sph3d
