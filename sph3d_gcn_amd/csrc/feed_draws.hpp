// feed_draws.hpp — the counter-based draws the feed kernels share (feed.hip, objfeed.hip); harness/feed.py states them in numpy.
//
//   cloud key   ck = mix(mix(mix(seed + G) + step + G) + b + G)           mix = the splitmix64 finaliser, G = 0x9e3779b97f4a7c15
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
                            kFeedShift = 7 };

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

}  // namespace sph3d
