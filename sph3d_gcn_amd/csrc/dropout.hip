// dropout.hip — keyed inverted dropout (tf.layers.dropout of the classifiers' fully connected layers, models/SPH3D_modelnet.py:99,102)
// as a pure function of (seed, step, row, layer, element): the mask is a counter-based draw of feed_draws.hpp like every other
// draw of a training run, so a resumed run and a second run from the seed drop the same elements.  harness/dropout.py states it
// in numpy; the device result equals the statement bit for bit.
//     ck = feed_cloud_key(seed, step, row0 + b)          row b of x [B, L]
//     w  = feed_draw(ck, kFeedDropout + layer, i)        element i < L of the row
//     y  = (w >> 32) >= thr ? x * scale : +0.0f          thr = min(2^32 - 1, ceil(rate 2^32)), scale = float32(1 / (1 - rate)): the host's
// The gradient is the same call on grad_output.  One streaming pass, 16-byte lanes.
#include "common.hpp"
#include "feed_draws.hpp"

namespace sph3d {

__global__ __launch_bounds__(256) void dropout_keyed_kernel(long long n4, long long n, long long L, const float* __restrict__ x,
                                                            float* __restrict__ y, unsigned long long seed, unsigned long long step,
                                                            unsigned row0, unsigned long long purpose, unsigned thr, float scale)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    auto one = [&](unsigned long long ck, unsigned i, float v) {
        return (unsigned)(feed_draw(ck, purpose, i) >> 32) >= thr ? v * scale : 0.f;       // a dropped slot is +0.0 whatever x holds
    };
    if (t < n4) {
        const float4 X = reinterpret_cast<const float4*>(x)[t];
        const float xs[4] = {X.x, X.y, X.z, X.w};
        float ys[4];
        long long b = (t * 4) / L;
        long long i = t * 4 - b * L;
        unsigned long long ck = feed_cloud_key(seed, step, row0 + (unsigned)b);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (i == L) {                                   // the quad crosses into the next row (L is not a multiple of 4)
                i = 0;
                b++;
                ck = feed_cloud_key(seed, step, row0 + (unsigned)b);
            }
            ys[u] = one(ck, (unsigned)i, xs[u]);
            i++;
        }
        reinterpret_cast<float4*>(y)[t] = make_float4(ys[0], ys[1], ys[2], ys[3]);
    } else {
        const long long e = n4 * 4 + (t - n4);              // the tail of a length that is not a multiple of 4 (or unaligned tensors)
        if (e < n) {
            const long long b = e / L;
            y[e] = one(feed_cloud_key(seed, step, row0 + (unsigned)b), (unsigned)(e - b * L), x[e]);
        }
    }
}

}  // namespace sph3d

using namespace sph3d;

extern "C" int sph3d_dropout_keyed(int B, long long row_len, const float* x, float* y, unsigned long long seed, unsigned long long step,
                                   long long row0, int layer, unsigned int threshold, float scale, sph3d_stream_t stream)
{
    SPH3D_REQUIRE(B >= 0 && row_len >= 0 && row_len < (1ll << 32), "dropout_keyed: B=%d rows of %lld elements (< 2^32 required)", B, row_len);
    SPH3D_REQUIRE(layer >= 0 && layer < kFeedDropoutLayers, "dropout_keyed: layer %d outside [0, %d)", layer, kFeedDropoutLayers);
    SPH3D_REQUIRE(row0 >= 0 && row0 + (long long)B <= (1ll << 32), "dropout_keyed: rows %lld .. %lld + %d do not fit 32 bits", row0, row0, B);
    const long long n = (long long)B * row_len;
    if (n == 0) return SPH3D_OK;
    const bool al = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & 15) == 0;
    const long long n4 = al ? n / 4 : 0;
    const long long threads = n4 + (n - n4 * 4);
    SPH3D_REQUIRE((threads + 255) / 256 < (1ll << 31), "dropout_keyed: %lld elements are too many for one launch", n);
    hipLaunchKernelGGL(dropout_keyed_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream), n4, n, row_len, x, y,
                       seed, step, (unsigned)row0, (unsigned long long)(kFeedDropout + layer), threshold, scale);
    return check_launch("sph3d_dropout_keyed");
}
