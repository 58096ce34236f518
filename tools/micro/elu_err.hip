// elu_err.hip — how far is the ELU of the separable kernels and of norm.hip, `y > 0.f ? y : __expf(y) - 1.f`, from expm1?
// Neither the library nor the programming guides state the accuracy of v_exp_f32, so the absolute term E of the float64 tests of the
// separable layer (tests/_sep_ref.py: |elu_fp32(y) - elu(y)| <= E 2^-24) is measured: EVERY fp32 y in [-104, 0] (-0.0f down to
// -104.0f by bit pattern, and +0.0f), about 1.12e9 values, one launch, each compared in the same kernel with float64 expm1.
// Prints the maximum of |err| / 2^-24 and the y that gives it.  For y > 0 the expression returns y itself: no error.
// build (the library's own floating-point flags): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/micro/elu_err.hip -o tools/micro/elu_err
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

__device__ __forceinline__ float elu1(float y) { return y > 0.f ? y : __expf(y) - 1.f; }      // a copy of csrc/common.hpp: elu1 (this program stands alone)

constexpr int kBlocks = 4096, kThreads = 256;

__global__ __launch_bounds__(kThreads) void elu_err_kernel(uint32_t first, uint32_t count, double* __restrict__ werr, uint32_t* __restrict__ wbits,
                                                            unsigned long long* __restrict__ nonfinite)
{
    __shared__ double serr[kThreads];
    __shared__ uint32_t sbits[kThreads];
    double worst = -1.0;
    uint32_t wb = first;
    unsigned long long bad = 0;
    const uint32_t stride = (uint32_t)kBlocks * kThreads;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < count; i += stride) {
        const uint32_t b = i + 1 == count ? 0u : first + i;              // the last one is +0.0f
        const float y = __uint_as_float(b);
        const float z = elu1(y);
        if (!(fabsf(z) <= 1.0f)) bad++;                                     // NaN, or outside [-1, 0]
        const double e = fabs((double)z - expm1((double)y)) * 16777216.0;
        if (e > worst) { worst = e; wb = b; }
    }
    serr[threadIdx.x] = worst;
    sbits[threadIdx.x] = wb;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && serr[threadIdx.x + o] > serr[threadIdx.x]) {
            serr[threadIdx.x] = serr[threadIdx.x + o];
            sbits[threadIdx.x] = sbits[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { werr[blockIdx.x] = serr[0]; wbits[blockIdx.x] = sbits[0]; }
    if (bad) atomicAdd(nonfinite, bad);
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main()
{
    const float lo = -104.0f;
    uint32_t first = 0x80000000u, last;
    memcpy(&last, &lo, 4);
    const uint32_t count = last - first + 2;                                // -0.0f .. -104.0f, and +0.0f
    double* werr; uint32_t* wbits; unsigned long long* bad;
    CHECK(hipMalloc(&werr, sizeof(double) * kBlocks));
    CHECK(hipMalloc(&wbits, sizeof(uint32_t) * kBlocks));
    CHECK(hipMalloc(&bad, sizeof(unsigned long long)));
    CHECK(hipMemset(bad, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(elu_err_kernel, dim3(kBlocks), dim3(kThreads), 0, 0, first, count, werr, wbits, bad);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<double> herr(kBlocks);
    std::vector<uint32_t> hbits(kBlocks);
    unsigned long long hbad = 0;
    CHECK(hipMemcpy(herr.data(), werr, sizeof(double) * kBlocks, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hbits.data(), wbits, sizeof(uint32_t) * kBlocks, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost));
    int w = 0;
    for (int i = 1; i < kBlocks; i++)
        if (herr[i] > herr[w]) w = i;
    float y;
    memcpy(&y, &hbits[w], 4);
    printf("elu_err: %u values of y in [-104, 0]; max |elu_fp32(y) - expm1(y)| / 2^-24 = %.6f at y = %.9g (bits 0x%08x); "
           "results that are NaN or outside [-1, 0]: %llu\n", count, herr[w], (double)y, hbits[w], hbad);
    return hbad ? 2 : 0;
}
