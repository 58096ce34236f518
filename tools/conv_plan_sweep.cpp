// conv_plan_sweep.cpp — conv_plan() (sph3d_gcn_amd/csrc/conv_plan.hpp) over the grid of tests/test_conv_forms.py, the 2^32 edges
// of the offset guards and the ends of the int range, as a host program of its own: built with the sanitizers it shows that the
// plan's integer arithmetic has no undefined behaviour there.  Prints the number of plans and a checksum of their fields.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/conv_plan_sweep.cpp -o /tmp/conv_plan_sweep
//   /tmp/conv_plan_sweep
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../sph3d_gcn_amd/csrc/conv_plan.hpp"

using namespace sph3d;

static unsigned long long sum = 1469598103934665603ull, count = 0;

static void one(int op, int B, int N, int M, int F, int Ca, int Cb, int r, int K)
{
    static const int hooks[3][2] = {{32768, 1024}, {1, 8}, {8192, 1}};
    for (int det = 0; det < 2; det++)
        for (int active = 0; active < 2; active++)
            for (const auto& h : hooks) {
                const ConvPlan p = conv_plan(op, B, N, M, F, Ca, Cb, r, K, det != 0, active != 0, h[0], h[1]);
                long long f[sizeof(ConvPlan) / sizeof(long long)] = {};
                memcpy(f, &p, offsetof(ConvPlan, bad));
                for (long long v : f) sum = (sum ^ (unsigned long long)v) * 1099511628211ull;
                sum = (sum ^ (unsigned long long)p.bad) * 1099511628211ull;
                count++;
            }
}

static void every_op(int B, int N, int M, int F, int C, int r, int K)
{
    one(kConvFwd, B, N, M, F, C, 0, r, K);
    one(kConvGradT, B, N, M, F, C, 0, r, K);
    const int ca[] = {4, 64, 128, 256, C - 4, C};
    for (int a : ca) {
        one(kConvFwdCat, B, N, M, F, a, C - a, r, K);
        one(kConvGradTCat, B, N, M, F, a, C - a, r, K);
    }
}

int main()
{
    const int Cs[] = {3, 4, 6, 35, 60, 64, 67, 68, 124, 128, 131, 132, 256, 257, 260, 512};
    const int rs[] = {1, 2, 3, 4};
    const int Fs[] = {1, 17, 18, 33, 34, 49, 63, 64, 65, 66, 159, 160, 161, 164, 165, 254, 255};
    const int Bs[] = {0, 1, 3, 8, 9, 16};
    const int Ns[] = {1, 7, 128, 768, 8192, 32767, 32768};
    const long long two32 = 1LL << 32, imax = 0x7fffffff;
    for (int C : Cs)
        for (int r : rs) {
            for (int F : Fs)
                for (int B : Bs)
                    for (int N : Ns) {
                        every_op(B, N, 107, F, C, r, 16);
                        every_op(B, N, 0, F, C, r, 16);
                    }
            // N = 2^24 and 2^24 + 1; N C 4 + 1024, N C + 256 and M C r + 256 one below, at and above 2^32 (where an int reaches them)
            std::vector<long long> n = {1 << 24, (1 << 24) + 1}, m;
            for (long long d = -1; d <= 1; d++) {
                n.push_back((two32 - 1024) / (4 * C) + d);
                n.push_back((two32 - 256) / C + d);
                m.push_back((two32 - 256) / (C * r) + d);
            }
            for (int F : {17, 33, 65, 159})
                for (int B : {1, 3, 16}) {
                    for (long long N : n)
                        if (N <= imax) every_op(B, (int)N, 107, F, C, r, 16);
                    for (long long M : m)
                        if (M <= imax) every_op(B, 768, (int)M, F, C, r, 16);
                }
        }
    // the ends of the int range, one dimension at a time and all at once
    const int ends[] = {-0x7fffffff - 1, -1, 0, 1, 0x7fffffff};
    const int base[8] = {3, 768, 107, 33, 64, 64, 2, 16};              // B, N, M, F, Ca, Cb, r, K
    for (int op = kConvFwd; op <= kConvGradTCat; op++) {
        for (int i = 0; i < 8; i++)
            for (int v : ends) {
                int d[8];
                memcpy(d, base, sizeof(d));
                d[i] = v;
                one(op, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
            }
        for (int v : ends) one(op, v, v, v, v, v, v, v, v);
        for (int F : {1, 33, 65, 160})
            for (int r : {1, 2, 256, 257, 0x7fffffff})
                for (int C : {1, 3, 4, 0x7ffffffc, 0x7fffffff})
                    one(op, 0x7fffffff, 0x7fffffff, 0x7fffffff, F, C, op == kConvFwdCat || op == kConvGradTCat ? 0x7fffffff : 0, r, 1);
    }
    printf("%llu plans, checksum %016llx\n", count, sum);
    return 0;
}
