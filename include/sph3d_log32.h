/* sph3d_log32.h — the ONE -log used by the keyed inverse-density sampler (csrc/idsample.hip, harness/idsample.py).
 *
 * Why it exists: the sampler's keys t = -log(u) / w must be equal, bit for bit, between the kernel and the numpy statement.
 * libm's, numpy's and the device library's logf differ in the last bits, so both sides evaluate THIS scheme, every operation one
 * fp32 operation rounded to nearest — no fused multiply-add, a correctly rounded division: build with -ffp-contract=off and
 * -fhip-fp32-correctly-rounded-divide-sqrt, as the library's Makefile does.
 *
 * The argument is u = k * 2^-24, k = 1 .. 2^24 (a normal fp32 in (0, 1]).  u = m * 2^e with m in [1, 2) by its bits; an m whose
 * bits exceed sqrt(2)'s (0x3fb504f3) is halved and e takes the 1, so m lies in (sqrt(1/2), sqrt(2)] and
 *     log(m) = 2 atanh(s) = s * sum_k 2/(2k+1) z^k,   s = (m - 1) / (m + 1),  z = s * s <= 0.02944.
 * The coefficients are 2/(2k+1), k = 0..5, rounded to fp32 (the k = 6 term is below 1e-10 of the sum), Horner's scheme with one
 * multiply and one add per coefficient.  r = float(e) * ln2 + s * q, and the result is 0.0f - r, not -r: u = 1 gives +0.
 * Over all 2^24 arguments: finite, sign bit clear, non-increasing in u, within 3.49 * 2^-24 (relative) of the float64 -log(u)
 * (tests/test_idsample.py walks them).  harness/idsample.py reads the lists below from this file: they are written once.
 *
 * Header is valid C99, C++ and HIP (host + device).
 */
#ifndef SPH3D_LOG32_H
#define SPH3D_LOG32_H

#define SPH3D_LOG32_DEGREE 5
/* c0 .. c5 = 2/(2k+1), nine significant digits each: the decimal form determines the fp32 value */
#define SPH3D_LOG32_COEFFS { 2.000000000e+00f, 6.666666865e-01f, 4.000000060e-01f, 2.857142985e-01f, 2.222222239e-01f, 1.818181872e-01f }
#define SPH3D_LOG32_LN2 6.931471825e-01f
#define SPH3D_LOG32_SQRT2_BITS 0x3fb504f3u

#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__
#endif
static inline float sph3d_neglog32(float u)
{
    const float c[SPH3D_LOG32_DEGREE + 1] = SPH3D_LOG32_COEFFS;
    unsigned bits, mbits;
    int e, k;
    float m, s, z, q, r;
    __builtin_memcpy(&bits, &u, sizeof(bits));
    e = (int)(bits >> 23) - 127;
    mbits = (bits & 0x007fffffu) | 0x3f800000u;
    if (mbits > SPH3D_LOG32_SQRT2_BITS) {
        mbits -= 0x00800000u;       /* m / 2, exact */
        e += 1;
    }
    __builtin_memcpy(&m, &mbits, sizeof(m));
    s = (m - 1.0f) / (m + 1.0f);
    z = s * s;
    q = c[SPH3D_LOG32_DEGREE];
    for (k = SPH3D_LOG32_DEGREE - 1; k >= 0; k--) q = q * z + c[k];
    r = (float)e * SPH3D_LOG32_LN2;
    s = s * q;
    r = r + s;
    /* = 0.0f - r.  The zero is returned as a literal: where the result feeds a division, hipcc's gfx950 lowering takes the
     * subtraction into the division's operand as a negation, (0 - r) / w -> (-r) / w, and u = 1 would give -0 */
    return r == 0.0f ? 0.0f : 0.0f - r;
}

#endif /* SPH3D_LOG32_H */
