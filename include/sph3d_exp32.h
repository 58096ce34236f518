/* sph3d_exp32.h — the ONE exp used by the scene merge's soft-max (csrc/scene.hip, harness/scenemerge.py).
 *
 * Why it exists: the merged per-scene probabilities must be equal, bit for bit, between the kernel and the numpy statement.
 * libm's, numpy's and the device library's expf differ in the last bits, so both sides evaluate THIS polynomial: Horner's
 * scheme with one fp32 multiply and one fp32 add per coefficient, each rounded to nearest — no fused multiply-add: build with
 * -ffp-contract=off, as the library's Makefile does (csrc/scene.hip also switches contraction off for the file).
 *
 * The argument is a component of a unit vector, |u| <= 1 (an ulp more when the norm rounds down).  The coefficients are the
 * Taylor coefficients 1/k!, k = 0..10, rounded to fp32: truncation error 1/11! = 2.5e-8 at |u| = 1, below half an ulp of the
 * result; with the rounding of the ten steps the result is within a few ulp of exp(u).  harness/scenemerge.py reads the list
 * below from this file: it is written once.
 *
 * Header is valid C99, C++ and HIP (host + device).
 */
#ifndef SPH3D_EXP32_H
#define SPH3D_EXP32_H

#define SPH3D_EXP32_DEGREE 10
/* c0 .. c10, nine significant digits each: the decimal form determines the fp32 value */
#define SPH3D_EXP32_COEFFS { 1.000000000e+00f, 1.000000000e+00f, 5.000000000e-01f, 1.666666716e-01f, 4.166666791e-02f, 8.333333768e-03f, 1.388888923e-03f, 1.984127011e-04f, 2.480158764e-05f, 2.755731884e-06f, 2.755731998e-07f }

#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__
#endif
static inline float sph3d_exp32(float u)
{
    const float c[SPH3D_EXP32_DEGREE + 1] = SPH3D_EXP32_COEFFS;
    float p = c[SPH3D_EXP32_DEGREE];
    int k;
    for (k = SPH3D_EXP32_DEGREE - 1; k >= 0; k--) p = p * u + c[k];
    return p;
}

#endif /* SPH3D_EXP32_H */
