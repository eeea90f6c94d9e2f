// Sub-pixel quotient of the fused pass's pair-layout left tail (bm2, dsx_bm.hip).  Plain C++ on the
// host (no HIP), so the CPU tests compile it directly (tests/test_subpix_quot.py).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSX_HD __host__ __device__ __forceinline__
#else
#define DSX_HD inline
#endif

namespace dsx {

// q = trunc(num / den2) (C semantics) for the parabola step num = (cm - cp) * 16 + den, den2 = 2 den,
// den = max(1, cm + cp - 2 cb) with cm, cp >= cb: den >= |cm - cp|, so num lies in [-15 den, 17 den],
// q in [-7, 8], den2 <= 229,500 (15x15 SAD) and |num| < 2^22 - every operand is exact in f32.
// rcp is an estimate of 1 / den2 within 1 ulp of the correctly rounded one (v_rcp_f32).
//   q0 = num * rcp               |q0 - q| <= 8.5 * (2^-22 + 2^-24) < 2.6e-6
//   r  = fma(-q0, den2, num)     the residual num - q0 den2 of the real q0, rounded once (|r| < 0.6)
//   q1 = fma(r, rcp, q0)         one Newton step: before its rounding, q1 - q = (q - q0) * (den2 rcp - 1) + r's
//                                rounding / den2, below 1e-12; rounded, |q1 - q| <= ulp(8) / 2 = 4.8e-7
// An exact multiple gives the integer q itself (the nearest float to a value 1e-12 away from it); any other
// quotient is at least 1 / den2 >= 4.3e-6 away from an integer, nine times q1's error, so truncating q1
// is C's truncation.  No integer multiply, no fix-up branches.
DSX_HD int subpix_quot_rcp(int num, int den2, float rcp) {
    const float nf = (float)num, df = (float)den2;
    const float q0 = nf * rcp;
    const float r = __builtin_fmaf(-q0, df, nf);
    return (int)__builtin_fmaf(r, rcp, q0);
}

DSX_HD int subpix_quot(int num, int den2) {
#if defined(__HIP_DEVICE_COMPILE__)
    return subpix_quot_rcp(num, den2, __builtin_amdgcn_rcpf((float)den2));
#else
    return subpix_quot_rcp(num, den2, 1.0f / (float)den2);
#endif
}

}  // namespace dsx
