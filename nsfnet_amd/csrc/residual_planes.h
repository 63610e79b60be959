// Reading the unweighted residual planes eq1..eq4 an evaluation left in the field buffer (rba.hip, resample.hip):
//   e2 = ((eq1^2 + eq2^2) + eq3^2) + w4 eq4^2     fp64 from the fp32 planes, one rounding per operation
#pragma once
#include "kernels.h"

__device__ __forceinline__ double sq(float v) { return __dmul_rn((double)v, (double)v); }   // exact

// w4 = 0: e4 is 0 as well (load_eq does not read the plane), the last term is +0 and changes nothing
__device__ __forceinline__ double e2_of(float e1, float e2, float e3, float e4, double w4) {
  const double s = __dadd_rn(__dadd_rn(sq(e1), sq(e2)), sq(e3));
  return __dadd_rn(s, __dmul_rn(w4, sq(e4)));
}

// v[c][j] = plane eq(c+1) of point base + j, one 16-byte load per plane (base % 4 == 0 and base < n <= npad,
// npad % 4 == 0: in bounds); !with4: the fourth plane is not read, v[3][.] = 0
__device__ __forceinline__ void load_eq(const float* __restrict__ fld, long npad, long base, bool with4, float v[4][4]) {
  const float4 q1 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ1 * npad + base);
  const float4 q2 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ2 * npad + base);
  const float4 q3 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ3 * npad + base);
  float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (with4) q4 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ4 * npad + base);
  v[0][0] = q1.x; v[0][1] = q1.y; v[0][2] = q1.z; v[0][3] = q1.w;
  v[1][0] = q2.x; v[1][1] = q2.y; v[1][2] = q2.z; v[1][3] = q2.w;
  v[2][0] = q3.x; v[2][1] = q3.y; v[2][2] = q3.z; v[2][3] = q3.w;
  v[3][0] = q4.x; v[3][1] = q4.y; v[3][2] = q4.z; v[3][3] = q4.w;
}
