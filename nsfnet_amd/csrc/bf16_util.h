// bf16 split helpers and LDS image geometry of the bf16x3 MFMA path (gfx950).
//
// bf16x3: every fp32 operand x is split x = hi + lo (both bf16, RNE) and a product is
// accumulated as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_32x32x16_bf16 with fp32
// accumulate (the dropped a_lo*b_lo term is ~2^-18 relative).  Operand layouts were checked
// on hardware by tests/micro/mfma_bf16_layout.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "spill_io.h"

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {   // lowers to v_cvt_pk_bf16_f32 (RNE)
  bf16x2_t v;
  v[0] = (__bf16)a; v[1] = (__bf16)b;
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf_lo_f(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi_f(unsigned p) { return __uint_as_float(p & 0xffff0000u); }

// four consecutive values -> packed hi (2 dwords) and lo (2 dwords)
__device__ __forceinline__ void split4(float x0, float x1, float x2, float x3, u32x2& hi, u32x2& lo) {
  unsigned h0 = pack_bf16(x0, x1), h1 = pack_bf16(x2, x3);
  hi[0] = h0; hi[1] = h1;
  lo[0] = pack_bf16(x0 - bf_lo_f(h0), x1 - bf_hi_f(h0));
  lo[1] = pack_bf16(x2 - bf_lo_f(h1), x3 - bf_hi_f(h1));
}

// tanh for the bf16 modes: 1 - 2/(exp(2z)+1) on v_exp_f32 / v_rcp_f32 (both 1 ulp: abs. error
// ~2e-7, far below the bf16x3 operand rounding); saturates correctly at +-inf.  The bare v_rcp_f32
// matters: an IEEE 1/x costs 11 VALU instructions, a fifth of the whole chain-rule epilogue.
__device__ __forceinline__ float fast_tanh(float z) {
  float e = __builtin_amdgcn_exp2f(z * 2.8853900817779268f);     // exp(2z) = 2^(2 z log2 e): one multiply
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}
struct TanhFast { __device__ __forceinline__ float operator()(float z) const { return fast_tanh(z); } };

// sine and cosine for the bf16 modes (the frozen sine first layer, spill_io.h layer0_sine): v_sin_f32 / v_cos_f32 take
// their argument in revolutions and are specified on [-256, 256] only, so the range is reduced explicitly: k = the
// nearest whole number of revolutions, f = z / 2 pi - k in [-1/2, 1/2] from ONE fused product (the rounding of the
// large product z / 2 pi never reaches f) plus the low part of 1 / 2 pi, which matters once |z| is tens of radians.
// Four VALU and two transcendental instructions; absolute error about 1e-6, below the bf16x3 operand rounding.
__device__ __forceinline__ void fast_sincos(float z, float& s, float& c) {
  constexpr float INV2PI_HI = 0.159154937f, INV2PI_LO = 6.42063824e-9f;     // 1 / 2 pi = hi + lo
  const float k = rintf(z * INV2PI_HI);
  const float f = fmaf(z, INV2PI_LO, fmaf(z, INV2PI_HI, -k));
  s = __builtin_amdgcn_sinf(f);
  c = __builtin_amdgcn_cosf(f);
}
struct SinCosFast { __device__ __forceinline__ void operator()(float z, float& s, float& c) const { fast_sincos(z, s, c); } };

__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
// Timing-only stand-in (PINN_ABL & 1024, scripts/abl_build.py): the same multiply-accumulate count, operand bytes and
// issue cycles as one 32x32x16 MFMA, as TWO v_mfma_f32_16x16x32_bf16 on half Q of the accumulator (wrong results on
// purpose).  It prices the MFMA SHAPE: the chip holds a higher clock on the 16x16x32 form (MI355X_MICROARCH.md, DVFS
// give-back item 7), at twice the MFMA issue slots.
__device__ __forceinline__ f32x16 mfma_bf16_shape16(int Q, u32x4 a, u32x4 b, f32x16 c) {      // Q: a constant after unrolling
  f32x4 c0 = {c[8 * Q + 0], c[8 * Q + 1], c[8 * Q + 2], c[8 * Q + 3]}, c1 = {c[8 * Q + 4], c[8 * Q + 5], c[8 * Q + 6], c[8 * Q + 7]};
  c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c0, 0, 0, 0);
  c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, b), __builtin_bit_cast(bf16x8_t, a), c1, 0, 0, 0);      // (operands swapped: not a common subexpression)
#pragma unroll
  for (int i = 0; i < 4; ++i) { c[8 * Q + i] = c0[i]; c[8 * Q + 4 + i] = c1[i]; }
  return c;
}
#ifndef PINN_ABL
#define PINN_ABL_SHAPE16 0
#else
#define PINN_ABL_SHAPE16 ((PINN_ABL) & 1024)
#endif
#define MFMA_Q(q, a, b, c) (PINN_ABL_SHAPE16 ? mfma_bf16_shape16((q) & 1, a, b, c) : mfma_bf16(a, b, c))

// ---- activation image in LDS for the fused fwd/bwd kernels -------------------
// X[hilo(2)][plane(4)][col in plane (PPL)][k (RSE)] bf16, RSE = HP rounded up to a power of two
// (>= 32); 16-byte chunks (8 k) XOR-swizzled so that the ds_read_b128 of one k-chunk by
// different columns is bank-conflict free.  PPL = 32 (128-column tile) or 16 (64-column tile).
template <int HP, int PPL = 32>
struct XImg {
  static constexpr int RSE = HP <= 32 ? 32 : HP <= 64 ? 64 : HP <= 128 ? 128 : HP <= 256 ? 256 : 512;
  static constexpr int NCH = RSE / 8;                    // chunks per row
  static constexpr int R = RSE >= 128 ? 1 : 128 / RSE;   // rows per 256-byte bank row
  static constexpr int MASK = (NCH < 16 ? NCH : 16) - 1;
  static constexpr int PLANE = PPL * RSE;                // elements per (hilo, plane)
  static constexpr int HALF = 4 * PLANE;                 // elements per hilo half
  static constexpr size_t BYTES = (size_t)2 * HALF * 2;
  // byte offset (within one plane) of chunk `ch` of column `col`
  __device__ static __forceinline__ int chunk_off(int col, int ch) {
    return (col * RSE + ((ch ^ ((col / R) & MASK)) << 3)) * 2;
  }
};
