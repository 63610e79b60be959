// Device side of the S / Z-bar spill (spill.h): the plane I/O of a register quad in both quad formats, the 24-bit
// packing, and the layer-0 values that the readers of a plan without a stored layer 0 recompute.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- plane I/O -------------------------------------------------------------------------------------------------------
// Plane k of one register quad, or all N of them, <-> the (tile, layer) block at blk; plane k starts k * plq f32x4 into it.
// The (tile, layer, plane) base is uniform and pinned to scalar registers (pin_base), `so` is the lane's one 32-bit
// offset; the spill is streamed once, so every access is nontemporal.
__device__ __forceinline__ void store_plane(float* blk, size_t plq, int k, unsigned so, const f32x4& x) {
  __builtin_nontemporal_store(x, pin_base(reinterpret_cast<const f32x4*>(blk) + k * plq) + so);
}
__device__ __forceinline__ f32x4 load_plane(const float* blk, size_t plq, int k, unsigned so) {
  return __builtin_nontemporal_load(pin_base(reinterpret_cast<const f32x4*>(blk) + k * plq) + so);
}
template <int N>
__device__ __forceinline__ void store_planes(float* blk, size_t plq, unsigned so, const f32x4 (&x)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) store_plane(blk, plq, k, so, x[k]);
}
template <int N>
__device__ __forceinline__ void load_planes(const float* blk, size_t plq, unsigned so, f32x4 (&x)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = load_plane(blk, plq, k, so);
}
// SPILL_QUAD_F32: the quad's four fp32 planes
__device__ __forceinline__ void store_quad4(float* blk, size_t plq, unsigned so, const f32x4& x0, const f32x4& x1, const f32x4& x2, const f32x4& x3) {
  const f32x4 x[4] = {x0, x1, x2, x3};
  store_planes<4>(blk, plq, so, x);
}
__device__ __forceinline__ void load_quad4(const float* blk, size_t plq, unsigned so, f32x4& x0, f32x4& x1, f32x4& x2, f32x4& x3) {
  f32x4 x[4];
  load_planes<4>(blk, plq, so, x);
  x0 = x[0]; x1 = x[1]; x2 = x[2]; x3 = x[3];
}

// ---- layer 0, recomputed ---------------------------------------------------------------------------------------------
// Layer 0's pre-activation of one feature at one point - the explicit fmaf nesting is the contract: the forward
// kernels' layer 0 and every reader that recomputes it call this, so that they agree bit for bit - and its saved quad
// (t, z_x, z_y, z_D) = (tanh z, w0x, w0y, 0) of four features, with the tanh of the caller's precision mode (TanhLibm
// here, TanhFast in bf16_util.h).
__device__ __forceinline__ float layer0_z(float wx, float wy, float b, float px, float py) { return fmaf(wx, px, fmaf(wy, py, b)); }
struct TanhLibm { __device__ __forceinline__ float operator()(float z) const { return tanhf(z); } };
template <class Tanh>
__device__ __forceinline__ float layer0_t(float wx, float wy, float b, float px, float py, Tanh th) { return th(layer0_z(wx, wy, b, px, py)); }
template <class Tanh>
__device__ __forceinline__ void layer0_saved(const f32x4& wx, const f32x4& wy, const f32x4& b, float px, float py, Tanh th,
                                             f32x4& s0, f32x4& s1, f32x4& s2, f32x4& s3) {
#pragma unroll
  for (int e = 0; e < 4; ++e) s0[e] = layer0_t(wx[e], wy[e], b[e], px, py, th);
  s1 = wx; s2 = wy; s3 = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- layer 0, frozen sine (the Fourier-feature first layer; include/nsfnet_pinn.h) -------------------
// The single statement of the layer: from its pre-activation z (layer0_z) and its weights, the four a-streams
//   a = sin z,  a_x = cos z * w0x,  a_y = cos z * w0y,  a_D = -sin z * (w0x^2 + w0y^2)
// with the sine / cosine pair of the caller's precision mode (SinCosLibm here, SinCosFast in bf16_util.h).  Every forward
// kernel's FF instantiation calls this for l == 0; the quad it returns is also what an FF plan SAVES for layer 0 (the
// a-streams themselves, not (t, z_x, z_y, z_D)), so the layer-1 dW workgroups read their A operand straight from it.
struct SinCosLibm { __device__ __forceinline__ void operator()(float z, float& s, float& c) const { s = sinf(z); c = cosf(z); } };
template <class SinCos>
__device__ __forceinline__ void layer0_sine(float z, float wx, float wy, SinCos sc, float& a, float& ax, float& ay, float& ad) {
  float s, c;
  sc(z, s, c);
  a = s; ax = c * wx; ay = c * wy; ad = -s * fmaf(wx, wx, wy * wy);
}
// value mode: only a
template <class SinCos>
__device__ __forceinline__ float layer0_sine_value(float z, SinCos sc) {
  float s, c;
  sc(z, s, c);
  return s;
}

// ---- SPILL_QUAD_P24: the 24-bit format ------------------------------------------------------------------------------
// The bf16x3 operand split consumes 16 significant bits of a value (bf16 hi + bf16 lo); the spilled activations and
// z-adjoints are read back only to be split (MFMA operands) or to enter chain-rule products whose other factors are
// bf16x3 GEMM outputs of that accuracy.  So they are spilled ROUNDED TO 24 BITS (sign, exponent, 15 mantissa bits:
// relative error <= 2^-16): the sixteen values of a register quad (4 features x 4 streams) travel as THREE 16-byte
// planes - top halves of streams 0-1, top halves of streams 2-3, third bytes of all four - instead of four fp32
// planes: a quarter fewer vector-memory instructions and bytes with the same 1-KiB-per-wave-instruction coalescing.
// (Measured first as separate 8-byte and 4-byte planes: the same bytes in TWICE the instructions was slower than
// fp32 - the spill is bound by memory instructions through the CU's vector-memory path, not by HBM bytes.)
// Round half up in magnitude on the integer image; v_perm_b32 moves the bytes.
// NaN / infinity through the spill: +-infinity and every NaN whose payload is below 0x7fff80 keep their class (the add
// stays inside the mantissa; the dropped low byte is never the only payload of a NaN that arithmetic produced, because
// the hardware sets the quiet bit 0x400000: its own NaNs are 0x7fc00000 / 0xffc00000).  A NaN with an all-ones payload
// (0x7fffff80 .. 0x7fffffff, either sign) would carry into the exponent and read back as +-0; no instruction of the
// sweeps produces one, and guarding the add costs three VALU per value in the hottest loop (96 per quarter phase),
// so the case is documented and pinned by tests/test_spill_format.py instead.
__device__ __forceinline__ void pack24(const f32x4& x, u32x2& hi, unsigned& lo) {
  const unsigned r0 = __float_as_uint(x[0]) + 0x80u, r1 = __float_as_uint(x[1]) + 0x80u;
  const unsigned r2 = __float_as_uint(x[2]) + 0x80u, r3 = __float_as_uint(x[3]) + 0x80u;
  hi[0] = __builtin_amdgcn_perm(r1, r0, 0x07060302u);      // (selector bytes 0-3: second operand, 4-7: first, 0x0c: zero)
  hi[1] = __builtin_amdgcn_perm(r3, r2, 0x07060302u);
  lo = __builtin_amdgcn_perm(r1, r0, 0x0c0c0501u) | __builtin_amdgcn_perm(r3, r2, 0x05010c0cu);
}
__device__ __forceinline__ f32x4 unpack24(const u32x2& hi, unsigned lo) {
  f32x4 x;
  x[0] = __uint_as_float(__builtin_amdgcn_perm(hi[0], lo, 0x0504000cu));
  x[1] = __uint_as_float(__builtin_amdgcn_perm(hi[0], lo, 0x0706010cu));
  x[2] = __uint_as_float(__builtin_amdgcn_perm(hi[1], lo, 0x0504020cu));
  x[3] = __uint_as_float(__builtin_amdgcn_perm(hi[1], lo, 0x0706030cu));
  return x;
}

// a register quad's four planes <-> the three 16-byte planes of the spill (hi16 of planes 0-1, of planes 2-3, lo8 of all)
__device__ __forceinline__ void pack24_quad(const f32x4& x0, const f32x4& x1, const f32x4& x2, const f32x4& x3, u32x4 (&pk)[3]) {
  u32x2 h; unsigned l;
  pack24(x0, h, l); pk[0][0] = h[0]; pk[0][1] = h[1]; pk[2][0] = l;
  pack24(x1, h, l); pk[0][2] = h[0]; pk[0][3] = h[1]; pk[2][1] = l;
  pack24(x2, h, l); pk[1][0] = h[0]; pk[1][1] = h[1]; pk[2][2] = l;
  pack24(x3, h, l); pk[1][2] = h[0]; pk[1][3] = h[1]; pk[2][3] = l;
}
__device__ __forceinline__ f32x4 unpack24_plane(const u32x4 (&pk)[3], int p) {
  return unpack24(u32x2{pk[p >> 1][2 * (p & 1)], pk[p >> 1][2 * (p & 1) + 1]}, pk[2][p]);
}
// plane p alone, for epilogues that produce a quad one plane at a time ...
__device__ __forceinline__ void pack24_plane(const f32x4& x, int p, u32x4 (&pk)[3]) {
  u32x2 h; unsigned l;
  pack24(x, h, l);
  pk[p >> 1][2 * (p & 1)] = h[0]; pk[p >> 1][2 * (p & 1) + 1] = h[1]; pk[2][p] = l;
}
// ... and, after plane p, the 16-byte planes of pk it completed into the block at dst (planes plq f32x4 apart)
__device__ __forceinline__ void store24_planes(float* dst, size_t plq, unsigned so, int p, const u32x4 (&pk)[3]) {
  if (p & 1) __builtin_nontemporal_store(__builtin_bit_cast(f32x4, pk[p >> 1]), pin_base(reinterpret_cast<const f32x4*>(dst) + (p >> 1) * plq) + so);
  if (p == 3) __builtin_nontemporal_store(__builtin_bit_cast(f32x4, pk[2]), pin_base(reinterpret_cast<const f32x4*>(dst) + 2 * plq) + so);
}
// a whole packed quad at once
__device__ __forceinline__ void store_quad24(float* blk, size_t plq, unsigned so, const u32x4 (&pk)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) store_plane(blk, plq, k, so, __builtin_bit_cast(f32x4, pk[k]));
}
__device__ __forceinline__ void load_quad24(const float* blk, size_t plq, unsigned so, u32x4 (&pk)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) pk[k] = __builtin_bit_cast(u32x4, load_plane(blk, plq, k, so));
}

// a register quad <-> its block in either quad format (Spill::quad, uniform): what the sweeps that serve both use
__device__ __forceinline__ void store_quad(int quad, float* blk, size_t plq, unsigned so, const f32x4& x0, const f32x4& x1, const f32x4& x2, const f32x4& x3) {
  if (quad == SPILL_QUAD_P24) {      // three instructions instead of four
    u32x4 pk[3];
    pack24_quad(x0, x1, x2, x3, pk);
    store_quad24(blk, plq, so, pk);
  } else {
    store_quad4(blk, plq, so, x0, x1, x2, x3);
  }
}
__device__ __forceinline__ void load_quad(int quad, const float* blk, size_t plq, unsigned so, f32x4& x0, f32x4& x1, f32x4& x2, f32x4& x3) {
  if (quad == SPILL_QUAD_P24) {
    u32x4 pk[3];
    load_quad24(blk, plq, so, pk);
    x0 = unpack24_plane(pk, 0); x1 = unpack24_plane(pk, 1); x2 = unpack24_plane(pk, 2); x3 = unpack24_plane(pk, 3);
  } else {
    load_quad4(blk, plq, so, x0, x1, x2, x3);
  }
}
