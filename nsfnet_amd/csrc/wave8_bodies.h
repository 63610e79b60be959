// What the four 8-wave bf16 / bf16x3 sweeps (fwd_bf16.hip, bwd_bf16.hip and their _wide variants) share as functions:
// the bf16 hi / lo restaging of a register quad into the LDS image, the cross-wave sum of the output layer and the
// workgroup's closing reductions.  Their epilogues, k-loops, weight prefetch, output partials and the v_permlane16_swap
// regrouping stay written out per kernel: as shared functions each of them moved the register allocation of some
// instantiation into scratch, and the epilogues also moved results in the last bit.
#pragma once
#include "kernels.h"
#include "bf16_util.h"
#include "reduce_util.h"

// one register quad (4 consecutive features, one column) of plane `plane` restaged as bf16 hi / lo: 8 bytes each at
// `off` = XI::chunk_off(pp, chunk) + 8 h of the plane
template <class XI, int TERMS>
__device__ __forceinline__ void restage(unsigned char* Xb, int plane, int off, const f32x4& v) {
  u32x2 vh, vl;
  split4(v[0], v[1], v[2], v[3], vh, vl);
  *reinterpret_cast<u32x2*>(Xb + plane * XI::PLANE * 2 + off) = vh;
  if (TERMS == 3) *reinterpret_cast<u32x2*>(Xb + XI::HALF * 2 + plane * XI::PLANE * 2 + off) = vl;
}

// output layer: outv[c][col] = bout[c] (value mode, or stream 0 of the residual mode) + the NW waves' partials part[w][c][col]
template <int NS, int PPL, int NW>
__device__ __forceinline__ void out_sum(const float* part, float* outv, const float* __restrict__ bout, int tid) {
  constexpr int COLS = 4 * PPL;
  for (int idx = tid; idx < 3 * COLS; idx += NW * 64) {
    int c3 = idx / COLS, cc = idx % COLS;
    float s = (NS == 1 || cc < PPL) ? bout[c3] : 0.f;
    for (int ww = 0; ww < NW; ++ww) s += part[(ww * 4 + c3) * COLS + cc];
    outv[c3 * COLS + cc] = s;
  }
}

// ---- the workgroup's closing reductions over its NT threads (red: the LDS, no longer in use) ------------------------
// forward: the four loss sums of the workgroup's points into its row of partials (the other entries are zero)
template <int NT>
__device__ __forceinline__ void flush_loss(float* red, const float (&lsum)[4], const FwdArgs& a, int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k * NT + tid] = lsum[k];
  __syncthreads();
  if (tid < 4) {
    float s = 0.f;
    for (int t = 0; t < NT; ++t) s += red[tid * NT + t];
    a.partials[blockIdx.x * PINN_NLOSS + tid] = s;
  } else if (tid < PINN_NLOSS) {
    a.partials[blockIdx.x * PINN_NLOSS + tid] = 0.f;
  }
}
// reverse sweep: d b_out into its slot of the skinny gradients, then those to the workgroup's row of a.sg
template <int HP, int NT>
__device__ __forceinline__ void flush_sg(float* red, const float (&dbo)[3], float* sgacc, int SG, const BwdArgs& a, int tid) {
  const int L = a.L;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) red[c * NT + tid] = dbo[c];
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int t = 0; t < NT; ++t) s += red[tid * NT + t];
    sgacc[sg_bout(HP, L) + tid] = s;
  }
  __syncthreads();
  float* out = a.sg + (size_t)blockIdx.x * SG;
  for (int i = tid; i < SG; i += NT) out[i] = sgacc[i];
}
