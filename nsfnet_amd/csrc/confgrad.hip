// Conflict-free combination of the per-term gradients: ConFIG (Liu, Chu & Thuerey, ICLR 2025)
// on the device.  Every step the update direction is the one with equal positive projection on every term's unit
// gradient, its length the sum of the terms' projections on it.  For the m <= 3 active terms t (r = collocation,
// b = boundary, s = supervised; g_t as the step seeds them, alpha baked in):
//   A_ij = g_i . g_j    n_t = sqrt(A_tt)    M_ij = A_ij / (n_i n_j)    M c = 1
//   k_t = (sum_i n_i / sum_i c_i) c_t / n_t                           g = sum_t k_t g_t
// Three pieces, all in a fixed order with fp64 sums and no float atomics, so every result is bit-reproducible and
// ranks that hold the same vectors compute the same coefficients:
//   confgrad_gram_kernel     per block of 64 parameters the six partial dot products rr, bb, ss, rb, rs, bs of three
//                            given vectors (multi-rank: after the all-reduce); reduce_terms_kernel (balance.hip)
//                            writes the same partials of the vectors it assembles (wave_gram, kernels.h)
//   confgrad_coef_kernel     one workgroup: partials -> A -> M -> c (Cramer, fp64) -> guards -> coef[3], record
//   confgrad_combine_kernel  g = k_r g_r + k_b g_b + k_s g_s with the coefficients read from device memory
// Guards (decided here, counted in the record): a term with n_t = 0 is dropped from the set (one left: g is that
// term; none left: g = 0); a non-finite Gram entry, det(M) <= 1e-10, sum c <= 0 or a non-finite c_t fall back to the
// plain sum k = (1, 1, 1).
#include <cmath>

#include "kernels.h"

namespace {

constexpr int kBlk = 64;          // parameters per partials block (one per reduce_terms_kernel workgroup)
constexpr int kCoefThreads = 256;
constexpr double kDetMin = 1e-10; // Gram entries are fp64 sums of exact fp32 products: det carries ~1e-15 of
                                  // cancellation error, the threshold leaves five digits

__global__ __launch_bounds__(64) void confgrad_gram_kernel(const float* __restrict__ v0, const float* __restrict__ v1,
                                                           const float* __restrict__ v2, long n,
                                                           double* __restrict__ partials) {
  const long p = blockIdx.x * (long)kBlk + threadIdx.x;
  const bool live = p < n;
  const float r = v0 && live ? v0[p] : 0.f, b = v1 && live ? v1[p] : 0.f, s = v2 && live ? v2[p] : 0.f;
  wave_gram(r, b, s, threadIdx.x, partials + (size_t)blockIdx.x * 6);
}

// record (fp64, PINN_CONFGRAD_RECORD entries): [0..2] n_r n_b n_s  [3..5] cos_rb cos_rs cos_bs  [6..8] k_r k_b k_s
// [9] |g|  [10] steps  [11] fallbacks  [12] dropped terms
__global__ __launch_bounds__(kCoefThreads) void confgrad_coef_kernel(const double* __restrict__ partials, long nblk,
                                                                     int nterms, float* __restrict__ coef,
                                                                     double* record) {
#pragma clang fp contract(off)
  __shared__ double red[kCoefThreads][6];
  const int tid = threadIdx.x;
  strided_tree_fold<kCoefThreads, FoldSum, FoldSum, FoldSum, FoldSum, FoldSum, FoldSum>(
      [&](long b, int c) { return partials[b * 6 + c]; }, nblk, red);
  if (tid != 0) return;
  const double A[3] = {red[0][0], red[0][1], red[0][2]};             // rr bb ss
  const double X[3] = {red[0][3], red[0][4], red[0][5]};             // rb rs bs
  const int pi[3] = {0, 0, 1}, pj[3] = {1, 2, 2};                    // the terms of cross entry q
  double n[3], cs[3] = {0, 0, 0}, k[3] = {1, 1, 1}, len;
  for (int t = 0; t < 3; ++t) n[t] = sqrt(A[t]);
  const double sumsq = ((A[0] + A[1]) + A[2]) + 2.0 * ((X[0] + X[1]) + X[2]);   // |g_r + g_b + g_s|^2
  bool finite = true;
  for (int t = 0; t < 3; ++t) finite = finite && isfinite(A[t]) && isfinite(X[t]);
  double fallbacks = 0.0, dropped = 0.0;
  if (!finite) {
    fallbacks = 1.0;
    len = sqrt(sumsq);
  } else {
    bool on[3];
    int m = 0;
    for (int t = 0; t < 3; ++t) {
      on[t] = t < nterms && A[t] > 0.0;
      if (t < nterms && !on[t]) dropped += 1.0;
      m += on[t];
    }
    for (int q = 0; q < 3; ++q)
      if (on[pi[q]] && on[pj[q]]) cs[q] = X[q] / (n[pi[q]] * n[pj[q]]);
    if (m == 0) {
      k[0] = k[1] = k[2] = 0.0;
      len = 0.0;
    } else {
      // M = [[1 a b] [a 1 c] [b c 1]], a term outside the set an identity row; c = adj(M) 1 / det(M)
      const double a = cs[0], b = cs[1], c = cs[2];
      const double det = ((1.0 + 2.0 * a * b * c) - a * a) - b * b - c * c;
      const double c01 = b * c - a, c02 = a * c - b, c12 = a * b - c;
      double x[3] = {((1.0 - c * c) + c01) + c02, (c01 + (1.0 - b * b)) + c12, (c02 + c12) + (1.0 - a * a)};
      double sc = 0.0, sn = 0.0;
      bool ok = det > kDetMin;
      for (int t = 0; t < 3; ++t) {
        x[t] = on[t] ? x[t] / det : 0.0;
        ok = ok && isfinite(x[t]);
        sc += x[t];
        if (on[t]) sn += n[t];
      }
      ok = ok && sc > 0.0;
      if (!ok) {
        fallbacks = 1.0;
        len = sqrt(sumsq > 0.0 ? sumsq : 0.0);
      } else {
        const double scale = sn / sc;
        for (int t = 0; t < 3; ++t) k[t] = on[t] ? scale * x[t] / n[t] : 0.0;
        len = sn / sqrt(sc);
      }
    }
  }
  for (int t = 0; t < 3; ++t) {
    record[t] = n[t];
    record[3 + t] = cs[t];
    record[6 + t] = k[t];
    coef[t] = (float)k[t];
  }
  record[9] = len;
  record[10] += 1.0;
  record[11] += fallbacks;
  record[12] += dropped;
}

// fixed order: k_r g_r (one fp32 product), then fma with k_b g_b, then fma with k_s g_s
__global__ void confgrad_combine_kernel(float* g, const float* gr, const float* __restrict__ gb,
                                        const float* __restrict__ gs, const float* __restrict__ coef, long n) {
  const float kr = coef[0], kb = coef[1], ks = gs ? coef[2] : 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = __fmul_rn(kr, gr[i]);
    v = fmaf(kb, gb[i], v);
    if (gs) v = fmaf(ks, gs[i], v);
    g[i] = v;
  }
}

}  // namespace

int launch_confgrad_gram(const float* v0, const float* v1, const float* v2, long n, double* partials, hipStream_t s) {
  hipLaunchKernelGGL(confgrad_gram_kernel, dim3((unsigned)balance_blocks(n)), dim3(kBlk), 0, s, v0, v1, v2, n, partials);
  return launch_status();
}

int launch_confgrad_coef(const double* partials, long n, int nterms, float* coef, double* record, hipStream_t s) {
  hipLaunchKernelGGL(confgrad_coef_kernel, dim3(1), dim3(kCoefThreads), 0, s, partials, balance_blocks(n), nterms, coef,
                     record);
  return launch_status();
}

int launch_confgrad_combine(float* g, const float* gr, const float* gb, const float* gs, const float* coef, long n,
                            hipStream_t s) {
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(confgrad_combine_kernel, dim3(blocks), dim3(256), 0, s, g, gr, gb, gs, coef, n);
  return launch_status();
}
