// Adaptive loss-weight balancing: the learning-rate-annealing rule of Wang, Teng &
// Perdikaris (2021, Algorithm 1) on the device.  Three pieces, all in a fixed order with fp64 sums and no float
// atomics, so every result is bit-reproducible and ranks that hold the same vectors compute the same weights:
//   reduce_terms_kernel    the gradient assembly of misc.hip with the sources split into the collocation, boundary
//                          and supervised groups, one fp32 vector per group, optionally with per-workgroup
//                          max|g| / sum|g| partials of what it wrote (and, on request, the Gram partials of
//                          confgrad.hip)
//   balance_stats_kernel   the same partials of three given vectors (multi-rank: after the all-reduce)
//   balance_update_kernel  one workgroup: partials -> max|g_r|, mean|g_t| -> lambda_hat_t -> lambda_t
//   balance_combine_kernel g = g_r + lambda_b g_b + lambda_s g_s with the weights read from device memory
#include <cmath>

#include "kernels.h"

namespace {

constexpr int kBlk = 64;          // parameters per partials block (one per reduce_terms_kernel workgroup)
constexpr int kUpdThreads = 256;

// max (NaN-propagating: a NaN gradient entry must reach lambda_hat and skip the update) and sum of |v| over the 64
// lanes of a wave; lane 0 holds the result
__device__ __forceinline__ void wave_abs_stats(float v, double& mx, double& sm) {
  const double a = fabs((double)v);
  mx = wave_fold<FoldNanMax>(a);
  sm = wave_fold<FoldSum>(a);
}

__global__ __launch_bounds__(512) void reduce_terms_kernel(TermReduceArgs a) {
  // as reduce_kernel: 64 consecutive flat parameters per workgroup, wave w of 8 sums the partial-gradient rows
  // w, w+8, ... of each source of a group in source order, the 8 wave sums are added in wave order
  __shared__ double part[3][8][64];
  const int H = a.H, HP = a.HP, L = a.L;
  const size_t P = flat_total(H, L, a.n_out);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t p = blockIdx.x * (size_t)64 + lane;
  const bool live = p < P;
  const ReduceLoc loc = live ? reduce_locate(p, H, HP, L, a.n_out) : ReduceLoc{-1, -1, 0};
  const size_t SG = sg_total(HP, L);
  const bool frozen = p < (size_t)a.frozen;      // (a frozen first layer: +0.0 in every vector, and in the statistics)
  int k = 0;
  for (int t = 0; t < 3; ++t) {
    double s = 0.0;
    for (int j = 0; j < a.nsrc[t]; ++j, ++k)
      if (live && !frozen) s = reduce_source_add(s, a.src[k], loc, HP, SG, w);
    part[t][w][lane] = s;
  }
  __syncthreads();
  if (w != 0) return;
  float vt[3];
  for (int t = 0; t < 3; ++t) {
    float v = 0.f;
    if (a.out[t] && live) {
      double s = part[t][0][lane];
#pragma unroll
      for (int i = 1; i < 8; ++i) s += part[t][i][lane];
      v = frozen ? 0.f : (a.acc_mask >> t) & 1 ? a.out[t][p] + (float)s : (float)s;
      a.out[t][p] = v;
    }
    if (a.partials) {
      double mx, sm;
      wave_abs_stats(v, mx, sm);
      if (lane == 0) {
        a.partials[(size_t)blockIdx.x * 6 + 2 * t] = mx;
        a.partials[(size_t)blockIdx.x * 6 + 2 * t + 1] = sm;
      }
    }
    vt[t] = v;
  }
  if (a.gram) wave_gram(vt[0], vt[1], vt[2], lane, a.gram + (size_t)blockIdx.x * 6);   // confgrad.hip's statistics
}

__global__ __launch_bounds__(64) void balance_stats_kernel(const float* __restrict__ v0, const float* __restrict__ v1,
                                                           const float* __restrict__ v2, long n,
                                                           double* __restrict__ partials) {
  const long p = blockIdx.x * (long)kBlk + threadIdx.x;
  const float* v[3] = {v0, v1, v2};
  for (int t = 0; t < 3; ++t) {
    double mx, sm;
    wave_abs_stats(v[t] && p < n ? v[t][p] : 0.f, mx, sm);
    if (threadIdx.x == 0) {
      partials[(size_t)blockIdx.x * 6 + 2 * t] = mx;
      partials[(size_t)blockIdx.x * 6 + 2 * t + 1] = sm;
    }
  }
}

// record (fp64, PINN_BALANCE_RECORD entries): [0] max|g_r| [1] mean|g_r| [2] max|g_b| [3] mean|g_b| [4] lambda_hat_b
// [5] max|g_s| [6] mean|g_s| [7] lambda_hat_s [8] skipped term updates [9] lambda_b [10] lambda_s [11] balance steps
__global__ __launch_bounds__(kUpdThreads) void balance_update_kernel(const double* __restrict__ partials, long nblk,
                                                                     long n, int terms, double beta,
                                                                     float* __restrict__ lam, double* record) {
  __shared__ double red[kUpdThreads][6];
  const int tid = threadIdx.x;
  strided_tree_fold<kUpdThreads, FoldNanMax, FoldSum, FoldNanMax, FoldSum, FoldNanMax, FoldSum>(
      [&](long b, int c) { return partials[b * 6 + c]; }, nblk, red);
  if (tid != 0) return;
  const double P = (double)n;
  const double max_r = red[0][0];
  double rec[12];
  for (int c = 0; c < 12; ++c) rec[c] = record[c];
  rec[0] = max_r; rec[1] = red[0][1] / P;
  for (int t = 1; t < 3; ++t) {
    const int base = 2 + 3 * (t - 1);                   // 2 (boundary) or 5 (supervised)
    const double mean = red[0][2 * t + 1] / P;
    rec[base] = red[0][2 * t]; rec[base + 1] = mean;
    if (!((terms >> (t - 1)) & 1)) { rec[base + 2] = 0.0; continue; }
    const double lhat = max_r / mean;
    rec[base + 2] = lhat;
    if (mean == 0.0 || !isfinite(lhat)) { rec[8] += 1.0; continue; }
    rec[8 + t] = (1.0 - beta) * rec[8 + t] + beta * lhat;
  }
  rec[11] += 1.0;
  for (int c = 0; c < 12; ++c) record[c] = rec[c];
  lam[0] = (float)rec[9];
  lam[1] = (float)rec[10];
}

__global__ void balance_combine_kernel(float* g, const float* gr, const float* __restrict__ gb,
                                       const float* __restrict__ gs, const float* __restrict__ lam, long n) {
  const float lb = lam[0], ls = gs ? lam[1] : 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = fmaf(lb, gb[i], gr[i]);
    if (gs) v = fmaf(ls, gs[i], v);
    g[i] = v;
  }
}

}  // namespace

long balance_blocks(long n) { return (n + kBlk - 1) / kBlk; }

int launch_reduce_terms(const TermReduceArgs& a, hipStream_t s) {
  size_t P = flat_total(a.H, a.L, a.n_out);
  hipLaunchKernelGGL(reduce_terms_kernel, dim3((unsigned)((P + 63) / 64)), dim3(512), 0, s, a);
  return launch_status();
}

int launch_balance_stats(const float* v0, const float* v1, const float* v2, long n, double* partials, hipStream_t s) {
  hipLaunchKernelGGL(balance_stats_kernel, dim3((unsigned)balance_blocks(n)), dim3(kBlk), 0, s, v0, v1, v2, n, partials);
  return launch_status();
}

int launch_balance_update(const double* partials, long n, int terms, double beta, float* lam, double* record,
                          hipStream_t s) {
  hipLaunchKernelGGL(balance_update_kernel, dim3(1), dim3(kUpdThreads), 0, s, partials, balance_blocks(n), n, terms,
                     beta, lam, record);
  return launch_status();
}

int launch_balance_combine(float* g, const float* gr, const float* gb, const float* gs, const float* lam, long n,
                           hipStream_t s) {
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(balance_combine_kernel, dim3(blocks), dim3(256), 0, s, g, gr, gb, gs, lam, n);
  return launch_status();
}
