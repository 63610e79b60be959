// Random weight factorization of the dense layers (Wang, Wang, Sankaran & Perdikaris 2022):
// every Linear layer's weight is W = diag(exp(s)) V with s and V trainable.  The factorisation lives between the
// optimizer and pinn_net_prepare: the optimizers update theta = [params with V where W stands | s], and three kernels
// of one launch each move between theta and the flat parameters the sweeps read:
//   rwf_split_kernel    V = W / g (one fp32 division), biases and s copied                    params, s -> theta
//   rwf_compose_kernel  W = g V (one rounded fp32 multiply), biases copied                    theta -> params
//   rwf_grad_kernel     dV = g G_W, db = G_b, ds_i = fp32(g_i sum_j V_ij G_ij)                theta, grads -> gtheta
// with g_i = fp32(exp((double) s_i)), rounded once, the same expression in all three.
// One wave handles one row of one layer (its weights, its bias and its scale): lane t takes the columns t, t + 64, ...
// ascending, so the accesses of a wave are contiguous.  The row sum of ds is fp64, not contracted, and combined over
// the lanes by a shuffle-down tree with offsets 32, 16, ..., 1: a fixed order, no atomics and no scratch.
#include "rwf.h"
#include "fixed_fold.h"
#include "layout.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct Row {
  size_t w, b;      // offsets of the row's first weight and of its bias in the flat vector
  int cols;
};

// row r = 0..R-1 counts the rows of layer 0, then layer 1, ...: the order of the scale factors behind the P parameters
__device__ __forceinline__ Row locate(const RwfNet& n, long r) {
  const int l = r < (long)n.L * n.H ? (int)(r / n.H) : n.L;
  const int i = (int)(r - (long)l * n.H);
  Row o;
  o.cols = l == 0 ? 2 : n.H;
  o.w = flat_w(n.H, l) + (size_t)i * o.cols;
  o.b = flat_b(n.H, l, n.L, n.n_out) + i;
  return o;
}

__device__ __forceinline__ float scale_of(float s) { return (float)exp((double)s); }

__device__ __forceinline__ float mul1(float a, float b) {
#pragma clang fp contract(off)
  const float r = a * b;
  return r;
}

__global__ __launch_bounds__(kThreads) void rwf_split_kernel(RwfNet n, const float* __restrict__ params,
                                                             const float* __restrict__ s, float* __restrict__ theta) {
  const long R = (long)n.L * n.H + n.n_out;
  const long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = threadIdx.x & 63;
  const Row row = locate(n, r);
  const float sr = s[r];
  const float g = scale_of(sr);
  for (int j = lane; j < row.cols; j += 64) theta[row.w + j] = params[row.w + j] / g;
  if (lane == 0) {
    theta[row.b] = params[row.b];
    theta[flat_total(n.H, n.L, n.n_out) + r] = sr;
  }
}

__global__ __launch_bounds__(kThreads) void rwf_compose_kernel(RwfNet n, const float* __restrict__ theta,
                                                               float* __restrict__ params) {
  const long R = (long)n.L * n.H + n.n_out;
  const long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= R) return;
  const int lane = threadIdx.x & 63;
  const Row row = locate(n, r);
  const float g = scale_of(theta[flat_total(n.H, n.L, n.n_out) + r]);
  for (int j = lane; j < row.cols; j += 64) params[row.w + j] = mul1(g, theta[row.w + j]);
  if (lane == 0) params[row.b] = theta[row.b];
}

__global__ __launch_bounds__(kThreads) void rwf_grad_kernel(RwfNet n, const float* __restrict__ theta,
                                                            const float* __restrict__ grads,
                                                            float* __restrict__ gtheta) {
#pragma clang fp contract(off)
  const long R = (long)n.L * n.H + n.n_out;
  const long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= R) return;      // whole waves leave: the shuffles below run in full waves only
  const int lane = threadIdx.x & 63;
  const Row row = locate(n, r);
  const size_t P = flat_total(n.H, n.L, n.n_out);
  const float g = scale_of(theta[P + r]);
  double acc = 0.0;
  for (int j = lane; j < row.cols; j += 64) {
    const float G = grads[row.w + j];
    acc += (double)theta[row.w + j] * (double)G;      // the product of two fp32 values is exact in fp64
    gtheta[row.w + j] = mul1(g, G);
  }
  acc = wave_fold<FoldSum>(acc);
  if (lane == 0) {
    gtheta[row.b] = grads[row.b];
    gtheta[P + r] = (float)((double)g * acc);
  }
}

unsigned blocks_of(const RwfNet& n) { return (unsigned)((rwf_rows(n) + kWaves - 1) / kWaves); }

}  // namespace

int launch_rwf_split(const RwfNet& n, const float* params, const float* s, float* theta, hipStream_t st) {
  hipLaunchKernelGGL(rwf_split_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, st, n, params, s, theta);
  return launch_status();
}

int launch_rwf_compose(const RwfNet& n, const float* theta, float* params, hipStream_t st) {
  hipLaunchKernelGGL(rwf_compose_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, st, n, theta, params);
  return launch_status();
}

int launch_rwf_grad(const RwfNet& n, const float* theta, const float* grads, float* gtheta, hipStream_t st) {
  hipLaunchKernelGGL(rwf_grad_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, st, n, theta, grads, gtheta);
  return launch_status();
}
