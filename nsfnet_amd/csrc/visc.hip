// Identification of the molecular viscosity nu = 1 / Re from data (include/nsfnet_pinn.h
// "Viscosity identification").  The residual sweeps read nu from device memory (FwdArgs::nu_dev) and leave the physical
// Laplacians Lap u, Lap v beside the field planes (FwdArgs::lap); nu enters the residuals as eq1 = ... - nu Lap u,
// eq2 = ... - nu Lap v, eq4 = eq1 (u - 1/2) + eq2 (v - 1/2) - e, so with loss_e = (alpha_e / N) sum_i w_i (eq1^2 + eq2^2 +
// eq3^2 + w4 eq4^2) (the lagged artificial viscosity does not depend on nu)
//   d loss / d nu = -(2 alpha_e / N) S,   S = sum_i t_i,
//   t_i = w_i ((eq1 + w4 eq4 (u - 1/2)) Lap u + (eq2 + w4 eq4 (v - 1/2)) Lap v).
// Two launches, both inside the captured step, nothing synchronises:
//   visc_grad_kernel    S over the planes of the evaluation, per point in fp64 from the fp32 planes, one rounding per
//                       operation in this order, without contraction:
//                         a1 = eq1 + (w4 eq4) (u - 1/2)     a2 = eq2 + (w4 eq4) (v - 1/2)      (w4 = 0: a1 = eq1, a2 = eq2,
//                         t  = w (a1 Lap u + a2 Lap v)                                          the eq4 plane is not read)
//                       rounded once to fp32 into a slot of the loss-sum block, so that the all-reduce that is sent
//                       anyway makes it global.  Grid-stride loop of 16-byte loads, block_fold, per-block partials, the
//                       last block folds them by strided_tree_fold.  No float atomics, a fixed order (fixed_fold.h).
//   visc_update_kernel  one workgroup, after the nets' updates.  s = (double)*sum; a non-finite s raises state[7] and
//                       changes nothing else.  Otherwise, everything fp64, one rounding per operation in this order:
//                         G = coef s                      (coef = -2 alpha_e / N, a launch constant)
//                         g = (double)*nu_dev G           (the chain rule onto theta = ln nu, at the nu the sweep read)
//                         p1 = p1 beta1, p2 = p2 beta2    (the running products beta^t: no pow)
//                         m = beta1 m + (1 - beta1) g     v = beta2 v + ((1 - beta2) g) g
//                         theta = theta - (lr / (1 - p1)) (m / (sqrt(v) / sqrt(1 - p2) + eps))
//                         theta = min(max(theta, theta_min), theta_max)      *nu_dev = (float)exp(theta)
// state, in doubles (PINN_VISC_STATE): theta, m, v, beta1^t, beta2^t, t, the last G, skipped.
#include "fixed_fold.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                            // points per thread and iteration: one 16-byte load per plane
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBlocks = 512;                    // grid cap: beyond kMaxBlocks * kTile points the loop repeats
// scratch, in doubles: [0] ticket [1..7] - [8..] partials [kMaxBlocks]
constexpr int kTicket = 0, kPart = 8;
constexpr int kScratchDoubles = kPart + kMaxBlocks;
// state, in doubles
constexpr int S_THETA = 0, S_M = 1, S_V = 2, S_P1 = 3, S_P2 = 4, S_T = 5, S_G = 6, S_SKIPPED = 7;

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__global__ __launch_bounds__(kThreads) void visc_grad_kernel(ViscGradArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[kThreads / 64];
  __shared__ int flag;
  const size_t np = (size_t)a.npad;
  const bool with4 = a.w4 != 0.0;
  double acc = 0.0;
  auto point = [&](float e1, float e2, float e4, float u, float v, float lu, float lv, float wf) {
    double a1 = (double)e1, a2 = (double)e2;
    if (with4) {
      const double c4 = a.w4 * (double)e4;
      const double du = (double)u - 0.5, dv = (double)v - 0.5;
      const double q1 = c4 * du, q2 = c4 * dv;
      a1 = a1 + q1; a2 = a2 + q2;
    }
    const double m1 = a1 * (double)lu, m2 = a2 * (double)lv;
    const double s = m1 + m2;
    const double t = (double)wf * s;
    acc = acc + t;
  };
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < a.n; base += (long)gridDim.x * kTile) {
    // base % 4 == 0 and base < n <= npad, npad % 4 == 0: the quads of the planes are in bounds
    const float4 e1 = load4(a.fld + FLD_EQ1 * np + base), e2 = load4(a.fld + FLD_EQ2 * np + base);
    const float4 lu = load4(a.lap + base), lv = load4(a.lap + np + base);
    float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f), u = e4, v = e4;
    if (with4) {
      e4 = load4(a.fld + FLD_EQ4 * np + base);
      u = load4(a.fld + FLD_U * np + base); v = load4(a.fld + FLD_V * np + base);
    }
    float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
    if (a.w) {
      if (base + kPer <= a.n) {
        w = load4(a.w + base);
      } else {                                     // the ragged tail: w has n entries
        w.x = a.w[base];
        if (base + 1 < a.n) w.y = a.w[base + 1];
        if (base + 2 < a.n) w.z = a.w[base + 2];
      }
    }
    point(e1.x, e2.x, e4.x, u.x, v.x, lu.x, lv.x, w.x);
    if (base + 1 < a.n) point(e1.y, e2.y, e4.y, u.y, v.y, lu.y, lv.y, w.y);
    if (base + 2 < a.n) point(e1.z, e2.z, e4.z, u.z, v.z, lu.z, lv.z, w.z);
    if (base + 3 < a.n) point(e1.w, e2.w, e4.w, u.w, v.w, lu.w, lv.w, w.w);
  }
  acc = block_fold<FoldSum, kThreads>(acc, red);
  double* part = a.scratch + kPart;
  if (threadIdx.x == 0) put(part + blockIdx.x, acc);
  if (!last_block(a.scratch + kTicket, &flag)) return;
  __shared__ double tree[kThreads][1];
  strided_tree_fold<kThreads, FoldSum>([&](long b, int) { return get(part + b); }, (long)gridDim.x, tree);
  if (threadIdx.x == 0) *a.sum_out = (float)tree[0][0];      // the one rounding to fp32
}

__device__ __forceinline__ bool finite64(double v) { return v == v && fabs(v) <= 1.79769313486231570815e308; }

__global__ __launch_bounds__(64) void visc_update_kernel(ViscUpdateArgs a) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  double* st = a.state;
  const double s = (double)*a.sum;
  if (!finite64(s)) {
    st[S_SKIPPED] += 1.0;
    return;
  }
  const double G = a.coef * s;
  const double g = (double)*a.nu_dev * G;
  const double p1 = st[S_P1] * a.beta1, p2 = st[S_P2] * a.beta2;
  const double c1 = 1.0 - a.beta1, c2 = 1.0 - a.beta2;
  const double m0 = a.beta1 * st[S_M], m1 = c1 * g;
  const double m = m0 + m1;
  const double v0 = a.beta2 * st[S_V], v1 = c2 * g;
  const double v2 = v1 * g;
  const double v = v0 + v2;
  const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
  const double step = __ddiv_rn(a.lr, bc1);
  const double r = __ddiv_rn(__dsqrt_rn(v), __dsqrt_rn(bc2));
  const double denom = r + a.eps;
  const double q = __ddiv_rn(m, denom);
  const double d = step * q;
  double theta = st[S_THETA] - d;
  theta = theta < a.theta_min ? a.theta_min : theta;
  theta = theta > a.theta_max ? a.theta_max : theta;
  st[S_THETA] = theta; st[S_M] = m; st[S_V] = v; st[S_P1] = p1; st[S_P2] = p2;
  st[S_T] += 1.0; st[S_G] = G;
  *a.nu_dev = (float)exp(theta);
}

}  // namespace

size_t visc_scratch_bytes(long) { return (size_t)kScratchDoubles * sizeof(double); }

int launch_visc_grad(const ViscGradArgs& a, hipStream_t s) {
  long blocks = (a.n + kTile - 1) / kTile;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(visc_grad_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  return launch_status();
}

int launch_visc_update(const ViscUpdateArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(visc_update_kernel, dim3(1), dim3(64), 0, s, a);
  return launch_status();
}
