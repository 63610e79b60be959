// Learning-rate schedules and gradient clipping for Adam (optim.hip): the schedule formula,
// shared by the update kernel and the host query, the one Adam update body of adam_kernel, adam_dev_kernel (misc.hip)
// and adam_sched_kernel (optim.hip), and the launch entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/nsfnet_pinn.h"

// lr_e of include/nsfnet_pinn.h: fp64 operations in the order written, none contracted, so that the host and the
// device differ by what their pow / cos differ and by nothing else.
__host__ __device__ inline double lr_schedule_value(const pinn_lr_schedule_t& s, double lr0, long long e) {
#pragma clang fp contract(off)
  const double ed = (double)e;
  double lr = lr0;
  if (s.kind == PINN_LR_MULTISTEP) {
    int k = 0;
    for (int i = 0; i < s.n_milestones; ++i) k += s.milestones[i] <= e ? 1 : 0;
    lr = lr0 * pow(s.gamma, (double)k);
  } else if (s.kind == PINN_LR_STEP) {
    lr = lr0 * pow(s.gamma, (double)(e / s.step_size));
  } else if (s.kind == PINN_LR_EXPONENTIAL) {
    lr = lr0 * pow(s.gamma, ed);
  } else if (s.kind == PINN_LR_COSINE) {
    lr = s.eta_min + (lr0 - s.eta_min) * (1.0 + cos(3.14159265358979323846 * ed / (double)s.t_max)) / 2.0;
  }
  if (s.warmup_epochs > 0) {
    const double w = (double)(e < s.warmup_epochs ? e : s.warmup_epochs) / (double)s.warmup_epochs;
    lr = lr * (s.warmup_start + (1.0 - s.warmup_start) * w);
  }
  return lr;
}

// g * coef as one rounded fp32 multiply, whatever consumes the product: what the caller's own `grads * coef` gives
__device__ __forceinline__ float scaled(float g, float coef) {
#pragma clang fp contract(off)
  const float r = g * coef;
  return r;
}

// Adam's bias corrections for update t + 1, t read from device memory: step_size = lr / (1 - b1^t), sqrt(1 - b2^t)
__device__ __forceinline__ void adam_bias_correction(float lr, float b1, float b2, const long long* step_counter,
                                                     float& step_size, float& bc2_sqrt) {
  const double t = (double)(__atomic_load_n(step_counter, __ATOMIC_RELAXED) + 1);
  const double bc1 = 1.0 - pow((double)b1, t), bc2 = 1.0 - pow((double)b2, t);
  step_size = (float)((double)lr / bc1);
  bc2_sqrt = (float)sqrt(bc2);
}

// torch.optim.Adam single-tensor semantics (weight_decay = 0, amsgrad = False) on entries first, first + stride, ... < n
// (the kernel hands its thread's grid-stride range in: blockDim read there is the launch's uniform one); CLIP: the
// gradient is scaled by coef first.
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)
template <bool CLIP>
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, long first, long stride, long n, float step_size,
                                            float b1, float b2, float eps, float bc2_sqrt, float coef = 1.f) {
  for (long i = first; i < n; i += stride) {
    float gi = CLIP ? scaled(g[i], coef) : g[i];
    float mi = m[i] + (gi - m[i]) * (1.f - b1);           // torch: exp_avg.lerp_(grad, 1-beta1)
    float vi = v[i] * b2 + (1.f - b2) * gi * gi;           // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] - step_size * (mi / denom);
    m[i] = mi; v[i] = vi;
  }
}

struct AdamSchedArgs {
  float* p;
  const float* g;
  float *m, *v;
  long n;
  pinn_lr_schedule_t sched;
  double lr0;
  float b1, b2, eps;
  long long* step_counter;                 // [t, ticket]
  long long* epoch;                        // [e]
  int advance;
  const double* sq;                        // squared gradient norm; NULL = no clipping
  double max_norm;
  double* record;                          // [PINN_OPTIM_RECORD]
};
size_t grad_sqnorm_scratch_bytes();
int launch_grad_sqnorm(const float* g0, long n0, const float* g1, long n1, double* scratch, hipStream_t s);
int launch_adam_sched(const AdamSchedArgs& a, hipStream_t s);
