// Learning-rate schedules and gradient clipping for Adam (optim.hip): the schedule formula,
// shared by the update kernel and the host query, and the launch entry points.
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
