// Random weight factorization of the dense layers (rwf.hip): the launch entry points.
#pragma once
#include <hip/hip_runtime.h>

// The net's geometry as the three kernels need it: L hidden layers of width H, n_out outputs.  Layer l = 0..L has
// rows(l) = (l < L ? H : n_out) rows of cols(l) = (l == 0 ? 2 : H) weights; R = L H + n_out rows in all.
struct RwfNet {
  int H, L, n_out;
};
inline long rwf_rows(const RwfNet& n) { return (long)n.L * n.H + n.n_out; }

int launch_rwf_split(const RwfNet& n, const float* params, const float* s, float* theta, hipStream_t st);
int launch_rwf_compose(const RwfNet& n, const float* theta, float* params, hipStream_t st);
int launch_rwf_grad(const RwfNet& n, const float* theta, const float* grads, float* gtheta, hipStream_t st);
