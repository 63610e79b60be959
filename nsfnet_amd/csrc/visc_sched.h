// Reynolds-number continuation (visc_sched.hip): the schedule formula of
// include/nsfnet_pinn.h, shared by the step kernel and the host query pinn_visc_schedule_value.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/nsfnet_pinn.h"

struct ViscRampValue {
  double s, re;          // the ramp coordinate and Re_t
  float nu, cap;         // what the residual launches read (cap 0 without cap_factor)
  int done;              // s >= 1
};

// fp64 operations in the order written, none contracted, so that the host and the device differ by what their exp / log
// differ and by nothing else - and the linear shapes by nothing at all.  The ends are selected, not computed.
__host__ __device__ inline ViscRampValue visc_schedule_value(const pinn_visc_schedule_t& c, long long t) {
#pragma clang fp contract(off)
  ViscRampValue r;
  const long long d = t - (long long)c.hold;
  double s = d <= 0 ? 0.0 : (d >= (long long)c.updates ? 1.0 : (double)d / (double)c.updates);
  if (c.stairs > 0 && s < 1.0) {
    const double k = (double)c.stairs;
    const double sk = s * k;
    s = floor(sk) / k;
  }
  const bool with_cap = c.cap_factor > 0.0;
  r.s = s; r.done = s >= 1.0 ? 1 : 0;
  if (s <= 0.0) {
    r.nu = c.nu_start; r.cap = with_cap ? c.cap_start : 0.f; r.re = c.re_start;
    return r;
  }
  if (s >= 1.0) {
    r.nu = c.nu_end; r.cap = with_cap ? c.cap_end : 0.f; r.re = c.re_end;
    return r;
  }
  const double n0 = (double)c.nu_start, n1 = (double)c.nu_end;
  double nu;
  if (c.shape == PINN_RAMP_LINEAR_RE) {
    const double r0 = 1.0 / n0, r1 = 1.0 / n1;
    const double dr = r1 - r0;
    const double sr = s * dr;
    const double re = r0 + sr;
    nu = 1.0 / re;
  } else if (c.shape == PINN_RAMP_LINEAR_NU) {
    const double dn = n1 - n0;
    const double sn = s * dn;
    nu = n0 + sn;
  } else {
    const double l0 = log(n0), l1 = log(n1);
    const double dl = l1 - l0;
    const double sl = s * dl;
    const double l = l0 + sl;
    nu = exp(l);
  }
  const double nlo = n0 < n1 ? n0 : n1, nhi = n0 < n1 ? n1 : n0;
  nu = nu < nlo ? nlo : nu;
  nu = nu > nhi ? nhi : nu;
  r.nu = (float)nu;
  r.re = 1.0 / nu;
  r.cap = 0.f;
  if (with_cap) {
    const double c0 = (double)c.cap_start, c1 = (double)c.cap_end;
    const double clo = c0 < c1 ? c0 : c1, chi = c0 < c1 ? c1 : c0;
    double cap = c.cap_factor * nu;
    cap = cap < clo ? clo : cap;
    cap = cap > chi ? chi : cap;
    r.cap = (float)cap;
  }
  return r;
}

struct ViscSchedArgs {
  pinn_visc_schedule_t sched;
  long long* pos;        // updates made so far (in/out)
  float* nu_dev;         // the fp32 the sweeps read in place of 1 / Re
  float* cap_dev;        // the fp32 the forward sweeps read in place of vis_t0, or null
  double* record;        // [PINN_RAMP_RECORD]
};
int launch_visc_sched(const ViscSchedArgs& a, hipStream_t s);

// the record of include/nsfnet_pinn.h (PINN_RAMP_RECORD doubles) for position t
__host__ __device__ inline void visc_schedule_record(const ViscRampValue& r, long long t, double* rec) {
  rec[0] = (double)t; rec[1] = r.s; rec[2] = r.re; rec[3] = (double)r.nu; rec[4] = (double)r.cap; rec[5] = (double)r.done;
}
