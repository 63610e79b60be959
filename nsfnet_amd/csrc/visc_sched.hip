// Reynolds-number continuation (include/nsfnet_pinn.h "Reynolds-number continuation").  The
// residual sweeps read nu = 1 / Re - and, ev flavour, the cap vis_t0 of the artificial viscosity - from device memory
// (FwdArgs::nu_dev, cap_dev; kernels.h resolve_viscosity).  One launch after the nets' updates, inside the captured
// step, moves both along a ramp from a viscous start to the configured Re:
//   visc_sched_kernel   one workgroup, one lane.  t = *pos + 1 (int64) -> *pos; visc_schedule_value(t) (visc_sched.h:
//                       fp64, nothing contracted, the ends selected) -> *nu_dev, *cap_dev, record.  No atomics: the
//                       launches of one stream are ordered, and nothing else writes these words.
#include "kernels.h"
#include "visc_sched.h"

namespace {

__global__ __launch_bounds__(64) void visc_sched_kernel(ViscSchedArgs a) {
  if (threadIdx.x != 0) return;
  const long long t = *a.pos + 1;
  const ViscRampValue r = visc_schedule_value(a.sched, t);
  *a.pos = t;
  *a.nu_dev = r.nu;
  if (a.cap_dev) *a.cap_dev = r.cap;
  visc_schedule_record(r, t, a.record);
}

}  // namespace

int launch_visc_sched(const ViscSchedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(visc_sched_kernel, dim3(1), dim3(64), 0, s, a);
  return launch_status();
}
