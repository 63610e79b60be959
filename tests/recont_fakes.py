"""CPU stand-ins for the Reynolds-number continuation entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top
of tests/visc_fakes.py: a residual plan that also reads the cap from the tensor it was handed, and the step launch as
the numpy statement of tests/recont_model.py, logged into the shared CALLS.  Nothing here is reachable from the product
path."""
import numpy as np
import torch

import recont_model as rm
import visc_fakes
from nsfnet_amd import engine as eng

CALLS = visc_fakes.CALLS
_SHAPE_NAMES = {v: k for k, v in rm.SHAPES.items()}


class RecontResidualPlan(visc_fakes.ViscResidualPlan):
    cap = None

    def set_viscosity(self, nu, with_lap=True):
        super().set_viscosity(nu, with_lap)
        self.cap = None                 # pinn_plan_set_viscosity drops the cap

    def set_viscosity_cap(self, cap):
        if cap is not None and self.nu is None:
            raise ValueError("cap_dev comes with nu_dev")
        self.cap = cap

    def forward(self, Re, e=None, vis_t0=0.0, alpha_evm=0.0, scale=1.0, save=True, sums_out=None):
        if self.cap is not None:        # the forward launches read *cap_dev in place of vis_t0
            vis_t0 = float(self.cap[0])
        super().forward(Re, e=e, vis_t0=vis_t0, alpha_evm=alpha_evm, scale=scale, save=save, sums_out=sums_out)


def constants(cs):
    """The recont_model constants of a _lib.ViscScheduleStruct."""
    return dict(shape=_SHAPE_NAMES[cs.shape], stairs=cs.stairs, hold=cs.hold, updates=cs.updates, re_start=cs.re_start,
                re_end=cs.re_end, cap_factor=cs.cap_factor, nu_start=np.float32(cs.nu_start), nu_end=np.float32(cs.nu_end),
                cap_start=np.float32(cs.cap_start), cap_end=np.float32(cs.cap_end))


def fake_visc_schedule_value(cstruct, t):
    return rm.value(constants(cstruct), t)


def fake_visc_schedule_step(cstruct, pos, nu, cap, rec):
    t = int(pos[0]) + 1
    CALLS.append(("visc_schedule_step", t))
    r = rm.value(constants(cstruct), t)
    pos[0] = t
    nu[0] = r[3]
    if cap is not None:
        cap[0] = r[4]
    rec.copy_(torch.tensor(r, dtype=torch.float64))


def install(monkeypatch=None):
    """visc_fakes.install plus the continuation entry points and the plan that carries the cap."""
    visc_fakes.install(monkeypatch)
    for name, val in [("ResidualPlan", RecontResidualPlan), ("visc_schedule_value", fake_visc_schedule_value),
                      ("visc_schedule_step", fake_visc_schedule_step)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
