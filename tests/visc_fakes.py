"""CPU stand-ins for the viscosity-identification entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of
tests/monitor_fakes.py (and with it state_fakes.py, val_fakes.py ...): a residual plan that reads nu from the tensor it
was handed and leaves the Laplacian planes, and the two launches as the fp64 model of tests/visc_model.py, both logged
into the shared CALLS.  Nothing here is reachable from the product path."""
import numpy as np
import torch

import fakes
import monitor_fakes
import visc_model as vm
from nsfnet_amd import engine as eng
from oracle import fwdmode_ref as fr

CALLS = monitor_fakes.CALLS


class ViscResidualPlan(fakes.FakeResidualPlan):
    nu = lap = None

    def set_viscosity(self, nu, with_lap=True):
        self.nu = nu
        self.lap = torch.zeros(2, self.npad) if nu is not None and with_lap else None

    def forward(self, Re, e=None, vis_t0=0.0, alpha_evm=0.0, scale=1.0, save=True, sums_out=None):
        if self.nu is not None:     # the launches read *nu_dev in place of 1 / Re
            Re = 1.0 / float(self.nu[0])
        super().forward(Re, e=e, vis_t0=vis_t0, alpha_evm=alpha_evm, scale=scale, save=save, sums_out=sums_out)
        if self.lap is not None:
            out, _ = fr.forward4(self.net.pairs(), *self._xy())
            self.lap.zero_()
            self.lap[0, :self.n] = torch.tensor(out[:, 0, 3] * scale * scale, dtype=torch.float32)
            self.lap[1, :self.n] = torch.tensor(out[:, 1, 3] * scale * scale, dtype=torch.float32)


def fake_visc_scratch(n, device):
    return torch.zeros(8, dtype=torch.float64)


def fake_visc_grad(plan, w4, sum_out, scratch):
    CALLS.append(("visc_grad", int(plan.n)))
    d = lambda t: t[:plan.n].numpy().astype(np.float64)
    eqs = [d(plan.field("eq%d" % k)) for k in (1, 2, 3, 4)]
    t = vm.terms(eqs, d(plan.field("u")), d(plan.field("v")), (d(plan.lap[0]), d(plan.lap[1])),
                 None if plan.w is None else d(plan.w), float(w4))
    sum_out[0] = float(np.float32(np.sum(t)))


def fake_visc_update(sum_in, coef, lr, betas, eps, theta_bounds, state, nu):
    CALLS.append(("visc_update", float(coef)))
    st, new = vm.update(state.numpy().copy(), np.float32(nu[0].item()), np.float32(sum_in[0].item()), coef, lr,
                        betas[0], betas[1], eps, theta_bounds[0], theta_bounds[1])
    state.copy_(torch.tensor(st))
    nu[0] = float(new)


def install(monkeypatch=None):
    """monitor_fakes.install plus the viscosity entry points and the plan that carries nu."""
    monitor_fakes.install(monkeypatch)
    for name, val in [("ResidualPlan", ViscResidualPlan), ("visc_scratch", fake_visc_scratch),
                      ("visc_grad", fake_visc_grad), ("visc_update", fake_visc_update)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
