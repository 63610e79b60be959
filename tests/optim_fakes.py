"""CPU stand-ins for the schedule / clipping entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of the
oracle-backed fakes of tests/fakes.py ... rba_fakes.py: the scheduled update and the squared norm are the fp64 model
of tests/optim_model.py.  Nothing here is reachable from the product path."""
import dataclasses

import numpy as np
import torch

import fakes
import optim_model as om
import rba_fakes
from nsfnet_amd import engine as eng

CALLS = []           # (name, ...) of every fake optimizer entry point, in call order


class FakeDeviceNet(fakes.FakeDeviceNet):
    def adam_step(self, grads, lr, betas=(0.9, 0.999), eps=1e-8):
        CALLS.append(("adam_step", self.n_out, float(lr)))
        super().adam_step(grads, lr, betas, eps)

    def adam_step_sched(self, grads, lr0, opt, advance, betas=(0.9, 0.999), eps=1e-8):
        CALLS.append(("adam_step_sched", self.n_out, float(lr0), bool(advance)))
        e = int(opt.epoch[0])
        lr = np.float32(om.lr_e(lr0, e, **dataclasses.asdict(opt.spec)))
        norm, coef = 0.0, None
        if opt.max_norm > 0.0:
            norm, coef = om.clip(float(opt.scratch[0]), opt.max_norm)
        self.adam_t += 1
        p, m, v = om.update(self.params.numpy(), grads.numpy(), self.m.numpy(), self.v.numpy(), self.adam_t, lr, coef,
                            betas[0], betas[1], eps)
        for dst, src in ((self.params, p), (self.m, m), (self.v, v)):
            dst.copy_(torch.tensor(src, dtype=torch.float32))
        opt.rec[:4] = torch.tensor([e, float(lr), norm, 1.0 if coef is None else float(coef)], dtype=torch.float64)
        if advance:
            opt.epoch[0] = e + 1
            opt.rec[om.R_CLIPPED] += 1.0 if coef is not None and coef < 1.0 else 0.0
            opt.rec[om.R_UPDATES] += 1.0


def fake_grad_sqnorm_scratch(device):
    return torch.zeros(8, dtype=torch.float64)


def fake_grad_sqnorm(g0, g1, scratch):
    CALLS.append(("grad_sqnorm", g0.numel(), 0 if g1 is None else g1.numel()))
    scratch[0] = om.sqnorm(g0.numpy(), None if g1 is None else g1.numpy())


def install(monkeypatch=None):
    """rba_fakes.install plus the schedule / clipping entry points."""
    rba_fakes.install(monkeypatch)
    del CALLS[:]
    for name, val in [("DeviceNet", FakeDeviceNet), ("grad_sqnorm_scratch", fake_grad_sqnorm_scratch),
                      ("grad_sqnorm", fake_grad_sqnorm)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
