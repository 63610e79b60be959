"""CPU stand-ins for the weight-factorization entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of
tests/optim_fakes.py: split, compose and the gradient transform are the model of tests/rwf_model.py, and the Adam
fakes run on theta.  Every entry point, the gradient assembly, the loss-balancing combine and prepare are logged into
optim_fakes.CALLS, so a test can read the order of a whole step.  Nothing here is reachable from the product path."""
import numpy as np
import torch

import optim_fakes
import rwf_model as rm
from nsfnet_amd import engine as eng

CALLS = optim_fakes.CALLS


class FakeDeviceNet(optim_fakes.FakeDeviceNet):
    def _shape(self):
        return (self.n_out, self.n_hidden, self.hidden)

    def prepare(self):
        CALLS.append(("prepare", self.n_out))

    def _rwf_split(self, s):
        CALLS.append(("rwf_split", self.n_out))
        self.theta.copy_(torch.tensor(rm.split(self.params.numpy(), s.numpy(), self._shape())))

    def compose(self):
        CALLS.append(("rwf_compose", self.n_out))
        self.params.copy_(torch.tensor(rm.compose(self.theta.numpy(), self._shape())))

    def rwf_grad(self, grads):
        CALLS.append(("rwf_grad", self.n_out))
        g, _ = rm.grad(self.theta.numpy(), grads.numpy(), self._shape())
        self.gtheta.copy_(torch.tensor(g.astype(np.float32)))
        return self.gtheta

    def _on_trainable(self, fn, *a, **k):
        """Run an Adam fake of the parent classes - they update self.params - on the trainable vector."""
        params = self.params
        self.params = self.trainable
        try:
            fn(*a, **k)
        finally:
            self.params = params
        self.update_params()

    def adam_step(self, grads, lr, betas=(0.9, 0.999), eps=1e-8):
        if self.theta is None:          # the parent fake as it is: no prepare, as before
            return super().adam_step(grads, lr, betas, eps)
        self._on_trainable(super().adam_step, grads, lr, betas, eps)

    def adam_step_sched(self, grads, lr0, opt, advance, betas=(0.9, 0.999), eps=1e-8):
        if self.theta is None:
            return super().adam_step_sched(grads, lr0, opt, advance, betas, eps)
        self._on_trainable(super().adam_step_sched, grads, lr0, opt, advance, betas, eps)


def _logged(name, fn):
    def wrapper(*a, **k):
        CALLS.append((name,))
        return fn(*a, **k)
    return wrapper


def install(monkeypatch=None):
    """optim_fakes.install plus the factorization: the net class, and logging wrappers around the gradient assembly and
    the combine."""
    optim_fakes.install(monkeypatch)
    repl = [("DeviceNet", FakeDeviceNet)] + [(n, _logged(n, getattr(eng, n)))
                                             for n in ("grad_reduce", "grad_reduce_terms", "balance_combine")]
    for name, val in repl:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
