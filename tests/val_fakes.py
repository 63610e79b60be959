"""CPU stand-ins for the validation entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of
tests/rwf_fakes.py (and with it optim_fakes.py, rba_fakes.py ...): the statistics, the record and the state update are
the fp64 model of tests/val_model.py applied to the planes of the fake plans, the keep is a conditional copy.  Both are
logged into optim_fakes.CALLS, so a test can read where a validation sits in a step.  Nothing here is reachable from
the product path."""
import numpy as np
import torch

import rwf_fakes
import rwf_model
import val_model as vm
from nsfnet_amd import engine as eng

CALLS = rwf_fakes.CALLS


class FakeDeviceNet(rwf_fakes.FakeDeviceNet):
    def composed(self, x):
        if self.theta is None:
            return x.clone()
        return torch.tensor(rwf_model.compose(x.numpy(), self._shape()))


def fake_val_scratch(device):
    return torch.zeros(16, dtype=torch.float64)


def fake_val_planes(n, device):
    return torch.zeros(3, (int(n) + 3) // 4 * 4, dtype=torch.float32)


def fake_val_stats(pred, tgt, n, with_p, metric, t, every, scratch, state, ring):
    CALLS.append(("val_stats", int(n), int(metric), float(t), int(every)))
    rows = 3 if with_p else 2
    name = {v: k for k, v in vm.METRICS.items()}[int(metric)]
    p = [pred[c, :n].numpy() if c < rows else None for c in range(3)]
    g = [tgt[c, :n].numpy() if c < rows else None for c in range(3)]
    S = vm.sums(p, g)
    scratch[1:12] = torch.tensor(S, dtype=torch.float64)
    st, rg = state.numpy().copy(), ring.numpy().copy()
    vm.record(S, name, t, every, st, rg)
    state.copy_(torch.tensor(st)); ring.copy_(torch.tensor(rg))


def fake_val_keep(segs, state):
    CALLS.append(("val_keep", tuple(s.numel() for s, _ in segs)))
    if float(state[vm.S_IMPROVED]) == 1.0:
        for s, d in segs:
            d.copy_(s)


def install(monkeypatch=None):
    """rwf_fakes.install plus the validation entry points."""
    rwf_fakes.install(monkeypatch)
    for name, val in [("DeviceNet", FakeDeviceNet), ("val_scratch", fake_val_scratch), ("val_planes", fake_val_planes),
                      ("val_stats", fake_val_stats), ("val_keep", fake_val_keep)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
