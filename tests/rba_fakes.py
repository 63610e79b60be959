"""CPU stand-ins for the residual-attention entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of the
oracle-backed fakes of tests/fakes.py, balance_fakes.py and batch_fakes.py: statistics, update and fill are the fp64
model of tests/rba_model.py applied to the field planes of the fake plans.  Nothing here is reachable from the product
path."""
import numpy as np
import torch

import batch_fakes
import rba_model as rm
from nsfnet_amd import engine as eng

EQ = slice(eng.FLD["eq1"], eng.FLD["eq4"] + 1)


def _eq(plan):
    return plan.fields[EQ, :plan.n].numpy()


def fake_rba_scratch(n, device):
    return torch.zeros(8, dtype=torch.float64)


def fake_rba_stats(plan, w4, scratch):
    rmax, sums = rm.stats(_eq(plan), w4)
    scratch[0] = float("nan") if np.isnan(rmax) else rmax      # the positive quiet NaN
    scratch[1:5] = torch.tensor(sums, dtype=torch.float64)


def fake_rba_apply(plan, w4, gamma, eta, idx, s, lam, w, scratch, record):
    assert lam.numel() == w.numel() and (s is None or s.numel() == lam.numel())
    assert idx is not None or plan.n == lam.numel()
    l, wn, rec = rm.apply(_eq(plan), w4, gamma, eta, lam.numpy(), None if s is None else s.numpy(),
                          None if idx is None else idx.numpy(), rmax=float(scratch[0]), w=w.numpy(),
                          record=record.numpy())
    lam.copy_(torch.tensor(l)); w.copy_(torch.tensor(wn)); record.copy_(torch.tensor(rec))


def fake_rba_fill(init, s, lam, w):
    l, wn = rm.fill(lam.numel(), init, None if s is None else s.numpy())
    lam.copy_(torch.tensor(l)); w.copy_(torch.tensor(wn))


def install(monkeypatch=None):
    """batch_fakes.install plus the residual-attention entry points."""
    batch_fakes.install(monkeypatch)
    for name, val in [("rba_scratch", fake_rba_scratch), ("rba_stats", fake_rba_stats), ("rba_apply", fake_rba_apply),
                      ("rba_fill", fake_rba_fill)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
