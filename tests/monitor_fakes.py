"""CPU stand-ins for the convergence-monitor entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of
tests/state_fakes.py (and with it val_fakes.py, rwf_fakes.py ...): both launches are the fp64 model of
tests/monitor_model.py applied to the tensors of the fake plans, and both are logged into the shared CALLS, so a test
can read where they sit in a step.  Nothing here is reachable from the product path."""
import numpy as np
import torch

import monitor_model as mm
import state_fakes
import val_fakes
from nsfnet_amd import engine as eng

CALLS = val_fakes.CALLS


def fake_monitor_scratch(device):
    return torch.zeros(8, dtype=torch.float64)


def fake_monitor_vis_stats(vis_t, n, vis_t0, sum_out, info, scratch):
    CALLS.append(("monitor_vis_stats", int(n)))
    slot, words = mm.vis_stats(vis_t[:n].numpy(), np.float32(vis_t0))
    sum_out[0] = float(slot)
    info.copy_(torch.tensor(words, dtype=torch.float64))


def _config(cfg):
    return mm.Config(every=cfg.every, window=cfg.window, patience=cfg.patience, min_updates=cfg.min_updates,
                     min_rel_improvement=cfg.min_rel_improvement if cfg.plateau_on else None,
                     re_eff_tol=cfg.re_eff_tol if cfg.re_eff_on else None,
                     quantity={v: k for k, v in mm.QUANTITIES.items()}[cfg.quantity], capacity=cfg.capacity, ev=bool(cfg.ev))


def fake_monitor_observe(eq, bc, sup, lam, alpha_b, alpha_s, alpha_e, w4, n_eq, n_b, n_s, n_p, Re, cfg, state, ring):
    CALLS.append(("monitor_observe", int(cfg.every)))
    st, rg = state.numpy().copy(), ring.numpy().copy()
    mm.observe(_config(cfg), st, rg, eq.numpy(), bc.numpy(), None if sup is None else sup.numpy(),
               None if lam is None else lam.numpy(), alpha_b, alpha_s, alpha_e, w4, n_eq, n_b, n_s, n_p, Re)
    state.copy_(torch.tensor(st)); ring.copy_(torch.tensor(rg))


def install(monkeypatch=None, base=val_fakes):
    """state_fakes.install plus the monitor entry points."""
    state_fakes.install(monkeypatch, base)
    for name, val in [("monitor_scratch", fake_monitor_scratch), ("monitor_vis_stats", fake_monitor_vis_stats),
                      ("monitor_observe", fake_monitor_observe)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
