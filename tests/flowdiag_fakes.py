"""CPU stand-ins for the flow-diagnostics entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of
tests/monitor_fakes.py (and with it state_fakes.py, val_fakes.py ...): both launches are the fp64 model of
tests/flowdiag_model.py applied to the field planes of the fake plan, and both are logged into the shared CALLS, so a
test can read where they sit in a step.  Nothing here is reachable from the product path."""
import torch

import flowdiag_model as fdm
import monitor_fakes
import val_fakes
from nsfnet_amd import engine as eng

CALLS = monitor_fakes.CALLS


def fake_flow_scratch(device):
    return torch.zeros(32, dtype=torch.float64)


def fake_flow_stream_function(fields, nx, ny, ys, psi):
    CALLS.append(("flow_stream_function", int(nx), int(ny)))
    psi.copy_(torch.tensor(fdm.stream_function(fields[fdm.U].numpy(), ys.numpy(), int(nx), int(ny))))


def fake_flow_stats(fields, nx, ny, xs, ys, psi, eps, t, every, scratch, state, ring):
    CALLS.append(("flow_stats", int(nx), int(ny), float(eps), float(t), int(every)))
    st, rg = state.numpy().copy(), ring.numpy().copy()
    fdm.stats(fields.numpy(), psi.numpy(), xs.numpy(), ys.numpy(), float(eps), float(t), int(every), st, rg)
    state.copy_(torch.tensor(st)); ring.copy_(torch.tensor(rg))


def install(monkeypatch=None, base=val_fakes):
    """monitor_fakes.install plus the flow-diagnostics entry points."""
    monitor_fakes.install(monkeypatch, base)
    for name, val in [("flow_scratch", fake_flow_scratch), ("flow_stream_function", fake_flow_stream_function),
                      ("flow_stats", fake_flow_stats)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
