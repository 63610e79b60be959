"""CPU stand-ins for the training-state entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of any of the
other fakes: state_pack / state_unpack are the numpy model of tests/state_model.py on CPU tensors, and the L-BFGS
history stand-in gains the flat workspace tensor the engine snapshots.  The host-only entry points (layout, host
digest) stay the real library's.  Nothing here is reachable from the product path."""
import numpy as np
import torch

import lbfgs_model
import state_model as sm
import val_fakes
from nsfnet_amd import engine as eng

CALLS = []           # ("state_pack" | "state_unpack", number of segments), in call order


def _raw(t):
    return t.detach().contiguous().numpy().reshape(-1).view(np.uint8)


def _put_digests(digests, rows):
    digests.copy_(torch.from_numpy(np.array(rows, dtype=np.uint64).reshape(-1, 2).view(np.int64)))


def fake_state_scratch(device):
    return torch.zeros(4, dtype=torch.float64)


def fake_state_pack(srcs, offsets, staging, digests, scratch):
    CALLS.append(("state_pack", len(srcs)))
    out = None if staging is None else staging.numpy()
    rows = []
    for t, o in zip(srcs, offsets):
        raw = _raw(t)
        rows.append(sm.digest(raw))
        if o >= 0:
            out[o:o + raw.size] = raw
            out[o + raw.size:sm.align256(o + raw.size)] = 0
    _put_digests(digests, rows)


def fake_state_unpack(staging, offsets, dsts, digests, scratch):
    CALLS.append(("state_unpack", len(dsts)))
    src = None if staging is None else staging.numpy()
    rows = []
    for t, o in zip(dsts, offsets):
        if o >= 0:
            n = t.numel() * t.element_size()
            _raw_view = t.numpy().reshape(-1).view(np.uint8)       # in place: the live tensor keeps its storage
            _raw_view[:] = src[o:o + n]
            if hasattr(t, "_restored"):
                t._restored()
        rows.append(sm.digest(_raw(t)))
    _put_digests(digests, rows)


class StateModelHistory(lbfgs_model.ModelHistory):
    """ModelHistory whose model state is also a flat fp64 tensor `ws`, refreshed from the model when it is read and
    pushed back into the model when an unpack has written it."""

    def __init__(self, n, history_size, device):
        super().__init__(n, history_size, device)
        m = self.model
        self._parts = [("S", m.S.shape), ("Y", m.Y.shape), ("R", m.R.shape), ("YY", m.YY.shape), ("g_prev", m.g_prev.shape),
                       ("d", m.d.shape)]
        self._ws = torch.zeros(sum(int(np.prod(s)) for _, s in self._parts) + self.history_size + 8, dtype=torch.float64)
        self._ws._restored = self._load

    @property
    def ws(self):
        m = self.model
        tail = np.full(self.history_size + 8, -1.0)
        tail[:5] = [len(m.order), m.staging, m.gamma, m.accepted, m.ys]
        tail[8:8 + len(m.order)] = m.order
        flat = np.concatenate([np.asarray(getattr(m, k), dtype=np.float64).reshape(-1) for k, _ in self._parts] + [tail])
        self._ws.copy_(torch.from_numpy(flat))
        return self._ws

    def _load(self):
        m, flat, off = self.model, self._ws.numpy(), 0
        for k, shape in self._parts:
            n = int(np.prod(shape))
            setattr(m, k, flat[off:off + n].reshape(shape).copy())
            off += n
        tail = flat[off:]
        m.staging, m.gamma, m.accepted, m.ys = int(tail[1]), float(tail[2]), int(tail[3]), float(tail[4])
        m.order = [int(v) for v in tail[8:8 + int(tail[0])]]


def install(monkeypatch=None, base=val_fakes):
    """base.install plus the training-state entry points."""
    base.install(monkeypatch)
    del CALLS[:]
    for name, val in [("state_scratch", fake_state_scratch), ("state_pack", fake_state_pack),
                      ("state_unpack", fake_state_unpack), ("LbfgsHistory", StateModelHistory)]:
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)
