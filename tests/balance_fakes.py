"""CPU stand-ins for the loss-balancing entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of the
oracle-backed fakes of tests/fakes.py: the term-split assembly sums each group's oracle gradients, the statistics,
update and combine are the fp64 model of tests/balance_model.py.  Nothing here is reachable from the product path."""
import numpy as np
import torch

import balance_model as bm
import fakes
from nsfnet_amd import engine as eng


def fake_grad_reduce_terms(net, groups, outs, acc_mask=0, partials=None):
    written = []
    for t, (grp, out) in enumerate(zip(groups, outs)):
        if out is None:
            assert not grp
            written.append(None)
            continue
        g = sum((p._grad for p in grp), np.zeros(out.numel()))
        v = torch.tensor(g, dtype=torch.float32)
        if (acc_mask >> t) & 1:
            out.add_(v)
        else:
            out.copy_(v)
        written.append(out.numpy().astype(np.float64))
    if partials is not None:
        n = outs[0].numel()
        partials.copy_(torch.tensor(bm.block_partials(written, n).reshape(-1)))


def fake_balance_partials(n, device):
    return torch.zeros(((n + bm.BLK - 1) // bm.BLK) * 6, dtype=torch.float64)


def fake_balance_stats(vecs, n, partials):
    partials.copy_(torch.tensor(bm.block_partials([None if v is None else v.numpy() for v in vecs], n).reshape(-1)))


def fake_balance_update(partials, n, terms, beta, lam, record):
    rec = bm.update(partials.numpy(), n, terms, beta, record.numpy())
    record.copy_(torch.tensor(rec))
    lam.copy_(torch.tensor([rec[9], rec[10]], dtype=torch.float32))


def fake_balance_combine(g, gr, gb, gs, lam):
    g.copy_(torch.tensor(bm.combine(gr.numpy(), gb.numpy(), None if gs is None else gs.numpy(), lam.numpy()),
                         dtype=torch.float32))


def install(monkeypatch=None):
    """fakes.install plus the balancing entry points."""
    fakes.install(monkeypatch)
    repl = [(eng, "grad_reduce_terms", fake_grad_reduce_terms), (eng, "balance_partials", fake_balance_partials),
            (eng, "balance_stats", fake_balance_stats), (eng, "balance_update", fake_balance_update),
            (eng, "balance_combine", fake_balance_combine)]
    for mod, name, val in repl:
        if monkeypatch is not None:
            monkeypatch.setattr(mod, name, val)
        else:
            setattr(mod, name, val)
