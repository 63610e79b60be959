"""CPU stand-ins for the conflict-free-gradient entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of
tests/balance_fakes.py: the term-split assembly sums each group's oracle gradients and, on request, writes the Gram
partials of what it wrote; the statistics, coefficients and combine are the fp64 model of tests/confgrad_model.py.
Every entry point is logged into CALLS.  Nothing here is reachable from the product path."""
import numpy as np
import torch

import balance_fakes
import confgrad_model as cm
from nsfnet_amd import engine as eng

CALLS = []


def fake_grad_reduce_terms(net, groups, outs, acc_mask=0, partials=None, gram=None):
    CALLS.append("grad_reduce_terms_gram" if gram is not None else "grad_reduce_terms")
    balance_fakes.fake_grad_reduce_terms(net, groups, outs, acc_mask, partials)
    if gram is not None:
        n = outs[0].numel()
        gram.copy_(torch.tensor(cm.block_partials([None if o is None else o.numpy() for o in outs], n).reshape(-1)))


def fake_confgrad_partials(n, device):
    return torch.zeros(((n + cm.BLK - 1) // cm.BLK) * 6, dtype=torch.float64)


def fake_confgrad_gram(vecs, n, partials):
    CALLS.append("confgrad_gram")
    partials.copy_(torch.tensor(cm.block_partials([None if v is None else v.numpy() for v in vecs], n).reshape(-1)))


def fake_confgrad_coef(partials, n, nterms, coef, record):
    CALLS.append("confgrad_coef")
    rec = cm.coefficients(cm.sum_partials(partials.numpy()), nterms, record.numpy())
    record.copy_(torch.tensor(rec))
    coef.copy_(torch.tensor(rec[6:9], dtype=torch.float32))


def fake_confgrad_combine(g, gr, gb, gs, coef):
    CALLS.append("confgrad_combine")
    g.copy_(torch.tensor(cm.combine(gr.numpy(), gb.numpy(), None if gs is None else gs.numpy(), coef.numpy()),
                         dtype=torch.float32))


def install(monkeypatch=None):
    """balance_fakes.install plus the conflict-free-gradient entry points (and a logging gradient assembly)."""
    balance_fakes.install(monkeypatch)
    plain = eng.grad_reduce

    def logged_grad_reduce(*a, **k):
        CALLS.append("grad_reduce")
        return plain(*a, **k)

    repl = [(eng, "grad_reduce", logged_grad_reduce), (eng, "grad_reduce_terms", fake_grad_reduce_terms),
            (eng, "confgrad_partials", fake_confgrad_partials), (eng, "confgrad_gram", fake_confgrad_gram),
            (eng, "confgrad_coef", fake_confgrad_coef), (eng, "confgrad_combine", fake_confgrad_combine)]
    for mod, name, val in repl:
        if monkeypatch is not None:
            monkeypatch.setattr(mod, name, val)
        else:
            setattr(mod, name, val)
