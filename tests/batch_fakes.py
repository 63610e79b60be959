"""CPU stand-ins for the mini-batching entry points of nsfnet_amd.engine (TEST INFRASTRUCTURE), on top of the
oracle-backed fakes of tests/fakes.py and tests/balance_fakes.py: the draw is the integer model of
tests/batch_model.py, gather and scatter are numpy indexing; the L-BFGS history is the model of tests/lbfgs_model.py.  Nothing here is reachable from the product path."""
import torch

import balance_fakes
import batch_model as bm
import lbfgs_model
from nsfnet_amd import engine as eng


def fake_batch_draw(store, batch, idx, n, b, seed, rank, counter):
    assert int(counter[1]) == 0
    i = torch.as_tensor(bm.draw(n, b, int(counter[0]), seed, rank))
    idx.copy_(i)
    for k in ("x", "y", "w", "vtm"):
        assert (store.get(k) is None) == (batch.get(k) is None), k
        if store.get(k) is not None:
            batch[k].copy_(store[k][i])
    counter[0] += 1


def fake_batch_scatter(idx, b, n, batch_vtm, store_vtm):
    assert idx.numel() == b and store_vtm.numel() == n
    store_vtm[idx] = batch_vtm


def install(monkeypatch=None):
    """balance_fakes.install (fakes.install plus the balancing entry points) plus the batching entry points and the L-BFGS history."""
    balance_fakes.install(monkeypatch)
    for mod, name, val in [(eng, "batch_draw", fake_batch_draw), (eng, "batch_scatter", fake_batch_scatter),
                           (eng, "LbfgsHistory", lbfgs_model.ModelHistory)]:
        if monkeypatch is not None:
            monkeypatch.setattr(mod, name, val)
        else:
            setattr(mod, name, val)
