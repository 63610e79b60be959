"""GPU tests of the stochastic mini-batching of the collocation term: pinn_batch_draw and
pinn_batch_scatter against the integer model of tests/batch_model.py (exact), a batch of all points against today's
step (bitwise), a batch step against a plain step on the drawn points (bitwise), graph replay against eager (bitwise,
the draw counter advances inside the graph) and the draw after a resample."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import batch_model as bm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SHAPES = [(1000, 384), (1000, 100), (360000, 36000), (7, 7), (5, 1)]


def _store(n, seed=0):
    rng = np.random.RandomState(seed)
    return {k: torch.tensor(rng.rand(n).astype(np.float32), device=DEV) for k in ("x", "y", "w", "vtm")}


def _batch(b, keys):
    return {k: torch.full((b,), -7.0, dtype=torch.float32, device=DEV) for k in keys}


# ---------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("n,b", SHAPES)
@pytest.mark.parametrize("absent", [(), ("w",), ("vtm",), ("w", "vtm")])
def test_draw_matches_the_model_exactly(n, b, absent):
    from nsfnet_amd import engine as eng
    seed, rank = 0x1234567887654321, 3            # only the low 32 bits of the seed enter the key
    store = {k: v for k, v in _store(n).items() if k not in absent}
    runs = []
    for _ in range(2):
        counter = torch.zeros(2, dtype=torch.int64, device=DEV)
        idx = torch.full((b,), -1, dtype=torch.int64, device=DEV)
        batch = _batch(b, store.keys())
        rec = []
        for t in range(3):
            eng.batch_draw(store, batch, idx, n, b, seed, rank, counter)
            torch.cuda.synchronize()
            assert counter.cpu().tolist() == [t + 1, 0]
            ref = bm.draw(n, b, t, seed & 0xFFFFFFFF, rank)
            np.testing.assert_array_equal(idx.cpu().numpy(), ref)
            for k in store:
                assert torch.equal(batch[k], store[k][torch.as_tensor(ref, device=DEV)]), k
            rec.append([idx.cpu().numpy().copy()] + [batch[k].cpu().numpy().copy() for k in sorted(batch)])
        runs.append(rec)
    for ra, rb in zip(*runs):
        for a, c in zip(ra, rb):
            np.testing.assert_array_equal(a, c)


def test_draw_counter_high_word_enters_the_counter():
    from nsfnet_amd import engine as eng
    n, b = 1000, 100
    store = _store(n)
    batch = _batch(b, store.keys())
    idx = torch.zeros(b, dtype=torch.int64, device=DEV)
    t0 = (5 << 32) + 9
    counter = torch.tensor([t0, 0], dtype=torch.int64, device=DEV)
    eng.batch_draw(store, batch, idx, n, b, 1, 0, counter)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx.cpu().numpy(), bm.draw(n, b, t0, 1, 0))
    assert counter.cpu().tolist() == [t0 + 1, 0]


@pytest.mark.parametrize("n,b", SHAPES)
def test_scatter_writes_exactly_idx(n, b):
    from nsfnet_amd import engine as eng
    store = torch.tensor(np.random.RandomState(1).rand(n).astype(np.float32), device=DEV)
    before = store.cpu().numpy().copy()
    idx = bm.draw(n, b, 4, 2, 0)
    vals = torch.tensor(10.0 + np.arange(b, dtype=np.float32), device=DEV)
    eng.batch_scatter(torch.as_tensor(idx, device=DEV), b, n, vals, store)
    torch.cuda.synchronize()
    want = before.copy()
    want[idx] = vals.cpu().numpy()
    np.testing.assert_array_equal(store.cpu().numpy(), want)


def test_c_abi_refuses_bad_arguments():
    from nsfnet_amd import _lib
    lib = _lib.load()
    assert lib.pinn_abi_version() == 3
    s = _store(10)
    bt = _batch(4, s.keys())
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    c = torch.zeros(2, dtype=torch.int64, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    args = lambda n, b, sw, dw: (n, b, 0, 0, p(c), p(s["x"]), p(s["y"]), p(sw), p(s["vtm"]), p(bt["x"]), p(bt["y"]), p(dw),
                                 p(bt["vtm"]), p(idx), None)
    assert lib.pinn_batch_draw(*args(10, 11, s["w"], bt["w"])) != 0          # b > n
    assert lib.pinn_batch_draw(*args(10, 0, s["w"], bt["w"])) != 0
    assert lib.pinn_batch_draw(*args(10, 4, s["w"], None)) != 0              # w on one side only
    torch.cuda.synchronize()
    assert c.cpu().tolist() == [0, 0]


# ---------------------------------------------------------------- engines
def _bc(every=16):
    return tuple(a.reshape(-1)[::every].astype(np.float32) for a in ar.cavity_boundary())


def _points(n, seed=5):
    rng = np.random.RandomState(seed)
    return (rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32), (0.5 + rng.rand(n)).astype(np.float32))


def _engine(flavour, L, H, prec, x, y, w, seed=5):
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=2, hidden_e=24, alpha_evm=0.05) if flavour == "ev" else {}
    E = eng.PinnEngine(DEV, L, H, 2000.0, alpha_b=10.0, alpha_e=1.0, precision=prec, **ev)
    E.net.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().copy()))
    if flavour == "ev":
        E.net_e.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(1, 2, 24, seed=seed + 1)).numpy().copy()))
    E.set_collocation(x, y, weights=w)
    E.set_boundary(*_bc())
    return E


def _state(E):
    torch.cuda.synchronize()
    out = [E.net.params, E.net.m, E.net.v]
    if E.net_e is not None:
        out += [E.net_e.params, E.net_e.m, E.net_e.v, E.plan_f.vis_t_minus]
    return [t.cpu().numpy().copy() for t in out]


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
@pytest.mark.parametrize("L,H,prec", [(3, 24, "fp32"), (6, 256, "bf16x3")])
def test_batch_of_all_points_is_todays_step_bitwise(flavour, L, H, prec, monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    N = 2000
    x, y, w = _points(N)
    res = []
    for batching in (False, True):
        E = _engine(flavour, L, H, prec, x, y, w if flavour == "ev" else None)
        if batching:
            E.set_batching(N, seed=3)
        for k in range(5):
            E.e_trainable = flavour == "ev" and k == 2       # one step with the entropy net in the gradient
            E.step(1e-3)
        if batching:
            assert torch.equal(E.batch_indices(), torch.arange(N, device=DEV))
            assert E.batch_info()["draws"] == 5
        res.append(_state(E) + [E.sums.cpu().numpy().copy()])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
@pytest.mark.parametrize("L,H,prec", [(3, 24, "fp32"), (6, 256, "bf16x3")])
def test_batch_step_is_a_plain_step_on_the_drawn_points_bitwise(flavour, L, H, prec, monkeypatch):
    """Equal inputs on an equal plan size: the kernels reduce in a fixed order, so the bits must agree."""
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    N, B = 2000, 384
    x, y, w = _points(N)
    E = _engine(flavour, L, H, prec, x, y, w)
    E.e_trainable = flavour == "ev"
    E.set_batching(B, seed=11)
    E.step(1e-3)                                              # the second batch meets a store some points of which were visited
    store_vtm = None if flavour != "ev" else E.plan_f.vis_t_minus.clone()
    params = E.net.params.clone()
    E.loss_and_grad()
    torch.cuda.synchronize()
    idx = E.batch_indices().cpu().numpy()
    np.testing.assert_array_equal(idx, bm.draw(N, B, 1, 11, 0))
    R = _engine(flavour, L, H, prec, x[idx], y[idx], w[idx])
    R.e_trainable = E.e_trainable
    R.net.set_flat(params.cpu())
    if flavour == "ev":
        R.net_e.set_flat(E.net_e.params.cpu())
        R.plan_f.vis_t_minus.copy_(store_vtm[torch.as_tensor(idx, device=DEV)])
    R.loss_and_grad()
    torch.cuda.synchronize()
    assert torch.equal(E.sums, R.sums)
    assert torch.equal(E.grads, R.grads)
    assert torch.equal(E.grads_e, R.grads_e)
    for k in E.loss_terms():
        assert float(E.loss_terms()[k]) == float(R.loss_terms()[k]), k
    f, _ = E.eval_plans()
    assert torch.equal(f.field("eq1"), R.plan_f.field("eq1"))
    if flavour == "ev":                                       # the scatter: R's new state at idx, the rest untouched
        want = store_vtm.clone()
        want[torch.as_tensor(idx, device=DEV)] = R.plan_f.vis_t_minus
        assert torch.equal(E.plan_f.vis_t_minus, want)


@pytest.mark.parametrize("flavour,balance", [("nsfnet", False), ("ev", False), ("ev", True)])
def test_graph_replay_draws_a_new_batch_every_step_bitwise(flavour, balance, monkeypatch):
    N, B = 2000, 250
    x, y, w = _points(N)

    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E = _engine(flavour, 3, 24, "fp32", x, y, w)
        if balance:
            E.set_loss_balancing(2, 0.3)
        E.set_batching(B, seed=8)
        idxs = []
        for _ in range(6):
            E.step(1e-3)
            torch.cuda.synchronize()
            idxs.append(E.batch_indices().cpu().numpy().copy())
        if graph:
            assert len(E._graphs) == (2 if balance else 1)
        assert E.batch_info()["draws"] == 6
        return _state(E) + idxs + ([E.loss_weights().cpu().numpy()] if balance else [])

    eager, graph = run(False), run(True)
    for a, b in zip(eager, graph):
        np.testing.assert_array_equal(a, b)
    idxs = eager[-7:-1] if balance else eager[-6:]
    for t, i in enumerate(idxs):
        np.testing.assert_array_equal(i, bm.draw(N, B, t, 8, 0))


def test_after_a_resample_the_batch_comes_from_the_new_store(monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    N, B = 2000, 200
    x, y, w = _points(N)
    E = _engine("ev", 3, 24, "fp32", x, y, w)
    E.set_batching(B, seed=2)
    E.step(1e-3)
    xp, yp, wp = _points(6000, seed=9)
    E.set_resample_pool(xp, yp, weights=wp)
    E.resample(seed=4)
    xs, ys, ws = (t.clone() for t in E.collocation_points())
    assert xs.numel() == N and not torch.equal(xs, torch.as_tensor(x, device=DEV))
    vtm = E.plan_f.vis_t_minus.clone()
    E.loss_and_grad()
    torch.cuda.synchronize()
    idx = E.batch_indices()
    np.testing.assert_array_equal(idx.cpu().numpy(), bm.draw(N, B, 1, 2, 0))      # the counter carried on
    f, pe = E.eval_plans()
    assert torch.equal(f.x, xs[idx]) and torch.equal(f.y, ys[idx]) and torch.equal(f.w, ws[idx])
    assert pe.x.data_ptr() == f.x.data_ptr()
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert torch.equal(E.plan_f.vis_t_minus[rest], vtm[rest])
