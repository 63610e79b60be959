"""The fused role-split sweeps (fwdbwd_bf16_split.hip, pinn_residual_forward_backward) give BIT-IDENTICAL results to
the forward + backward launches on the same plan: loss sums, field planes, vis_t, vis_t_minus, ebar and the reduced
gradient - at odd tile counts with a partial last tile, below two tiles per workgroup, at two and three layers, with the
ev flavour's inputs, per chunk of a chunked engine, under graph replay, and for a full 360 000-point engine step."""
import numpy as np
import pytest
import torch

from oracle import autograd_ref as ar

pytestmark = pytest.mark.gpu


def _clear_sched(monkeypatch):
    for k in ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_FUSE", "PINN_TILE_COLS", "NSFNET_GRAPH"):
        monkeypatch.delenv(k, raising=False)


def _plan_pair(L, H, n, prec, ev, seed=11):
    """Two identically prepared plans of one net: the split launches on one, the fused call on the other."""
    from nsfnet_amd import engine as eng
    dev = torch.device("cuda:0")
    net = eng.DeviceNet(3, L, H, dev, prec)
    net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=seed)))
    rng = np.random.RandomState(seed)
    x = rng.rand(n).astype(np.float32); y = rng.rand(n).astype(np.float32)
    w = (0.5 + rng.rand(n)).astype(np.float32) if ev else None
    plans = [eng.ResidualPlan(net, x, y, weights=w) for _ in range(2)]
    e = None
    if ev:
        e = torch.tensor(rng.randn(n).astype(np.float32) * 0.1, device=dev)
        vtm = torch.tensor(rng.rand(n).astype(np.float32) * 0.01, device=dev)
        for p in plans:
            p.vis_t_minus = vtm.clone()
    return net, plans, e


def _compare(net, plans, e, ev, Re=1500.0):
    from nsfnet_amd import engine as eng
    c = 2.0 / plans[0].n
    coef = (c, c, c, 0.1 * c if ev else 0.0)
    kw = dict(e=e, vis_t0=0.02 if ev else 0.0, alpha_evm=0.05 if ev else 0.0, scale=1.3)
    a, b = plans
    assert a.lib.pinn_plan_kernel(a.handle, 0) == b"fwd_split_kernel"
    a.forward(Re, save=True, **kw)
    a.backward(Re, coef, e=e, scale=kw["scale"], want_ebar=ev)
    b.forward_backward(Re, coef, want_ebar=ev, **kw)
    ga = torch.empty(net.num_params, dtype=torch.float32, device=net.device)
    gb = torch.empty_like(ga)
    eng.grad_reduce(net, [a], ga)
    eng.grad_reduce(net, [b], gb)
    torch.cuda.synchronize()
    assert torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    assert torch.equal(a.sums, b.sums)
    assert torch.equal(a.fields, b.fields)
    assert torch.equal(a.vis_t, b.vis_t)
    assert torch.equal(ga, gb)
    if ev:
        assert torch.equal(a.vis_t_minus, b.vis_t_minus)
        assert torch.equal(a.ebar, b.ebar)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_fused_equals_split_odd_tiles(monkeypatch, prec):
    _clear_sched(monkeypatch)
    n = 32 * 601 - 5                      # 601 tiles (a dummy partner), partial last tile, pairs loop over the grid
    net, plans, e = _plan_pair(6, 256, n, prec, ev=False)
    _compare(net, plans, e, ev=False)


@pytest.mark.parametrize("n", [70, 32 * 5])
def test_fused_equals_split_below_two_tiles_per_workgroup(monkeypatch, n):
    _clear_sched(monkeypatch)
    net, plans, e = _plan_pair(6, 256, n, "bf16x3", ev=False)
    _compare(net, plans, e, ev=False)


@pytest.mark.parametrize("L", [2, 3])
def test_fused_equals_split_shallow(monkeypatch, L):
    _clear_sched(monkeypatch)
    net, plans, e = _plan_pair(L, 256, 32 * 77 + 9, "bf16x3", ev=False)
    _compare(net, plans, e, ev=False)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_fused_equals_split_ev_inputs(monkeypatch, prec):
    _clear_sched(monkeypatch)
    net, plans, e = _plan_pair(6, 256, 32 * 311 + 17, prec, ev=True)
    _compare(net, plans, e, ev=True)


def test_fused_fallback_plans_are_the_two_calls(monkeypatch):
    """PINN_FUSE=0: pinn_residual_forward_backward is exactly forward + backward."""
    _clear_sched(monkeypatch)
    monkeypatch.setenv("PINN_FUSE", "0")
    net, plans, e = _plan_pair(4, 256, 32 * 41 + 3, "bf16x3", ev=True)
    _compare(net, plans, e, ev=True)


def _engine(flavour, L, H, x, y, chunk=None, prec="bf16x3"):
    from nsfnet_amd import engine as eng
    dev = torch.device("cuda:0")
    kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05) if flavour == "ev" else {}
    E = eng.PinnEngine(dev, L, H, 2000.0, alpha_b=10.0, alpha_e=1.0, precision=prec, **kw)
    E.net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=21)))
    if flavour == "ev":
        E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=22)))
        E.e_trainable = True
    xb, yb, ub, vb = (a.reshape(-1)[::4].astype(np.float32) for a in ar.cavity_boundary())
    E.set_collocation(x, y, chunk_points=chunk)
    E.set_boundary(xb, yb, ub, vb)
    return E


def _engine_ab(monkeypatch, flavour, L, H, n, chunk=None, steps=2):
    rng = np.random.RandomState(5)
    x = rng.rand(n).astype(np.float32); y = rng.rand(n).astype(np.float32)
    out = []
    for fuse in ("0", "1"):
        monkeypatch.setenv("PINN_FUSE", fuse)
        E = _engine(flavour, L, H, x, y, chunk)
        for _ in range(steps):
            E.step(1e-3)
        E.loss_and_grad()
        torch.cuda.synchronize()
        r = [E.sums.clone(), E.grads.clone(), E.net.params.clone(), E.plan_f.field("eq1").clone(), E.plan_f.vis_t.clone()]
        if flavour == "ev":
            r += [E.grads_e.clone(), E.plan_f.vis_t_minus.clone(), E.plan_f.ebar.clone()]
        out.append(r)
        del E
    for u, v in zip(*out):
        assert torch.equal(u, v)


def test_engine_ev_step_fused_equals_split(monkeypatch):
    _clear_sched(monkeypatch)
    _engine_ab(monkeypatch, "ev", 6, 256, 32 * 203 + 11)


def test_engine_chunked_step_fused_equals_split(monkeypatch):
    _clear_sched(monkeypatch)
    _engine_ab(monkeypatch, "nsfnet", 6, 256, 3 * 4096 + 1000, chunk=4096)


def test_engine_graph_replay_equals_eager(monkeypatch):
    _clear_sched(monkeypatch)
    rng = np.random.RandomState(6)
    x = rng.rand(9000).astype(np.float32); y = rng.rand(9000).astype(np.float32)
    out = []
    for graph in ("0", "1"):
        monkeypatch.setenv("NSFNET_GRAPH", graph)
        E = _engine("nsfnet", 6, 256, x, y)
        for _ in range(4):
            E.step(1e-3)
        torch.cuda.synchronize()
        out.append((E.net.params.clone(), E.sums.clone()))
        del E
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])


def test_engine_full_size_step_fused_equals_split(monkeypatch):
    """The headline shape: 6x256, 360 000 points, bf16x3."""
    _clear_sched(monkeypatch)
    _engine_ab(monkeypatch, "nsfnet", 6, 256, 360000, steps=1)
