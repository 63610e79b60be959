"""Residual-based resampling of the collocation points on the MI355X: the selection kernels against the numpy replay
(tests/resample_replay.py), determinism, and the in-place rewrite of the live buffers - a resampled engine must
compute exactly what a fresh engine built on the selected points computes, eagerly and from a captured graph."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_replay as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _net(n_out, L, H, precision, seed):
    from nsfnet_amd import engine as eng
    from oracle import autograd_ref as ar
    net = eng.DeviceNet(n_out, L, H, DEV, precision)
    net.set_flat(ar.flat_params(ar.seeded_net(n_out, L, H, seed=seed)))
    return net


def _points(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)


@pytest.mark.parametrize("L,H,precision", [(4, 50, "fp32"), (6, 256, "bf16x3")])
def test_selection_matches_numpy_replay(L, H, precision):
    from nsfnet_amd import engine as eng
    N, M = 1_000_003, 360_000
    net = _net(3, L, H, precision, seed=21)
    x, y = _points(N, 1)
    pool = eng.ResidualPlan(net, x, y, with_backward=False)
    pool.forward(2000.0, save=False)
    scratch = eng.resample_scratch(N, DEV)
    eq = pool.fields[6:10, :N].cpu().numpy()
    eq[3] = eq[0] * 0.5                          # (the plain forward leaves eq4 = 0: give w4 something to weigh)
    pool.fields[9, :N] = torch.from_numpy(eq[3]).to(DEV)
    for w4 in (0.0, 0.1):
        for k in (0.0, 1.0, 2.0):
            for c in (0.0, 1.0):
                u = 0.3141 + 0.1 * k + 0.05 * c
                idx, S = eng.resample_select(pool, w4, k, c, u, M, scratch)
                idx = idx.cpu().numpy()
                o_ref, v, S_ref = rr.offsets(eq, w4, k, c, u, M)
                assert abs(S - S_ref) <= 1e-12 * abs(S_ref), (w4, k, c, S, S_ref)
                assert idx.size == M and np.all(np.diff(idx) >= 0) and 0 <= idx[0] and idx[-1] < N
                o = rr.offsets_of(idx, N)
                clear = np.abs(v - np.round(v)) > 1e-9
                bad = np.flatnonzero(clear & (o != o_ref))
                assert bad.size == 0, (w4, k, c, bad[:10], o[bad[:10]], o_ref[bad[:10]])
                assert np.count_nonzero(~clear) < 10


def test_concentrated_density_and_non_finite_residuals():
    """One point holding nearly all the mass (c = 0, k = 2): its copies fill most of the output, written by its whole
    block.  A NaN residual shows in S for every k, k = 0 included."""
    from nsfnet_amd import engine as eng
    N, M = 200_003, 150_000
    net = _net(3, 4, 50, "fp32", seed=23)
    x, y = _points(N, 9)
    pool = eng.ResidualPlan(net, x, y, with_backward=False)
    pool.forward(1000.0, save=False)
    pool.fields[6:10, :N] *= 1e-3
    pool.fields[6, 77_777] = 1e4
    pool.fields[7, 150_000] = 3e3
    scratch = eng.resample_scratch(N, DEV)
    eq = pool.fields[6:10, :N].cpu().numpy()
    for k, c in ((2.0, 0.0), (1.0, 0.0), (2.0, 1e-3)):
        idx, S = eng.resample_select(pool, 0.0, k, c, 0.5, M, scratch)
        o_ref, v, _ = rr.offsets(eq, 0.0, k, c, 0.5, M)
        o = rr.offsets_of(idx.cpu().numpy(), N)
        clear = np.abs(v - np.round(v)) > 1e-9
        assert np.array_equal(o[clear], o_ref[clear]), (k, c)
        if (k, c) == (2.0, 0.0):
            assert int((idx == 77_777).sum()) > 0.9 * M
    pool.fields[8, 12_345] = float("nan")
    for k in (0.0, 1.0, 2.0, 1.5):
        _, S = eng.resample_select(pool, 0.0, k, 1.0, 0.5, M, scratch)
        assert np.isnan(S), k


def test_selection_is_deterministic():
    from nsfnet_amd import engine as eng
    net = _net(3, 4, 50, "fp32", seed=22)
    x, y = _points(300_001, 2)
    pool = eng.ResidualPlan(net, x, y, with_backward=False)
    pool.forward(1000.0, save=False)
    scratch = eng.resample_scratch(pool.n, DEV)
    a, _ = eng.resample_select(pool, 0.0, 1.0, 1.0, 0.25, 100_000, scratch)
    b, _ = eng.resample_select(pool, 0.0, 1.0, 1.0, 0.25, 100_000, scratch)
    assert torch.equal(a, b)
    picks = []
    for seed in (5, 5, 6):
        E = _engine("nsfnet", 4, 50, "fp32", 20_000, 300_001)
        picks.append(E.resample(k=1.0, c=1.0, seed=seed).cpu())
    assert torch.equal(picks[0], picks[1]) and not torch.equal(picks[0], picks[2])


def _engine(flavour, L, H, precision, M, NP, weights=True, seed=31):
    from nsfnet_amd import engine as eng
    from oracle import autograd_ref as ar
    ev = flavour == "ev"
    E = eng.PinnEngine(DEV, L, H, 2000.0, alpha_b=10.0, alpha_e=1.0, flavour=flavour, n_hidden_e=3, hidden_e=20,
                       alpha_evm=0.03, precision=precision)
    E.net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=seed)))
    if ev:
        E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 3, 20, seed=seed + 1)))
        E.e_trainable = True
    x, y = _points(M, 3)
    xp, yp = _points(NP, 4)
    rng = np.random.default_rng(5)
    w = (0.2 + rng.random(M)).astype(np.float32) if weights else None
    wp = (0.2 + rng.random(NP)).astype(np.float32) if weights else None
    E.set_collocation(x, y, w)
    xb, yb, ub, vb = (a.reshape(-1)[::8].astype(np.float32) for a in ar.cavity_boundary())
    E.set_boundary(xb, yb, ub, vb)
    E.set_resample_pool(xp, yp, wp)
    E._case = dict(xp=xp, yp=yp, wp=wp, b=(xb, yb, ub, vb))
    return E


def _fresh_like(E, idx):
    """A second engine with E's parameters and Adam state, built by set_collocation on the selected points."""
    from nsfnet_amd import engine as eng
    ev = E.net_e is not None
    F = eng.PinnEngine(DEV, E.net.n_hidden, E.net.hidden, E.Re, alpha_b=E.alpha_b, alpha_e=E.alpha_e, flavour=E.flavour,
                       n_hidden_e=3, hidden_e=20, alpha_evm=E.alpha_evm, precision=E.net.precision)
    for a, b in ((F.net, E.net),) + (((F.net_e, E.net_e),) if ev else ()):
        a.set_flat(b.params.clone())
        a.m.copy_(b.m); a.v.copy_(b.v); a.adam_t_dev.copy_(b.adam_t_dev); a.adam_t = b.adam_t
    F.e_trainable = E.e_trainable
    c, i = E._case, idx.cpu().numpy()
    _, _, w_new = E.collocation_points()
    F.set_collocation(c["xp"][i], c["yp"][i], None if w_new is None else w_new.cpu().numpy())
    F.set_boundary(*c["b"])
    return F


def _assert_same_evaluation(E, F):
    E.loss_and_grad()
    F.loss_and_grad()
    torch.cuda.synchronize()
    assert torch.equal(E.flat, F.flat)                   # gradients | entropy-net gradients | loss sums
    for name in ("u", "v", "p", "u_x", "u_y", "v_x", "v_y", "eq1", "eq2", "eq3", "eq4"):
        assert torch.equal(E.plan_f.field(name), F.plan_f.field(name)), name
    assert torch.equal(E.plan_f.vis_t, F.plan_f.vis_t)
    if E.net_e is not None:
        assert torch.equal(E.plan_f.ebar, F.plan_f.ebar)
        assert torch.equal(E.plan_f.vis_t_minus, F.plan_f.vis_t_minus)


@pytest.mark.parametrize("flavour,L,H,precision,chunk", [
    ("nsfnet", 4, 50, "fp32", None), ("nsfnet", 4, 50, "fp32", 1024), ("ev", 4, 50, "fp32", None),
    ("ev", 4, 50, "fp32", 1024), ("ev", 6, 256, "bf16x3", None), ("nsfnet", 6, 256, "bf16x3", 2048)])
def test_in_place_resample_equals_fresh_engine(monkeypatch, flavour, L, H, precision, chunk):
    from nsfnet_amd import engine as eng
    if chunk:
        monkeypatch.setenv("NSFNET_CHUNK_POINTS", str(chunk))
    else:
        monkeypatch.delenv("NSFNET_CHUNK_POINTS", raising=False)
    M, NP = 5000, 20011
    E = _engine(flavour, L, H, precision, M, NP)
    assert isinstance(E.plan_f, eng.ChunkedResidual) == bool(chunk)
    if L == 6:
        assert E.plan_f.kernel_names()[0] == "fwd_split_kernel" if not chunk else True
    E.step(1e-3)                                         # parameters and Adam moments away from their start
    idx = E.resample(k=1.0, c=1.0, seed=3)
    assert idx.numel() == M and bool((idx[1:] >= idx[:-1]).all())
    _, _, w = E.collocation_points()
    wp = E._case["wp"][idx.cpu().numpy()].astype(np.float64)
    np.testing.assert_allclose(w.cpu().numpy(), wp / wp.mean(), rtol=2e-7)
    F = _fresh_like(E, idx)
    if flavour == "ev":                                  # vis_t_minus at the new points: what init_vis_t gives
        assert torch.equal(E.plan_f.vis_t_minus, F.plan_f.vis_t_minus)
        assert torch.equal(E.plan_e.x, F.plan_e.x) and torch.equal(E.plan_e.y, F.plan_e.y)
    _assert_same_evaluation(E, F)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_captured_step_replays_on_the_resampled_points(monkeypatch, flavour):
    monkeypatch.setenv("NSFNET_GRAPH", "1")
    monkeypatch.delenv("NSFNET_CHUNK_POINTS", raising=False)
    E = _engine(flavour, 4, 50, "fp32", 4000, 15013)
    E.e_trainable = False
    E.step(1e-3)                                         # eager run + capture
    assert len(E._graphs) == 1
    graph = next(iter(E._graphs.values()))
    idx = E.resample(k=2.0, c=0.5, seed=9)
    F = _fresh_like(E, idx)
    E.step(1e-3)                                         # replay
    assert len(E._graphs) == 1 and next(iter(E._graphs.values())) is graph
    F.loss_and_grad()
    F.adam_step(1e-3)
    torch.cuda.synchronize()
    assert torch.equal(E.net.params, F.net.params) and torch.equal(E.net.m, F.net.m) and torch.equal(E.net.v, F.net.v)
    assert torch.equal(E.sums, F.sums)


def test_resample_touches_only_the_collocation_set():
    E = _engine("ev", 4, 50, "fp32", 3000, 9001)
    from oracle import autograd_ref as ar
    xs, ys = _points(40, 8)
    E.alpha_s = 0.5
    E.set_supervised(xs, ys, xs * 0.1, ys * 0.1, xs * 0.0)
    E.step(1e-3)
    torch.cuda.synchronize()
    keep = [E.net.params, E.net.m, E.net.v, E.net.adam_t_dev, E.net_e.params, E.net_e.m, E.net_e.v, E.plan_b.x, E.plan_b.y,
            E.plan_s.x, E.plan_s.y] + [t for t in E.plan_b.targets + E.plan_s.targets if t is not None]
    before = [t.clone() for t in keep]
    graphs, n_global, plan_b, plan_s = dict(E._graphs), E.n_f_global, E.plan_b, E.plan_s
    E.resample(seed=1)
    torch.cuda.synchronize()
    for a, b in zip(before, keep):
        assert torch.equal(a, b)
    assert E._graphs == graphs and E.n_f_global == n_global and E.plan_b is plan_b and E.plan_s is plan_s
    # a NaN coordinate in the pool: the call raises and the live set stays as it was
    xp, yp = E._case["xp"].copy(), E._case["yp"]
    xp[4321] = np.nan
    E.set_resample_pool(xp, yp, E._case["wp"])
    live = [t.clone() for t in E.collocation_points()] + [E.plan_f.vis_t_minus.clone(), E.plan_e.x.clone()]
    with pytest.raises(FloatingPointError):
        E.resample(seed=2)
    torch.cuda.synchronize()
    after = list(E.collocation_points()) + [E.plan_f.vis_t_minus, E.plan_e.x]
    for a, b in zip(live, after):
        assert torch.equal(a, b)
    del ar


def test_solver_schedule_equals_manual_loop(monkeypatch, tmp_path):
    """train(n) with set_resampling(every=R), graph replay on, against a hand-written eager loop of resample + step."""
    from nsfnet_amd import pinn_solver as ps
    from oracle import autograd_ref as ar
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("NSFNET_CHUNK_POINTS", raising=False)
    x, y = ar.uniform_grid(40, 40)
    xp, yp = _points(30011, 6)

    def build():
        torch.manual_seed(3)
        P = ps.PysicsInformedNeuralNetwork(Re=400.0, layers=3, hidden_size=40, N_f=1600, bc_weight=10.0)
        P.set_boundary_data(X=ar.cavity_boundary())
        P.set_eq_training_data(X=(x, y))
        P.set_resample_pool(X=(xp, yp))
        P.log_every = P.save_every = 0
        return P

    monkeypatch.setenv("NSFNET_GRAPH", "1")
    A = build()
    A.set_resampling(every=3, k=1.0, c=1.0, seed=7)
    A.train(num_epoch=10, lr=1e-3)
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    B = build()
    for i in range(10):
        if i > 0 and i % 3 == 0:
            B.engine.resample(k=1.0, c=1.0, seed=7)
        B.engine.step(1e-3)
    torch.cuda.synchronize()
    assert A.engine._resample_calls == B.engine._resample_calls == 3
    assert torch.equal(A.engine.net.params, B.engine.net.params)
    assert torch.equal(A.x_f.reshape(-1), B.engine.plan_f.x)
