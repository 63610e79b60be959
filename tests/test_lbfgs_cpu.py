"""CPU tests of the L-BFGS optimizer: the compact-form model of the direction kernels against the two-loop
recursion, the host driver (nsfnet_amd.lbfgs) against torch.optim.LBFGS, two gloo ranks with the fakes,
and the ev drop-in's YAML keys.  The kernels themselves are checked against the model in test_lbfgs_gpu.py."""
import importlib.util
import io
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lbfgs_model import LbfgsModel, ModelHistory, NumpySpace, two_loop  # noqa: E402
from nsfnet_amd import lbfgs as L  # noqa: E402


# ---------------------------------------------------------------- 1. compact form vs two-loop
def _pairs(rng, n, count, reject_every=0):
    """(g, t, accept?) pushes of a well-conditioned quadratic-like sequence; every reject_every-th pair has y's < 0."""
    A = 1.0 + rng.rand(n)
    g = rng.randn(n)
    for k in range(count):
        s = rng.randn(n) * 0.1
        bad = reject_every and k % reject_every == reject_every - 1
        y = -A * s if bad else A * s + 0.01 * rng.randn(n) * np.abs(s)
        yield g, s, y, not bad


@pytest.mark.parametrize("m,pushes", [(1, 4), (5, 17), (100, 330)])
def test_compact_direction_matches_two_loop(m, pushes):
    rng = np.random.RandomState(m)
    n = 600
    mod = LbfgsModel(n, m)
    g0 = rng.randn(n)
    mod.direction(g0, 0.0)
    ref_pairs, gamma = [], 1.0
    for k, (_, s, y, ok) in enumerate(_pairs(rng, n, pushes, reject_every=3)):
        # choose g so that the model forms exactly (s, y): s = t d_prev, y = g - g_prev
        t = 0.5
        mod.d = s / t
        g = mod.g_prev + y
        s, y = t * mod.d, g - mod.g_prev                        # the pair exactly as the model forms it
        before = [(a.copy(), b.copy()) for a, b in mod.pairs()]
        r = mod.direction(g, t)
        if ok:
            ref_pairs.append((s, y))
            ref_pairs = ref_pairs[-m:]
            gamma = (y @ s) / (y @ y)
            assert r[4] == 1
        else:
            assert r[4] == 0
            after = mod.pairs()
            assert len(after) == len(before)
            for (a0, b0), (a1, b1) in zip(before, after):      # a rejected pair leaves the history alone
                np.testing.assert_array_equal(a0, a1)
                np.testing.assert_array_equal(b0, b1)
        assert len(mod.order) == len(ref_pairs) and mod.staging not in mod.order
        for (a, b), (s_, y_) in zip(mod.pairs(), ref_pairs):
            np.testing.assert_allclose(a, s_, rtol=1e-15, atol=0)
            np.testing.assert_allclose(b, y_, rtol=1e-15, atol=0)
        d_ref = two_loop(g, ref_pairs, gamma)
        assert np.linalg.norm(mod.d - d_ref) <= 1e-12 * np.linalg.norm(d_ref)
        assert abs(r[6] - gamma) <= 1e-15 * gamma
    assert pushes <= m or pushes - pushes // 3 >= 2 * m         # the ring wrapped at least twice


# ---------------------------------------------------------------- 2. host driver vs torch.optim.LBFGS (fp64)
def _rosenbrock():
    x = torch.linspace(-1.2, 1.0, 50, dtype=torch.float64).requires_grad_(True)
    return [x], lambda: torch.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)


def _pinn():
    from oracle import autograd_ref as ar
    rng = np.random.RandomState(0)
    x, y = rng.rand(64, 1), rng.rand(64, 1)
    xb, yb, ub, vb = (a[::40] for a in ar.cavity_boundary())
    net = ar.seeded_net(3, 2, 12, seed=7, dtype=torch.float64)
    o = ar.NSFnetOracle(net, 100.0, alpha_b=1.0, alpha_e=1.0)
    o.set_data(x, y, xb, yb, ub, vb)
    return list(net.parameters()), o.loss


def _np_fun(make):
    """fp64 (loss, gradient) of a fresh copy of the objective at a flat x."""
    params, loss = make()

    def fun(x):
        with torch.no_grad():
            torch.nn.utils.vector_to_parameters(torch.tensor(x, dtype=torch.float64), params)
        out = loss()
        g = torch.autograd.grad(out, params)
        return float(out.detach()), torch.cat([t.reshape(-1) for t in g]).numpy().copy()
    return fun, torch.nn.utils.parameters_to_vector(params).detach().numpy().copy()


def _torch_exit_reason(ts, fun, xt, iters, evals, max_iter, max_eval, tol_grad, tol_change):
    """Why torch.optim.LBFGS.step returned, from its own state and the objective at its final x (the accepted
    point's gradient is the gradient at x_init + t d, which is where torch leaves the parameters)."""
    if iters == 0:
        return "tolerance_grad"                      # max|g| at entry
    d, t = ts["d"], float(ts["t"])
    if float(ts["prev_flat_grad"] @ d) > -tol_change:
        return "gtd"                                 # (the loop went on only if this was <= -tolerance_change)
    if iters == max_iter:
        return "max_iter"
    if evals >= max_eval:
        return "max_eval"
    f, g = fun(xt)
    if np.abs(g).max() <= tol_grad:
        return "tolerance_grad"
    if float((d * t).abs().max()) <= tol_change:
        return "tolerance_change"
    if abs(f - float(ts["prev_loss"])) < tol_change:
        return "loss_change"
    return "none"


@pytest.mark.parametrize("objective", ["rosenbrock", "pinn"])
@pytest.mark.parametrize("ls", [None, "strong_wolfe"])
@pytest.mark.parametrize("tol_change", [1e-9, 1e-5])
def test_host_driver_matches_torch_lbfgs(objective, ls, tol_change):
    make = _rosenbrock if objective == "rosenbrock" else _pinn
    lr = 1.0 if ls else (1e-3 if objective == "rosenbrock" else 0.05)
    schedule = [7, 12, 3, 11, 9, 10, 8]               # max_iter per step call (max_eval exits end some early)
    params, loss = make()
    opt = torch.optim.LBFGS(params, lr=lr, max_iter=schedule[0], history_size=5, line_search_fn=ls,
                            tolerance_change=tol_change)
    t_losses = []

    def closure():
        opt.zero_grad()
        out = loss()
        out.backward()
        t_losses.append(float(out.detach()))
        return out

    fun, x0 = _np_fun(make)
    check_fun, _ = _np_fun(make)
    space = NumpySpace(fun, x0, 5)
    reasons = set()
    st = L.LbfgsState()
    iters = 0
    for k, mi in enumerate(schedule):
        opt.param_groups[0]["max_iter"] = mi
        opt.param_groups[0]["max_eval"] = mi * 5 // 4
        s0 = dict(opt.state[params[0]]) if params[0] in opt.state else dict(n_iter=0, func_evals=0)
        n_t = len(t_losses)
        opt.step(closure)
        n_d = len(space.losses)
        _, info = L.step(space, st, lr=lr, max_iter=mi, tolerance_grad=1e-7, tolerance_change=tol_change,
                         line_search_fn=ls)
        ts = opt.state[params[0]]
        assert len(space.losses) - n_d == len(t_losses) - n_t == info["evals"] == ts["func_evals"] - s0["func_evals"], k
        assert info["iters"] == ts["n_iter"] - s0["n_iter"], k
        xd, xt = space.x, torch.nn.utils.parameters_to_vector(params).detach().numpy()
        t_reason = _torch_exit_reason(ts, check_fun, xt, ts["n_iter"] - s0["n_iter"], ts["func_evals"] - s0["func_evals"],
                                      mi, mi * 5 // 4, 1e-7, tol_change)
        assert info["reason"] == t_reason, (k, info, t_reason)
        reasons.add(t_reason)
        assert np.linalg.norm(xd - xt) <= 1e-9 * np.linalg.norm(xt), (k, np.linalg.norm(xd - xt))
        np.testing.assert_allclose(space.losses[n_d:], t_losses[n_t:], rtol=1e-8)     # (loss: a sum of squares)
        iters += info["iters"]
    assert iters >= 40 or reasons - {"max_iter", "max_eval"}, (iters, reasons)   # 40 iterations or an early exit


def test_driver_rejects_unknown_line_search():
    with pytest.raises(ValueError, match="line_search_fn"):
        L.step(NumpySpace(_np_fun(_rosenbrock)[0], np.zeros(50), 2), L.LbfgsState(), line_search_fn="backtracking")


# ---------------------------------------------------------------- 3. two gloo ranks with the fakes
def _gloo_case():
    rng = np.random.RandomState(42)
    N, Nb = 70, 33
    x, y = rng.rand(N, 1), rng.rand(N, 1)
    from oracle import autograd_ref as ar
    xb, yb, ub, vb = (a[::63][:Nb] for a in ar.cavity_boundary())
    w = (0.5 + rng.rand(N)).astype(np.float32)
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb, w=w)


def _gloo_solver(case, monkeypatch=None):
    import fakes
    from nsfnet_amd import engine as eng
    fakes.install(monkeypatch)
    if monkeypatch is not None:
        monkeypatch.setattr(eng, "LbfgsHistory", ModelHistory)
    else:
        eng.LbfgsHistory = ModelHistory
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(3)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]), weights=case["w"])
    P.log_interval = 1000
    P.save = lambda *a, **k: None
    return P


def _lbfgs_train(P):
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=1, history_size=5, line_search_fn="strong_wolfe")
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=5, lr=1.0, optimizer=opt)


def _gloo_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank,
                            world_size=world)
    try:
        P = _gloo_solver(_gloo_case())
        assert P.is_distributed
        _lbfgs_train(P)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=P.engine.net.params.numpy().copy(),
                 iters=P.engine._lbfgs_state.n_iter)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_lbfgs_matches_single_process(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_gloo_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    np.testing.assert_array_equal(r0["params"], r1["params"])
    assert int(r0["iters"]) == 5
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    P = _gloo_solver(_gloo_case(), monkeypatch)
    p0 = P.engine.net.params.clone()
    e0 = P.engine.net_e.params.clone()
    _lbfgs_train(P)
    assert not torch.equal(P.engine.net.params, p0)
    assert torch.equal(P.engine.net_e.params, e0)            # the entropy net stays frozen
    assert P.engine.net.adam_t == 0 and float(P.engine.net.m.abs().max()) == 0.0
    np.testing.assert_allclose(r0["params"], P.engine.net.params.numpy(), rtol=0, atol=1e-6)


def test_new_lbfgs_object_after_adam_starts_fresh(monkeypatch):
    """LBFGS(a) -> Adam -> LBFGS(b): b starts like a fresh torch.optim.LBFGS (first iteration: d = -g, the
    1/|g|_1 step) and gives what an engine that never saw `a` gives from the same point.  Going back to `a` after
    `b` is again a change of owner."""
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    from nsfnet_amd.pinn_solver import AdamHandle

    def lbfgs(P):
        return torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=1, max_eval=10, history_size=5,
                                 line_search_fn="strong_wolfe")

    def run(P, opt, n):
        with contextlib.redirect_stdout(io.StringIO()):
            P.train(num_epoch=n, lr=1.0, optimizer=opt)

    P = _gloo_solver(_gloo_case(), monkeypatch)
    a = lbfgs(P)
    run(P, a, 3)
    P.set_optimizers(AdamHandle(1e-3))
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=2, lr=1e-3)
    mid = P.engine.net.params.clone()
    run(P, lbfgs(P), 3)
    assert P.engine._lbfgs_state.n_iter == 3                 # counted from the new object's first iteration
    fresh = _gloo_solver(_gloo_case(), monkeypatch)
    fresh.engine.net.set_flat(mid)
    run(fresh, lbfgs(fresh), 3)
    assert torch.equal(P.engine.net.params, fresh.engine.net.params)
    run(P, a, 1)                                             # the first object again: a new owner, fresh again
    assert P.engine._lbfgs_state.n_iter == 1


def test_solver_dispatches_lbfgs_and_keeps_its_history(monkeypatch):
    """train(optimizer=LBFGS) runs the L-BFGS loop (the Adam path would leave the moments non-zero), the history
    persists across train() calls and lbfgs_reset clears it."""
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    P = _gloo_solver(_gloo_case(), monkeypatch)
    _lbfgs_train(P)
    assert P.engine._lbfgs_state.n_iter == 5
    assert float(P.engine.net.m.abs().max()) == 0.0
    P.engine.lbfgs_reset()
    assert P.engine._lbfgs_state.n_iter == 0


def test_an_l2_evaluation_does_not_change_the_lbfgs_objective(monkeypatch):
    """The loss mode is an argument of one evaluation: an L2 fwd_computing_loss_2d before lbfgs_step leaves it on the
    MSE loss, with the iterate and loss of a run without that call."""
    import fakes
    from nsfnet_amd import engine as eng
    from nsfnet_amd import pinn_solver as ps
    fakes.install(monkeypatch)
    monkeypatch.setattr(eng, "LbfgsHistory", ModelHistory)
    case = _gloo_case()

    def run(l2_first):
        torch.manual_seed(3)
        P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=10, N_f=70, bc_weight=10, eq_weight=1)
        P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
        P.set_eq_training_data(X=(case["x"], case["y"]))
        if l2_first:
            P.fwd_computing_loss_2d(loss_mode="L2")
        entry = P.engine.lbfgs_step(max_iter=3, history_size=5, line_search_fn="strong_wolfe")
        return entry, float(P.engine.loss_terms()["loss"]), P.engine.net.params.clone()

    a, b = run(False), run(True)
    assert a[:2] == b[:2]
    assert torch.equal(a[2], b[2])


# ---------------------------------------------------------------- 4. ev drop-in YAML
def _config_module():
    path = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py")
    spec = importlib.util.spec_from_file_location("ev_dropin_config_lbfgs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


STAGES = """
training:
  training_stages:
    - {name: warm, alpha: 0.05, epochs: 100, lr: 1.0e-3}
    - {name: finish, alpha: 0.05, epochs: 20, lr: 1.0, optimizer: %s, history_size: 30, line_search: %s}
"""


def test_ev_config_parses_an_lbfgs_stage(tmp_path):
    cfg = _config_module()
    p = tmp_path / "c.yaml"
    p.write_text(STAGES % ("lbfgs", "strong_wolfe"))
    st = cfg.ConfigManager.from_file(str(p)).config.training.training_stages
    assert [s.optimizer for s in st] == ["adam", "lbfgs"]
    assert st[1].history_size == 30 and st[1].line_search == "strong_wolfe" and st[0].history_size == 100
    p.write_text(STAGES % ("lbfgs", "none"))
    assert cfg.ConfigManager.from_file(str(p)).config.training.training_stages[1].line_search == "none"


@pytest.mark.parametrize("opt,ls", [("sgd", "strong_wolfe"), ("lbfgs", "armijo")])
def test_ev_config_rejects_unknown_optimizer_values(tmp_path, opt, ls):
    cfg = _config_module()
    p = tmp_path / "c.yaml"
    p.write_text(STAGES % (opt, ls))
    with pytest.raises(ValueError, match="optimizer" if opt == "sgd" else "line_search"):
        cfg.ConfigManager.from_file(str(p))
