"""CPU tests of the device learning-rate schedules and gradient clipping of the Adam stages: the
fp64 model against torch.optim.lr_scheduler and clip_grad_norm_, the engine's host logic on the oracle-backed fakes
(the off path makes the parent's calls, the epoch counter survives reset_adam and L-BFGS, the graph key), two gloo
ranks, the solvers' scheduler= argument, the ev drop-in's YAML keys and the C ABI.  The kernels are checked against the
model in test_lr_schedule_gpu.py."""
import contextlib
import ctypes
import dataclasses
import importlib.util
import io
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import optim_model as om  # noqa: E402
from nsfnet_amd.schedule import LrSchedule, from_torch  # noqa: E402

LR0 = 1e-3


# ------------------------------------------------------------------ the model
def _torch_sequence(make, n):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=LR0)
    sched = make(opt)
    out = [opt.param_groups[0]["lr"]]
    for _ in range(n):
        opt.step()
        sched.step()
        out.append(opt.param_groups[0]["lr"])
    return sched, out


@pytest.mark.parametrize("name,make", [
    ("multistep", lambda o: torch.optim.lr_scheduler.MultiStepLR(o, [300, 1000, 1000, 2500], gamma=0.3)),
    ("step", lambda o: torch.optim.lr_scheduler.StepLR(o, 700, gamma=0.5)),
    ("exponential", lambda o: torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.999)),
    ("cosine", lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=2500, eta_min=1e-6)),
])
def test_model_matches_torch_schedulers_over_3000_epochs(name, make):
    """The closed forms against torch's own (recursive) sequence.  The bound 1e-12 lr0 is the drift of torch's
    recursion (measured: at most 1.8e-14 lr0 over these 3000 epochs, 0 for multistep and step) with room for longer
    runs; the cosine form runs past t_max."""
    sched, seq = _torch_sequence(make, 3000)
    spec, lr0, e = from_torch(sched)
    assert spec.kind == name and lr0 == LR0 and e == 3000
    worst = 0.0
    for k, want in enumerate(seq):
        got = om.lr_e(LR0, k, **dataclasses.asdict(spec))
        assert got == spec.value(LR0, k)           # the LrSchedule's host formula is the model's, bit for bit
        worst = max(worst, abs(got - want))
    print("%s: max |closed form - torch| = %.3e lr0" % (name, worst / LR0))
    assert worst <= 1e-12 * LR0


def test_from_torch_refuses_what_it_does_not_know():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=LR0)
    assert from_torch(torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)) is None

    class Mine(torch.optim.lr_scheduler.StepLR):       # a subclass may compute something else
        pass
    assert from_torch(Mine(opt, 3)) is None
    assert from_torch(object()) is None


def test_hand_examples_and_warmup_at_exact_values():
    assert om.lr_e(0.5, 7) == 0.5
    ms = dict(kind="multistep", milestones=(2, 4, 4), gamma=0.5)
    assert [om.lr_e(1.0, e, **ms) for e in range(6)] == [1.0, 1.0, 0.5, 0.5, 0.125, 0.125]
    st = dict(kind="step", step_size=3, gamma=0.25)
    assert [om.lr_e(2.0, e, **st) for e in (0, 2, 3, 5, 6)] == [2.0, 2.0, 0.5, 0.5, 0.125]
    assert om.lr_e(1.0, 3, kind="exponential", gamma=0.5) == 0.125
    cs = dict(kind="cosine", t_max=4, eta_min=0.25)
    assert om.lr_e(1.0, 0, **cs) == 1.0 and om.lr_e(1.0, 4, **cs) == 0.25
    assert om.lr_e(1.0, 2, **cs) == pytest.approx(0.625, abs=1e-16)
    assert om.lr_e(1.0, 8, **cs) == 1.0                       # past t_max the cosine comes back, as torch's closed form
    wu = dict(warmup_epochs=4, warmup_start=0.5)
    assert [om.lr_e(1.0, e, **wu) for e in (0, 1, 2, 4, 9)] == [0.5, 0.625, 0.75, 1.0, 1.0]
    assert om.lr_e(1.0, 1, kind="exponential", gamma=0.5, warmup_epochs=2) == 0.25     # the product of the two
    assert om.lr_e(1.0, 0, warmup_epochs=3) == 0.0


def test_lr_schedule_validates():
    for bad in (dict(kind="linear"), dict(kind="step", gamma=0.0), dict(kind="exponential", gamma=float("nan")),
                dict(kind="multistep", milestones=(5, 3)), dict(kind="multistep", milestones=(-1,)),
                dict(kind="multistep", milestones=tuple(range(17))), dict(kind="cosine", t_max=0),
                dict(kind="step", step_size=0), dict(warmup_start=1.5), dict(warmup_start=-0.1),
                dict(warmup_epochs=-1), dict(kind="cosine", t_max=2.5), dict(kind="cosine", eta_min=float("inf"))):
        with pytest.raises(ValueError):
            LrSchedule(**bad)
    s = LrSchedule("multistep", milestones=[1, 2, 2], gamma=0.5)
    assert s.milestones == (1, 2, 2) and hash(s.key()) == hash(LrSchedule("multistep", milestones=(1, 2, 2), gamma=0.5).key())
    assert len(LrSchedule("multistep", milestones=range(16)).milestones) == 16


def test_clipping_matches_clip_grad_norm():
    """Coefficient and scaled gradients against torch.nn.utils.clip_grad_norm_ on a (main, entropy net) parameter
    list, to fp32 rounding (torch forms the norm in fp32, the model in fp64: one rounding apart)."""
    rng = np.random.RandomState(0)
    g0, g1 = rng.randn(5000).astype(np.float32), (3.0 * rng.randn(317)).astype(np.float32)
    for max_norm in (1.0, 50.0, 1e4):
        ps = [torch.nn.Parameter(torch.zeros(g.size)) for g in (g0, g1)]
        for p, g in zip(ps, (g0, g1)):
            p.grad = torch.tensor(g)
        total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        norm, coef = om.clip(om.sqnorm(g0, g1), max_norm)
        np.testing.assert_allclose(norm, total, rtol=2.0 ** -23)
        if max_norm == 1e4:        # below max_norm nothing changes
            assert coef == 1.0
            np.testing.assert_array_equal(om.scaled(g0, coef), g0)
            np.testing.assert_array_equal(ps[1].grad.numpy(), g1)
            continue
        assert coef < 1.0
        np.testing.assert_allclose(float(coef), max_norm / (total + 1e-6), rtol=2.0 ** -23)
        for p, g in zip(ps, (g0, g1)):
            np.testing.assert_allclose(om.scaled(g, coef), p.grad.numpy(), rtol=2.0 ** -23, atol=0)
    assert np.isnan(om.clip(float("nan"), 1.0)[1]) and om.clip(float("inf"), 1.0)[1] == 0.0


# ------------------------------------------------------------------ the engine on the fakes
L, H, RE = 2, 10, 400.0
LR = 2.0 ** -10      # an fp32 value: the fake's plain path takes lr as fp64, the scheduled path rounds lr_e to fp32


def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", **kw):
    import optim_fakes
    optim_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=2, hidden_e=6, alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev, **kw)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"])
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    return e


COSINE = LrSchedule("cosine", t_max=10, eta_min=1e-5, warmup_epochs=3, warmup_start=0.1)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_off_makes_the_parents_calls(monkeypatch, flavour):
    """With both features off - never set, or set and switched off again - adam_step makes the plain
    DeviceNet.adam_step(grads, lr) calls in the plain order, with the same results, and the graph key is the plain
    one."""
    import optim_fakes
    case = _case()
    a = _engine(monkeypatch, case, flavour)
    b = _engine(monkeypatch, case, flavour)
    b.set_lr_schedule(COSINE); b.set_grad_clipping(0.5)
    assert b.optimizer_info() is not None
    b.set_lr_schedule(None)
    assert b.optimizer_info()["schedule"] is None and b.optimizer_info()["max_norm"] == 0.5
    b.set_grad_clipping(0.0)
    assert a.optimizer_info() is None and b.optimizer_info() is None and b._opt is None
    calls = []
    for e in (a, b):
        if flavour == "ev":
            e.e_trainable = True
        del optim_fakes.CALLS[:]
        for _ in range(2):
            e.step(LR)
        calls.append(list(optim_fakes.CALLS))
    want = [("adam_step", 3, LR)] + ([("adam_step", 1, LR)] if flavour == "ev" else [])
    assert calls[0] == calls[1] == want * 2
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    assert _keys(monkeypatch, a, [lambda e: None])[0] == _keys(monkeypatch, b, [lambda e: None])[0]


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_constant_schedule_without_clipping_is_the_plain_step(monkeypatch, flavour):
    import optim_fakes
    case = _case()
    a = _engine(monkeypatch, case, flavour)
    b = _engine(monkeypatch, case, flavour)
    b.set_lr_schedule(LrSchedule())
    for e in (a, b):
        if flavour == "ev":
            e.e_trainable = True
    del optim_fakes.CALLS[:]
    for _ in range(3):
        a.step(LR)
    for _ in range(3):
        b.step(LR)
    assert all(c[0] == "adam_step" for c in optim_fakes.CALLS[:len(optim_fakes.CALLS) // 2])
    # the scheduled order: the entropy net first without advancing, the main net last
    tail = optim_fakes.CALLS[len(optim_fakes.CALLS) // 2:]
    one = ([("adam_step_sched", 1, LR, False)] if flavour == "ev" else []) + [("adam_step_sched", 3, LR, True)]
    assert tail == one * 3
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    np.testing.assert_array_equal(a.net.m.numpy(), b.net.m.numpy())
    if flavour == "ev":
        np.testing.assert_array_equal(a.net_e.params.numpy(), b.net_e.params.numpy())
    info = b.optimizer_info()
    assert info["epoch"] == 2 and info["next_epoch"] == 3 and info["updates"] == 3 and info["clipped"] == 0
    assert info["lr"] == LR and info["clip_coef"] == 1.0 and info["grad_norm"] == 0.0


def test_schedule_and_clipping_follow_the_model(monkeypatch):
    """ev flavour, both nets trainable: each update uses lr_e of the epoch counter and the coefficient of the norm over
    BOTH gradients, the same for both nets; grads stays the raw gradient; the counter advances once per step."""
    import optim_fakes
    case = _case()
    e = _engine(monkeypatch, case, "ev")
    e.e_trainable = True
    e.set_lr_schedule(COSINE)
    e.set_grad_clipping(0.5)
    clipped = 0
    for k in range(5):
        e.loss_and_grad()
        g, ge = e.grads.numpy().copy(), e.grads_e.numpy().copy()
        before = [t.numpy().copy() for t in (e.net.params, e.net.m, e.net.v, e.net_e.params, e.net_e.m, e.net_e.v)]
        del optim_fakes.CALLS[:]
        e.adam_step(LR0)
        assert [c[0] for c in optim_fakes.CALLS] == ["grad_sqnorm", "adam_step_sched", "adam_step_sched"]
        assert optim_fakes.CALLS[0] == ("grad_sqnorm", e.P, e.P1)
        np.testing.assert_array_equal(e.grads.numpy(), g)
        lr = np.float32(COSINE.value(LR0, k))
        norm, coef = om.clip(om.sqnorm(g, ge), 0.5)
        clipped += coef < 1.0
        for net, grad, (p0, m0, v0) in ((e.net, g, before[:3]), (e.net_e, ge, before[3:])):
            p, m, v = om.update(p0, grad, m0, v0, k + 1, lr, coef)
            np.testing.assert_array_equal(net.params.numpy(), p.astype(np.float32))
            np.testing.assert_array_equal(net.v.numpy(), v.astype(np.float32))
        info = e.optimizer_info()
        assert (info["epoch"], info["next_epoch"], info["updates"], info["clipped"]) == (k, k + 1, k + 1, clipped)
        assert info["lr"] == float(lr) and info["grad_norm"] == norm and info["clip_coef"] == float(coef)
    assert clipped > 0
    # main net alone (the entropy net frozen): the norm is the main gradient's
    e.e_trainable = False
    e.loss_and_grad()
    del optim_fakes.CALLS[:]
    e.adam_step(LR0)
    assert optim_fakes.CALLS[0] == ("grad_sqnorm", e.P, 0) and len(optim_fakes.CALLS) == 2
    assert e.optimizer_info()["grad_norm"] == om.clip(om.sqnorm(e.grads.numpy()), 0.5)[0]


def test_epoch_survives_reset_adam_and_lbfgs_and_setters_restart_it(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, "ev")
    e.set_lr_schedule(COSINE)
    e.set_grad_clipping(0.5)
    for _ in range(3):
        e.step(LR0)
    assert e.optimizer_info()["next_epoch"] == 3
    e.net.reset_adam(); e.net_e.reset_adam()                 # the ev freeze schedule re-creates Adam
    assert int(e.net.adam_t_dev[0]) == 0 and e.optimizer_info()["next_epoch"] == 3
    e.step(LR0)
    info = e.optimizer_info()
    assert info["epoch"] == 3 and info["lr"] == float(np.float32(COSINE.value(LR0, 3))) and e.net.adam_t == 1
    params = e.net.params.numpy().copy()
    e.lbfgs_step(max_iter=3, line_search_fn="strong_wolfe")
    assert (e.net.params.numpy() != params).any()
    after = e.optimizer_info()
    assert after["next_epoch"] == 4 and after["updates"] == info["updates"] == 4
    e.set_grad_clipping(0.25)                                # clipping does not move the schedule
    assert e.optimizer_info()["next_epoch"] == 4
    e.reset_lr_schedule(7)
    assert e.optimizer_info()["next_epoch"] == 7
    e.reset_lr_schedule()
    assert e.optimizer_info()["next_epoch"] == 0
    e.reset_lr_schedule(5)
    e.set_lr_schedule(LrSchedule("exponential", gamma=0.9))  # a new schedule starts at 0
    assert e.optimizer_info()["next_epoch"] == 0
    with pytest.raises(ValueError):
        e.reset_lr_schedule(-1)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            e.set_grad_clipping(bad)
    with pytest.raises(TypeError):
        e.set_lr_schedule("cosine")


def _keys(monkeypatch, e, setups, lrs=None):
    """The graph keys step() looks up after each setup (the probe of test_rba_cpu.py)."""
    keys = []

    class Stop(Exception):
        pass

    class Probe(dict):
        def get(self, key, default=None):
            keys.append(key)
            raise Stop

        def clear(self):
            pass

    monkeypatch.setattr(e, "_graphs_enabled", lambda: True)
    old = e._graphs
    e._graphs = Probe()
    for i, setup in enumerate(setups):
        setup(e)
        with pytest.raises(Stop):
            e.step(LR0 if lrs is None else lrs[i])
    e._graphs = old
    return keys


def test_graph_key_is_constant_over_a_stage_and_carries_the_settings(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    e._graphs["stale"] = object()
    e.set_lr_schedule(COSINE)
    assert not e._graphs
    e._graphs["stale"] = object()
    e.set_grad_clipping(1.0)
    assert not e._graphs
    # a cosine stage: the key does not move while the device epoch does
    nop = lambda e: e.reset_lr_schedule(int(e.optimizer_info()["next_epoch"]) + 1)
    assert len(set(_keys(monkeypatch, e, [nop] * 5))) == 1
    setups = [lambda e: None,
              lambda e: e.set_grad_clipping(2.0),                                            # max_norm
              lambda e: e.set_lr_schedule(dataclasses.replace(COSINE, t_max=11)),           # the schedule
              lambda e: e.set_lr_schedule(dataclasses.replace(COSINE, t_max=11, warmup_epochs=4)),
              lambda e: e.set_grad_clipping(0.0),
              lambda e: e.set_lr_schedule(None)]                                            # off: the plain key
    keys = _keys(monkeypatch, e, setups)
    assert len(set(keys)) == len(keys)
    assert len(set(_keys(monkeypatch, e, [lambda e: e.set_lr_schedule(COSINE)] * 2, lrs=[1e-3, 2e-3]))) == 2   # lr0


# ------------------------------------------------------------------ two gloo ranks
def _run_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank,
                            world_size=world)
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        import optim_fakes
        optim_fakes.install(None)
        from nsfnet_amd import engine as eng
        case = _case()
        lo, hi = (0, 35) if rank == 0 else (35, 70)
        e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, process_group=dist.group.WORLD, world_size=world)
        rng = np.random.RandomState(5)
        e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
        e.set_collocation(case["x"][lo:hi], case["y"][lo:hi], n_global=70)
        blo, bhi = (0, 16) if rank == 0 else (16, 33)
        e.set_boundary(*(case[k][blo:bhi] for k in ("xb", "yb", "ub", "vb")), n_global=33)
        e.set_lr_schedule(COSINE)
        e.set_grad_clipping(0.5)
        for _ in range(4):
            e.step(LR0)
        info = e.optimizer_info()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=e.net.params.numpy(), norm=info["grad_norm"],
                 coef=info["clip_coef"], clipped=info["clipped"], epoch=info["next_epoch"])
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_keep_identical_parameters_with_clipping(tmp_path):
    world = 2
    mp.spawn(_run_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    np.testing.assert_array_equal(r0["params"], r1["params"])
    assert float(r0["norm"]) == float(r1["norm"]) and float(r0["coef"]) == float(r1["coef"]) < 1.0
    assert int(r0["clipped"]) == int(r1["clipped"]) > 0 and int(r0["epoch"]) == int(r1["epoch"]) == 4


# ------------------------------------------------------------------ the solvers
def _plain_solver(monkeypatch, case):
    import optim_fakes
    optim_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=10, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.save = lambda *a, **k: None
    P.log_every = 2
    return P


def _train(P, **kw):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        P.train(**kw)
    return out.getvalue()


def test_torch_multistep_and_the_equivalent_lr_schedule_give_one_trajectory(monkeypatch):
    import optim_fakes
    case = _case()
    A = _plain_solver(monkeypatch, case)
    opt = torch.optim.Adam(A.net.parameters(), lr=LR0)
    A.set_optimizers(opt)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [2, 4], gamma=0.5)
    log = _train(A, num_epoch=6, lr=LR0, scheduler=sched)
    assert "device lr=" in log and "grad_norm" not in log
    assert all(c[0] == "adam_step_sched" and c[2] == LR0 for c in optim_fakes.CALLS)     # lr0, not the host's rate
    assert sched.last_epoch == 6 and opt.param_groups[0]["lr"] == pytest.approx(LR0 / 4)   # the loop still steps it
    info = A.engine.optimizer_info()
    assert info["next_epoch"] == 6 and info["lr"] == float(np.float32(LR0 / 4))
    pa = A.net.dev_net.params.numpy().copy()
    B = _plain_solver(monkeypatch, case)
    spec = LrSchedule("multistep", milestones=(2, 4), gamma=0.5)
    _train(B, num_epoch=6, lr=LR0, scheduler=spec)
    np.testing.assert_array_equal(B.net.dev_net.params.numpy(), pa)
    # a torch scheduler that has already run starts the device schedule at its last_epoch
    _train(A, num_epoch=1, lr=LR0 / 4, scheduler=sched)
    assert A.engine.optimizer_info()["epoch"] == 6
    # every train() call with an LrSchedule starts at 0, also one set on the solver
    _train(B, num_epoch=2, lr=LR0, scheduler=spec)
    assert B.engine.optimizer_info()["epoch"] == 1
    B.set_lr_schedule(COSINE)
    B.set_grad_clipping(0.5)
    log = _train(B, num_epoch=3, lr=LR0)
    info = B.engine.optimizer_info()
    assert info["epoch"] == 2 and info["schedule"] is COSINE and "grad_norm=" in log and "clipped=" in log
    log = _train(B, num_epoch=2, lr=LR0)
    assert B.engine.optimizer_info()["epoch"] == 1


def test_an_unrecognised_scheduler_takes_the_old_path(monkeypatch):
    import optim_fakes
    case = _case()
    P = _plain_solver(monkeypatch, case)
    opt = torch.optim.Adam(P.net.parameters(), lr=LR0)
    P.set_optimizers(opt)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    log = _train(P, num_epoch=3, lr=LR0, scheduler=sched)
    assert optim_fakes.CALLS == [("adam_step", 3, LR0), ("adam_step", 3, LR0 / 2), ("adam_step", 3, LR0 / 4)]
    assert P.engine.optimizer_info() is None and "device lr" not in log
    # ... and an L-BFGS stage ignores schedule and clipping and leaves the position alone
    P.set_lr_schedule(COSINE)
    _train(P, num_epoch=2, lr=LR0)
    lb = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=2, line_search_fn="strong_wolfe")
    n = len(optim_fakes.CALLS)
    _train(P, num_epoch=2, lr=1.0, optimizer=lb, scheduler=COSINE)
    assert len(optim_fakes.CALLS) == n and P.engine.optimizer_info()["next_epoch"] == 2


def test_ev_solver_schedule_survives_the_freeze_schedule(monkeypatch):
    import optim_fakes
    optim_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "NSFNET_CHUNK_POINTS"):
        monkeypatch.delenv(k, raising=False)
    case = _case()
    torch.manual_seed(3)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_interval = 2
    P.save = lambda *a, **k: None
    P.set_grad_clipping(0.5)
    log = _train(P, num_epoch=4, lr=LR0, scheduler=COSINE)       # epoch 0 and 1 re-create Adam (freeze_evm_net)
    info = P.engine.optimizer_info()
    assert info["epoch"] == 3 and info["lr"] == float(np.float32(COSINE.value(LR0, 3))) and info["updates"] == 4
    assert "device lr=" in log and "grad_norm=" in log


# ------------------------------------------------------------------ YAML, drop-in, C ABI
def _config_module():
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_optim", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


STAGE = "training:\n  training_stages:\n    - {alpha: 0.05, epochs: 1000, lr: 1.0e-3, name: S1%s}\n"


def test_ev_config_parses_scales_and_prints_the_scheduler_keys(tmp_path, capsys):
    cfg = _config_module()
    mgr = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                   "production.yaml"))
    assert mgr.config.training.grad_clip.max_norm == 0.0
    assert all(st.scheduler == "constant" and st.warmup_epochs == 0 for st in mgr.config.training.training_stages)
    mgr.print_config()
    out = capsys.readouterr().out
    assert "scheduler" not in out and "grad clip" not in out          # printed only when on
    p = tmp_path / "c.yaml"
    p.write_text(STAGE % "")
    st = cfg.ConfigManager.from_file(str(p)).config.training.training_stages[0]
    assert st.scheduler == "constant" and LrSchedule(**st.schedule_args()) == LrSchedule(t_max=1000)
    p.write_text(STAGE % ", scheduler: cosine, eta_min: 1.0e-6, warmup_epochs: 100, warmup_start: 0.1")
    st = cfg.ConfigManager.from_file(str(p)).config.training.training_stages[0]
    assert LrSchedule(**st.schedule_args()) == LrSchedule("cosine", t_max=1000, eta_min=1e-6, warmup_epochs=100,
                                                          warmup_start=0.1)       # t_max defaults to the epochs
    assert LrSchedule(**st.schedule_args(0.01)) == LrSchedule("cosine", t_max=10, eta_min=1e-6, warmup_epochs=1,
                                                              warmup_start=0.1)   # every count scales like epochs
    p.write_text(STAGE % ", scheduler: multistep, milestones: [300, 600], gamma: 0.5, t_max: 400")
    st = cfg.ConfigManager.from_file(str(p)).config.training.training_stages[0]
    assert LrSchedule(**st.schedule_args(0.1)) == LrSchedule("multistep", milestones=(30, 60), gamma=0.5, t_max=40)
    p.write_text(STAGE % ", scheduler: step, step_size: 250, gamma: 0.3" + "  grad_clip: {max_norm: 2.5}\n")
    mgr = cfg.ConfigManager.from_file(str(p))
    st = mgr.config.training.training_stages[0]
    assert LrSchedule(**st.schedule_args(0.001)).step_size == 1 and st.schedule_args(0.5)["step_size"] == 125
    assert mgr.config.training.grad_clip.max_norm == 2.5
    mgr.print_config()
    out = capsys.readouterr().out
    assert "grad clip  : max_norm=2.5" in out and "S1: step step_size=250 gamma=0.3" in out
    p.write_text(STAGE % ", scheduler: exponential, gamma: 0.999")
    assert cfg.ConfigManager.from_file(str(p)).config.training.training_stages[0].schedule_args()["gamma"] == 0.999


@pytest.mark.parametrize("bad", [
    ", scheduler: linear", ", scheduler: step, gamma: 0.0", ", scheduler: exponential, gamma: -1",
    ", scheduler: multistep, milestones: [5, 3]", ", scheduler: multistep, milestones: [-1]",
    ", scheduler: multistep, milestones: [%s]" % ", ".join(str(i) for i in range(17)),
    ", scheduler: step, step_size: 0", ", scheduler: cosine, t_max: -1", ", scheduler: cosine, eta_min: .inf",
    ", warmup_epochs: -1", ", warmup_epochs: 10, warmup_start: 1.5", ", warmup_start: -0.5",
    ", optimizer: lbfgs, scheduler: cosine", ", optimizer: lbfgs, warmup_epochs: 5",
    "}\n  grad_clip: {max_norm: -1.0", "}\n  grad_clip: {max_norm: .nan"])
def test_ev_config_validation_errors(tmp_path, bad):
    cfg = _config_module()
    p = tmp_path / "c.yaml"
    p.write_text(STAGE % bad)
    with pytest.raises(ValueError):
        cfg.ConfigManager.from_file(str(p))
    p.write_text(STAGE % ", optimizer: lbfgs, scheduler: constant")      # ... but this is fine
    cfg.ConfigManager.from_file(str(p))


def test_dropin_train_script_passes_the_stage_schedule(tmp_path, monkeypatch):
    """train.py's stage loop on a stub solver: a stage with a scheduler or a warm-up reaches train() with the scaled
    LrSchedule, a constant one without scheduler=, an L-BFGS one with its optimizer."""
    d = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet")
    monkeypatch.syspath_prepend(d)
    for name in ("train", "config", "logger", "cavity_data", "pinn_solver"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    spec = importlib.util.spec_from_file_location("ev_dropin_train_optim", os.path.join(d, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    cfg = sys.modules["config"]
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  training_stages:\n"
                 "    - {alpha: 0.05, epochs: 1000, lr: 1.0e-3, name: A, scheduler: cosine, eta_min: 1.0e-6}\n"
                 "    - {alpha: 0.03, epochs: 2000, lr: 2.0e-4, name: B}\n"
                 "    - {alpha: 0.02, epochs: 400, lr: 1.0e-4, name: C, warmup_epochs: 100, warmup_start: 0.5}\n"
                 "    - {alpha: 0.01, epochs: 300, lr: 1.0, name: D, optimizer: lbfgs}\n"
                 "    - {alpha: 0.01, epochs: 600, lr: 1.0e-5, name: E, scheduler: multistep, milestones: [200, 400]}\n")
    stages = cfg.ConfigManager.from_file(str(p)).config.training.training_stages
    calls = []

    class Stub:
        net = torch.nn.Linear(2, 2)

        def set_alpha_evm(self, a):
            pass

        def set_optimizers(self, o):
            pass

        def train(self, **kw):
            calls.append(kw)

    class Log:
        def stage(self, *a):
            pass

    train.run_stages(Stub(), stages, 0.1, 0, Log())
    assert [c["num_epoch"] for c in calls] == [100, 200, 40, 30, 60] and [c["lr"] for c in calls] == [1e-3, 2e-4, 1e-4, 1.0, 1e-5]
    assert calls[0]["scheduler"] == LrSchedule("cosine", t_max=100, eta_min=1e-6)
    assert "scheduler" not in calls[1] and "optimizer" not in calls[1]
    assert calls[2]["scheduler"] == LrSchedule(t_max=40, warmup_epochs=10, warmup_start=0.5)
    assert isinstance(calls[3]["optimizer"], torch.optim.LBFGS) and "scheduler" not in calls[3]
    assert calls[4]["scheduler"] == LrSchedule("multistep", milestones=(20, 40), t_max=60)
    src = open(os.path.join(d, "train.py")).read()
    assert re.search(r"PINN\.set_grad_clipping\(max_norm=\w+\.max_norm\)", src)
    assert src.index("PINN.set_grad_clipping") < src.rindex("run_stages(PINN,")       # the call in main()


def test_header_declares_and_lib_binds_the_calls():
    hdr = open(os.path.join(ROOT, "include", "nsfnet_pinn.h")).read()
    from nsfnet_amd import _lib, build, engine as eng
    assert "optim.hip" in build.SOURCES
    for name, nargs in (("pinn_lr_schedule_value", 3), ("pinn_grad_sqnorm_scratch_bytes", 0), ("pinn_grad_sqnorm", 6),
                        ("pinn_adam_step_sched", 17)):
        assert re.search(r"\b(int|int64_t|double) %s\(" % name, hdr), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert "#define PINN_OPTIM_RECORD %d" % om.RECORD in hdr and eng.OPTIM_RECORD == om.RECORD
    assert "#define PINN_LR_MAX_MILESTONES 16" in hdr
    from nsfnet_amd import schedule
    assert schedule.KINDS == om.KINDS and ctypes.sizeof(_lib.LrScheduleStruct) == 8 + 16 * 8 + 3 * 8 + 3 * 8
    for i, k in enumerate(("CONSTANT", "MULTISTEP", "STEP", "EXPONENTIAL", "COSINE")):
        assert re.search(r"PINN_LR_%s = %d\b" % (k, i), hdr)
    if not os.path.exists(_lib.LIB_PATH):
        return
    lib = _lib.load()
    assert lib.pinn_abi_version() == 3
    assert lib.pinn_grad_sqnorm_scratch_bytes() >= 8 * (2 + 512)
    # the host formula against the model on a grid of epochs: both are fp64 closed forms on the same libm
    specs = [LrSchedule(), LrSchedule("multistep", milestones=(3, 10, 10, 50), gamma=0.3),
             LrSchedule("step", step_size=7, gamma=0.5, warmup_epochs=10, warmup_start=0.1),
             LrSchedule("exponential", gamma=0.999), LrSchedule("cosine", t_max=2500, eta_min=1e-6, warmup_epochs=100)]
    for spec in specs:
        st = spec.c_struct()
        for e in list(range(0, 120)) + [2499, 2500, 2501, 5000, 100000]:
            got = lib.pinn_lr_schedule_value(ctypes.byref(st), LR0, e)
            want = om.lr_e(LR0, e, **dataclasses.asdict(spec))
            assert abs(got - want) <= 1e-15 * abs(want), (spec, e, got, want)
    # argument checks happen on the host, before any launch
    good = specs[4].c_struct()
    assert np.isnan(lib.pinn_lr_schedule_value(None, LR0, 0)) and b"pinn_lr_schedule_value" in lib.pinn_last_error()
    assert np.isnan(lib.pinn_lr_schedule_value(ctypes.byref(good), LR0, -1))

    def broken(**kw):
        s = LrSchedule("multistep", milestones=(1, 2), gamma=0.5).c_struct()
        for k, v in kw.items():
            if k == "m1":
                s.milestones[1] = v
            else:
                setattr(s, k, v)
        return ctypes.byref(s)

    for kw, word in ((dict(kind=9), b"kind"), (dict(gamma=0.0), b"gamma"), (dict(n_milestones=17), b"milestones"),
                     (dict(m1=0), b"milestones"), (dict(kind=2, step_size=0), b"step_size"),
                     (dict(kind=4, t_max=0), b"t_max"), (dict(warmup_epochs=-1), b"warmup_epochs"),
                     (dict(warmup_epochs=2, warmup_start=2.0), b"warmup_start")):
        assert np.isnan(lib.pinn_lr_schedule_value(broken(**kw), LR0, 1)) and word in lib.pinn_last_error(), kw
        assert lib.pinn_adam_step_sched(16, 16, 16, 16, 10, broken(**kw), LR0, 0.9, 0.999, 1e-8, 16, 16, 1, None, 0.0, 16,
                                        None) < 0
    assert lib.pinn_grad_sqnorm(None, 10, None, 0, 16, None) < 0 and b"pinn_grad_sqnorm" in lib.pinn_last_error()
    assert lib.pinn_grad_sqnorm(16, 0, None, 0, 16, None) < 0 and b"n0" in lib.pinn_last_error()
    assert lib.pinn_grad_sqnorm(16, 10, None, 5, 16, None) < 0 and b"g1" in lib.pinn_last_error()
    assert lib.pinn_grad_sqnorm(16, 10, 32, 0, 16, None) < 0
    assert lib.pinn_grad_sqnorm(16, 10, None, 0, 12, None) < 0 and b"aligned" in lib.pinn_last_error()
    assert lib.pinn_grad_sqnorm(16, 10, None, 0, None, None) < 0
    ok = ctypes.byref(good)
    assert lib.pinn_adam_step_sched(None, 16, 16, 16, 10, ok, LR0, 0.9, 0.999, 1e-8, 16, 16, 1, None, 0.0, 16, None) < 0
    assert b"pinn_adam_step_sched" in lib.pinn_last_error()
    assert lib.pinn_adam_step_sched(16, 16, 16, 16, 10, None, LR0, 0.9, 0.999, 1e-8, 16, 16, 1, None, 0.0, 16, None) < 0
    assert lib.pinn_adam_step_sched(16, 16, 16, 16, 0, ok, LR0, 0.9, 0.999, 1e-8, 16, 16, 1, None, 0.0, 16, None) < 0
    assert lib.pinn_adam_step_sched(16, 16, 16, 16, 10, ok, LR0, 0.9, 0.999, 1e-8, 16, None, 1, None, 0.0, 16, None) < 0
    assert lib.pinn_adam_step_sched(16, 16, 16, 16, 10, ok, LR0, 0.9, 0.999, 1e-8, 16, 16, 1, 16, 0.0, 16, None) < 0
    assert b"max_norm" in lib.pinn_last_error()
    assert lib.pinn_adam_step_sched(16, 16, 16, 16, 10, ok, float("nan"), 0.9, 0.999, 1e-8, 16, 16, 1, None, 0.0, 16,
                                    None) < 0
    assert lib.pinn_adam_step_sched(16, 16, 16, 16, 10, ok, LR0, 0.9, 0.999, 1e-8, 16, 16, 1, None, 0.0, 12, None) < 0
