"""CPU tests of the adaptive loss-weight balancing: the engine's host logic on the oracle-backed
fakes (cadence, weights, L-BFGS freeze, L2 rejection, two gloo ranks), the solvers' lam_bcs / save path, the ev
drop-in's YAML block and the C ABI's argument checks.  The kernels are checked against the model in
test_loss_balancing_gpu.py."""
import contextlib
import ctypes
import importlib.util
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import balance_model as bm  # noqa: E402
from oracle import fwdmode_ref as fr  # noqa: E402


def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N), rng.rand(N)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, alpha_b=10.0, every=10, beta=0.1, chunk=None):
    import balance_fakes
    balance_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    e = eng.PinnEngine("cpu", 2, 10, 400.0, alpha_b=alpha_b, alpha_e=1.0)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"], chunk_points=chunk)
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    e.set_loss_balancing(every, beta)
    return e


def _reference(params0, case, steps, every, beta, alpha_b, lr, extra_eval=()):
    """fp64 trajectory: per-term oracle gradients, the model's update and combine, Adam.  Returns the weight
    after each update and the final parameters."""
    p = np.asarray(params0, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    rec = bm.initial_record(alpha_b, 0.0)
    cad = bm.Cadence(every)
    lams = []
    N, Nb = case["x"].size, case["xb"].size
    for n in range(steps):
        pairs = fr.unflatten(p, 2, 3, 2, 10)
        gr = fr.pde_loss_and_grad(pairs, case["x"], case["y"], 400.0, coef_eq=[2.0 / N] * 3 + [0.0])["grad"]
        gb = fr.bc_loss_and_grad(pairs, case["xb"], case["yb"], case["ub"], case["vb"], alpha_b=1.0, n_total=Nb)["grad"]
        for _ in range(1 + (n in extra_eval)):
            if cad.evaluate():
                rec = bm.update(bm.block_partials([gr, gb, None], p.size), p.size, 1, beta, rec)
        g = bm.combine(gr, gb, None, rec[9:11])
        p, m, v = fr.adam_step(p, g, m, v, n + 1, lr)
        cad.adam()
        lams.append(rec[9])
    return np.array(lams), p, rec


def test_lambda_trajectory_follows_the_fp64_model(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    p0 = e.net.params.numpy().copy()
    lams = []
    for _ in range(30):
        e.step(1e-3)
        lams.append(float(e.loss_weights()[0]))
    ref, p_ref, rec = _reference(p0, case, 30, 10, 0.1, 10.0, 1e-3)
    assert len(set(lams)) == 3 and lams[0] != 10.0                 # updates at n = 0, 10, 20 only
    np.testing.assert_allclose(lams, ref, rtol=2e-5)
    np.testing.assert_allclose(e.net.params.numpy(), p_ref, rtol=0, atol=2e-5)
    info = e.balance_info()
    assert info["updates"] == 3 and info["skipped"] == 0 and info["adam_updates"] == 30
    assert abs(info["lambda_b"] - rec[9]) <= 2e-5 * rec[9]
    t = e.loss_terms()
    assert float(t["lambda_b"]) == lams[-1] and float(t["lambda_s"]) == 0.0
    np.testing.assert_allclose(float(t["loss"]), float(t["loss_e"]) + lams[-1] * float(t["loss_b"]), rtol=1e-6)


def test_one_update_per_balance_index_with_an_extra_evaluation(monkeypatch):
    """A log-epoch evaluation (loss_and_grad, then adam_step) before a balance update: the rule runs once, in the
    first evaluation; the second uses the updated weight."""
    case = _case()
    e = _engine(monkeypatch, case, every=5)
    p0 = e.net.params.numpy().copy()
    extra = (0, 5, 7)
    for n in range(12):
        if n in extra:
            e.loss_and_grad()
            u = e.balance_info()["updates"]
            e.loss_and_grad()
            assert e.balance_info()["updates"] == u
            e.adam_step(1e-3)
        else:
            e.step(1e-3)
    assert e.balance_info()["updates"] == 3          # n = 0, 5, 10
    ref, p_ref, _ = _reference(p0, case, 12, 5, 0.1, 10.0, 1e-3, extra_eval=extra)
    np.testing.assert_allclose(float(e.loss_weights()[0]), ref[-1], rtol=2e-5)
    np.testing.assert_allclose(e.net.params.numpy(), p_ref, rtol=0, atol=2e-5)


def test_off_restart_and_bad_arguments(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, every=0)
    assert e.balance_info() is None and "lambda_b" not in e.loss_terms()
    assert e.loss_weights().tolist() == [10.0, 0.0]
    e.set_loss_balancing(3, 0.5)
    for _ in range(4):
        e.step(1e-3)
    assert e.balance_info()["updates"] == 2 and float(e.loss_weights()[0]) != 10.0
    e.set_loss_balancing(3, 0.5)                     # restart: configured weight, count from 0
    assert float(e.loss_weights()[0]) == 10.0 and e.balance_info()["updates"] == 0
    e.step(1e-3)
    assert e.balance_info()["updates"] == 1 and e.balance_info()["adam_updates"] == 1
    for bad in (dict(every=-1), dict(every=5, beta=0.0), dict(every=5, beta=1.5)):
        with pytest.raises(ValueError):
            e.set_loss_balancing(**bad)


def test_l2_argument_is_rejected_before_the_stream_switch(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    switched = []
    monkeypatch.setattr(torch.cuda, "set_stream", lambda s: switched.append(s))
    e.device = torch.device("cuda")                   # what decides the side-stream switch in loss_and_grad
    e._overlap = True
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: "main")
    monkeypatch.setattr(e, "_side_stream", lambda main: type("S", (), {"wait_stream": lambda self, m: None})())
    with pytest.raises(ValueError, match="MSE"):
        e.loss_and_grad("L2")
    assert switched == []
    e.device = torch.device("cpu")


def test_lambda_is_frozen_through_lbfgs(monkeypatch):
    import lbfgs_model
    from nsfnet_amd import engine as eng
    case = _case()
    e = _engine(monkeypatch, case, every=1)
    monkeypatch.setattr(eng, "LbfgsHistory", lbfgs_model.ModelHistory)
    e.step(1e-3)
    info = e.balance_info()
    lam = float(e.loss_weights()[0])
    e.lbfgs_step(lr=1.0, max_iter=4, history_size=5, line_search_fn="strong_wolfe")
    after = e.balance_info()
    assert float(e.loss_weights()[0]) == lam
    assert (after["updates"], after["skipped"], after["adam_updates"]) == (info["updates"], info["skipped"], 1)
    # the objective L-BFGS saw used that weight: its loss is the weighted one
    t = e.loss_terms()
    np.testing.assert_allclose(float(t["loss"]), float(t["loss_e"]) + lam * float(t["loss_b"]), rtol=1e-6)
    e.step(1e-3)                                      # the next Adam update balances again
    assert e.balance_info()["updates"] == 2


def test_chunked_equals_unchunked_on_the_fakes(monkeypatch):
    case = _case(N=300)
    a = _engine(monkeypatch, case, every=2)
    b = _engine(monkeypatch, case, every=2, chunk=128)
    from nsfnet_amd import engine as eng
    assert isinstance(b.plan_f, eng.ChunkedResidual) and len(b.plan_f.chunks) == 3
    for _ in range(5):
        a.step(1e-3)
        b.step(1e-3)
    np.testing.assert_allclose(b.loss_weights().numpy(), a.loss_weights().numpy(), rtol=1e-6)
    np.testing.assert_allclose(b.net.params.numpy(), a.net.params.numpy(), rtol=0, atol=1e-6)


# ---------------------------------------------------------------- two gloo ranks (ev flavour, supervised points)
def _ev_solver(monkeypatch=None):
    import balance_fakes
    balance_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    case = _case(seed=3)
    rng = np.random.RandomState(9)
    w = (0.5 + rng.rand(case["x"].size)).astype(np.float32)
    torch.manual_seed(3)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]), weights=w)
    xs, ys = rng.rand(9, 1), rng.rand(9, 1)
    P.set_supervised_data((xs, ys, np.sin(xs), np.cos(ys), xs * ys))
    P.set_supervised_loss_weight(2.0)
    P.log_interval = 1000
    P.save = lambda *a, **k: None
    P.set_loss_balancing(every=3, beta=0.2)
    return P


def _ev_train(P, n=8):
    from nsfnet_amd.pinn_solver import AdamHandle
    P.set_optimizers(AdamHandle(1e-3))
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=n, lr=1e-3)


def _gloo_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank,
                            world_size=world)
    try:
        P = _ev_solver()
        assert P.is_distributed
        _ev_train(P)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=P.engine.net.params.numpy().copy(),
                 lam=P.engine.loss_weights().numpy().copy(), rec=P.engine._bal.rec.numpy().copy())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_balancing_matches_single_process(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_gloo_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    np.testing.assert_array_equal(r0["lam"], r1["lam"])
    np.testing.assert_array_equal(r0["rec"], r1["rec"])
    np.testing.assert_array_equal(r0["params"], r1["params"])
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    P = _ev_solver(monkeypatch)
    _ev_train(P)
    rec = P.engine._bal.rec.numpy()
    assert rec[11] == 3 and rec[8] == 0 and rec[10] != 2.0      # both weights balanced at n = 0, 3, 6
    np.testing.assert_allclose(r0["rec"], rec, rtol=1e-5)
    np.testing.assert_allclose(r0["params"], P.engine.net.params.numpy(), rtol=0, atol=1e-6)


# ---------------------------------------------------------------- solvers: lam_bcs, save path, log line
def test_solvers_write_the_current_weight_keep_the_configured_path_and_refuse_l2(monkeypatch, tmp_path):
    import scipy.io
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    P = _ev_solver(monkeypatch)
    del P.save
    out = io.StringIO()
    from nsfnet_amd.pinn_solver import AdamHandle
    P.set_optimizers(AdamHandle(1e-3))
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=2, lr=1e-3)
    assert "lambda_b=" in out.getvalue() and "lambda_s=" in out.getvalue()
    lam = float(P.engine.loss_weights()[0])
    assert lam != 10.0 and P.alpha_b == 10
    case = _case()
    with contextlib.redirect_stdout(io.StringIO()):
        P.test(case["x"].reshape(-1, 1), case["y"].reshape(-1, 1), case["x"], case["y"], case["x"], loop=1,
               save_dir=str(tmp_path / "t"))
    assert float(scipy.io.loadmat(str(tmp_path / "t" / "cavity_result_loop_1.mat"))["lam_bcs"].item()) == pytest.approx(lam)
    P.save("m.pth", directory=str(tmp_path), N_HLayer=2, N_neu=10, N_f=70)
    assert len(list(tmp_path.glob("results/Re800/*lamB10_*/m.pth"))) == 1

    from nsfnet_amd import pinn_solver as ps
    Q = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=10, N_f=70, bc_weight=10, eq_weight=1)
    Q.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    Q.set_eq_training_data(X=(case["x"].reshape(-1, 1), case["y"].reshape(-1, 1)))
    Q.set_loss_balancing(every=1)
    Q.set_optimizers(AdamHandle(1e-3))
    Q.log_every, Q.save_every = 1, 0
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        Q.train(num_epoch=2, lr=1e-3)
    lam = float(Q.engine.loss_weights()[0])
    assert "lambda_b: " in out.getvalue() and lam != 10.0 and Q.alpha_b == 10
    with contextlib.redirect_stdout(io.StringIO()):
        Q.test(case["x"], case["y"], case["x"], case["y"], loop=2)
    assert float(scipy.io.loadmat(str(tmp_path / "cavity_result_loop_2.mat"))["lam_bcs"].item()) == pytest.approx(lam)
    Q.save("q.pth", directory=str(tmp_path), N_HLayer=2, N_neu=10, N_f=70)
    assert len(list(tmp_path.glob("results/Re400/*lamB10*/q.pth"))) == 1
    with pytest.raises(ValueError, match="MSE"):
        Q.fwd_computing_loss_2d(loss_mode="L2")
    _assert_next_published_loss_is_mse(Q)


def _assert_next_published_loss_is_mse(P):
    """After a refused L2 call, the next Adam epoch publishes the MSE terms, not 2-norms of the same sums."""
    P.log_every = P.save_every = 0
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=1, lr=1e-3)
    mse, l2 = P.engine.loss_terms(), P.engine.loss_terms("L2")
    for k in ("loss", "loss_e", "loss_b"):
        assert float(getattr(P, k)) == float(mse[k]) != float(l2[k]), k


def test_refused_l2_call_leaves_the_solver_on_mse(monkeypatch):
    """A chunked collocation set refuses the L2 mode; the solver then goes on publishing MSE terms."""
    import fakes
    from nsfnet_amd import pinn_solver as ps
    fakes.install(monkeypatch)
    monkeypatch.setenv("NSFNET_CHUNK_POINTS", "128")
    case = _case(N=300)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=10, N_f=70, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"].reshape(-1, 1), case["y"].reshape(-1, 1)))
    with pytest.raises(NotImplementedError, match="L2"):
        P.fwd_computing_loss_2d(loss_mode="L2")
    _assert_next_published_loss_is_mse(P)


# ---------------------------------------------------------------- ev drop-in YAML
def _config_module():
    path = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py")
    spec = importlib.util.spec_from_file_location("ev_dropin_config_balance", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_ev_config_parses_and_validates_loss_balancing(tmp_path):
    cfg = _config_module()
    mgr = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml"))
    lb = mgr.config.training.loss_balancing
    assert (lb.enabled, lb.every, lb.beta) == (False, 100, 0.1)
    p = tmp_path / "lb.yaml"
    p.write_text("training:\n  loss_balancing: {enabled: true, every: 50, beta: 0.25}\n")
    mgr = cfg.ConfigManager.from_file(str(p))
    lb = mgr.config.training.loss_balancing
    assert (lb.enabled, lb.every, lb.beta) == (True, 50, 0.25)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mgr.print_config()
    assert "balancing  : every=50 beta=0.25" in out.getvalue()
    for bad in ("{enabled: true, every: 0}", "{enabled: true, beta: 0}", "{enabled: true, beta: 1.5}"):
        p.write_text("training:\n  loss_balancing: %s\n" % bad)
        with pytest.raises(ValueError, match="loss_balancing"):
            cfg.ConfigManager.from_file(str(p))


# ---------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def test_balance_entry_points_are_declared_and_reject_bad_arguments(lib):
    from nsfnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nsfnet_pinn.h")).read()
    for name in ("pinn_balance_partials_count", "pinn_grad_reduce_terms", "pinn_balance_stats", "pinn_balance_update",
                 "pinn_balance_combine"):
        assert name in hdr and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.pinn_abi_version() == 3
    assert lib.pinn_balance_partials_count(1) == 6 and lib.pinn_balance_partials_count(65) == 12
    assert lib.pinn_balance_partials_count(0) == -1
    buf = ctypes.c_void_p(16)        # never dereferenced: every call below fails its argument check
    assert lib.pinn_balance_update(buf, 10, 1, 0.0, buf, buf, None) != 0
    assert b"beta" in lib.pinn_last_error()
    assert lib.pinn_balance_update(buf, 10, 4, 0.1, buf, buf, None) != 0
    assert lib.pinn_balance_update(buf, 0, 1, 0.1, buf, buf, None) != 0
    assert lib.pinn_balance_combine(buf, buf, None, None, buf, 10, None) != 0
    vec = (ctypes.c_void_p * 3)(16, 16, 16)
    assert lib.pinn_balance_stats(vec, 0, buf, None) != 0
    h = ctypes.c_void_p()
    assert lib.pinn_net_create(3, 2, 16, ctypes.byref(h)) == 0
    try:
        ns = (ctypes.c_int * 3)(0, 0, 0)
        outs = (ctypes.c_void_p * 3)(16, None, None)
        plans = (ctypes.c_void_p * 1)(None)
        assert lib.pinn_grad_reduce_terms(h, ns, plans, plans, outs, 0, None, None) != 0     # no source
        ns = (ctypes.c_int * 3)(0, 1, 0)
        assert lib.pinn_grad_reduce_terms(h, ns, plans, plans, outs, 0, None, None) != 0     # group 1 has no output
        assert b"output" in lib.pinn_last_error()
    finally:
        lib.pinn_net_destroy(h)
