"""CPU tests of the conflict-free combination of the per-term gradients: the fp64 model against
the paper's pseudo-inverse definition, the engine's host logic on the oracle-backed fakes (trajectory, chunked passes,
two gloo ranks, refusals, the L-BFGS freeze), the ev drop-in's YAML block and the C ABI's argument checks.  The
kernels are checked against the model in test_confgrad_gpu.py."""
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

import confgrad_model as cm  # noqa: E402
from oracle import fwdmode_ref as fr  # noqa: E402

LR = 1e-3


# ---------------------------------------------------------------- the model itself
@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_equals_the_pinv_definition(m, seed):
    rng = np.random.RandomState(seed)
    P = 500
    vecs = [rng.randn(P) * s for s in (3.0, 0.05, 1e-3)[:m]] + [None] * (3 - m)
    vecs[1] = vecs[1] + 0.3 * vecs[0] * 0.05 / 3.0                  # a visible cosine
    rec = cm.coefficients(cm.sum_partials(cm.block_partials(vecs, P)), m)
    g = cm.combine(vecs[0], vecs[1], vecs[2], rec[6:9])
    ref = cm.config_pinv(vecs)
    assert np.abs(g - ref).max() <= 1e-12 * np.abs(ref).max()
    assert rec[10] == 1 and rec[11] == 0 and rec[12] == 0
    assert abs(rec[9] - np.linalg.norm(ref)) <= 1e-12 * rec[9]
    # equal positive projection on every unit term gradient
    proj = [g @ v / np.linalg.norm(v) for v in vecs if v is not None]
    assert np.ptp(proj) <= 1e-12 * max(proj) and min(proj) > 0


def test_two_term_closed_form():
    rng = np.random.RandomState(7)
    gr, gb = rng.randn(300) * 2.0, rng.randn(300) * 1e-2
    for mix in (0.0, 0.9, -0.9):                                    # independent of the cosine
        b = gb + mix * gr * 1e-2
        rec = cm.coefficients(cm.sum_partials(cm.block_partials([gr, b, None], 300)), 2)
        nr, nb = np.linalg.norm(gr), np.linalg.norm(b)
        np.testing.assert_allclose(rec[6:8], [(nr + nb) / (2 * nr), (nr + nb) / (2 * nb)], rtol=1e-12)
        assert rec[8] == 0.0


def test_model_guards():
    rng = np.random.RandomState(3)
    r, b, s = rng.randn(130), rng.randn(130), rng.randn(130)
    z = np.zeros(130)

    def rec(vecs, m):
        return cm.coefficients(cm.sum_partials(cm.block_partials(vecs, 130)), m)

    x = rec([r, z, s], 3)                                            # a zero-norm term leaves the set
    assert x[12] == 1 and x[11] == 0 and x[7] == 0 and x[6] > 0 and x[8] > 0
    x = rec([r, z, None], 2)                                         # one term left: that term
    assert x[12] == 1 and x[11] == 0 and list(x[6:9]) == [1.0, 0.0, 0.0] and x[9] == x[0]
    np.testing.assert_allclose(x[0], np.linalg.norm(r), rtol=1e-12)
    x = rec([z, z, z], 3)                                            # none left: g = 0
    assert x[12] == 3 and x[11] == 0 and list(x[6:9]) == [0.0, 0.0, 0.0] and x[9] == 0.0
    bad = s.copy(); bad[5] = np.nan
    x = rec([r, b, bad], 3)                                          # non-finite: the plain sum
    assert x[11] == 1 and x[12] == 0 and list(x[6:9]) == [1.0, 1.0, 1.0]
    x = rec([r, -2.0 * r, s], 3)                                     # anti-parallel: no such direction
    assert x[11] == 1 and list(x[6:9]) == [1.0, 1.0, 1.0]
    np.testing.assert_allclose(x[9], np.linalg.norm(r - 2.0 * r + s), rtol=1e-12)
    x = rec([r, 3.0 * r, None], 2)                                   # parallel to every digit: det = 0
    assert x[11] == 1
    x = cm.coefficients(cm.sum_partials(cm.block_partials([r[:1], b[:1], s[:1]], 1)), 3)
    assert x[11] == 1                                                # one parameter: every cosine is +-1


# ---------------------------------------------------------------- engine on the fakes
def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N), rng.rand(N)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, alpha_b=10.0, on=True, chunk=None):
    import confgrad_fakes
    confgrad_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    e = eng.PinnEngine("cpu", 2, 10, 400.0, alpha_b=alpha_b, alpha_e=1.0)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"], chunk_points=chunk)
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    if on:
        e.set_conflict_free_gradients()
    return e


def _reference(params0, case, steps, alpha_b, lr):
    """fp64 trajectory: per-term oracle gradients (alpha_b baked in), the model's rule, Adam."""
    p = np.asarray(params0, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    rec = None
    N, Nb = case["x"].size, case["xb"].size
    for n in range(steps):
        pairs = fr.unflatten(p, 2, 3, 2, 10)
        gr = fr.pde_loss_and_grad(pairs, case["x"], case["y"], 400.0, coef_eq=[2.0 / N] * 3 + [0.0])["grad"]
        gb = fr.bc_loss_and_grad(pairs, case["xb"], case["yb"], case["ub"], case["vb"], alpha_b=alpha_b,
                                 n_total=Nb)["grad"]
        g, rec = cm.step([gr, gb, None], rec)
        p, m, v = fr.adam_step(p, g, m, v, n + 1, lr)
    return p, rec


@pytest.mark.parametrize("N,chunk", [(70, None), (300, 128)])       # 128: the chunk granularity, 300 points = 3 passes
def test_adam_trajectory_follows_the_fp64_model(monkeypatch, N, chunk):
    import confgrad_fakes
    case = _case(N=N)
    e = _engine(monkeypatch, case, chunk=chunk)
    if chunk:
        from nsfnet_amd import engine as eng
        assert isinstance(e.plan_f, eng.ChunkedResidual) and len(e.plan_f.chunks) == 3
    p0 = e.net.params.numpy().copy()
    t0 = None
    for n in range(20):
        del confgrad_fakes.CALLS[:]
        e.step(LR)
        if n == 0:
            t0 = {k: float(v) for k, v in e.loss_terms().items()}
            assert confgrad_fakes.CALLS == (["grad_reduce_terms"] * 2 if chunk else []) + [
                "grad_reduce_terms_gram", "confgrad_coef", "confgrad_combine"]
    p_ref, rec = _reference(p0, case, 20, 10.0, LR)
    np.testing.assert_allclose(e.net.params.numpy(), p_ref, rtol=0, atol=2e-5)
    info = e.conflict_info()
    assert info["steps"] == 20 and info["fallbacks"] == 0 and info["dropped"] == 0
    for key, want in (("n_r", rec[0]), ("n_b", rec[1]), ("k_r", rec[6]), ("k_b", rec[7]), ("norm", rec[9])):
        assert abs(info[key] - want) <= 1e-3 * abs(want), key
    assert abs(info["cos_rb"] - rec[3]) <= 1e-3 and info["k_s"] == 0.0 and info["n_s"] == 0.0
    # the logged loss stays the alpha-weighted sum
    np.testing.assert_allclose(t0["loss"], t0["loss_e"] + 10.0 * t0["loss_b"], rtol=1e-6)
    assert "lambda_b" not in t0


def test_off_by_default_and_switching_off_restores_the_plain_calls(monkeypatch):
    import confgrad_fakes
    case = _case()
    a = _engine(monkeypatch, case, on=False)
    b = _engine(monkeypatch, case, on=True)
    assert a.conflict_info() is None and b.conflict_info()["steps"] == 0
    b.step(LR)
    assert b.conflict_info()["steps"] == 1
    b.set_conflict_free_gradients(True)                              # a call restarts the counters
    assert b.conflict_info()["steps"] == 0
    b.set_conflict_free_gradients(False)
    assert b.conflict_info() is None
    b.net.set_flat(a.net.params.clone())
    b.net.m.zero_(); b.net.v.zero_(); b.net.adam_t = 0
    logs = []
    for e in (a, b):
        del confgrad_fakes.CALLS[:]
        e.step(LR)
        logs.append(list(confgrad_fakes.CALLS))
    assert logs[0] == logs[1] == ["grad_reduce"]
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())


def test_refused_with_loss_balancing_in_both_orders(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, on=False)
    e.set_loss_balancing(5, 0.1)
    with pytest.raises(ValueError, match="loss balancing"):
        e.set_conflict_free_gradients()
    assert e.conflict_info() is None and e.balance_info() is not None
    e.set_loss_balancing(0)
    e.set_conflict_free_gradients()
    with pytest.raises(ValueError, match="conflict-free"):
        e.set_loss_balancing(5, 0.1)
    assert e.balance_info() is None and e.conflict_info() is not None
    e.set_loss_balancing(0)                                          # switching the other one off is no conflict
    e.set_conflict_free_gradients(False)
    e.set_loss_balancing(5, 0.1)
    e.step(LR)


def test_l2_is_refused_before_the_stream_switch(monkeypatch):
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


def test_lbfgs_uses_the_plain_sum_and_leaves_the_record_alone(monkeypatch):
    import confgrad_fakes
    import lbfgs_model
    from nsfnet_amd import engine as eng
    case = _case()
    e = _engine(monkeypatch, case)
    monkeypatch.setattr(eng, "LbfgsHistory", lbfgs_model.ModelHistory)
    e.step(LR)
    rec = e._cfg.rec.numpy().copy()
    del confgrad_fakes.CALLS[:]
    e.lbfgs_step(lr=1.0, max_iter=4, history_size=5, line_search_fn="strong_wolfe")
    assert confgrad_fakes.CALLS and set(confgrad_fakes.CALLS) == {"grad_reduce"}
    np.testing.assert_array_equal(e._cfg.rec.numpy(), rec)
    assert not e._cfg_frozen
    e.step(LR)                                        # the next Adam update combines again
    assert e.conflict_info()["steps"] == 2


def test_graph_key_names_the_feature(monkeypatch):
    case = _case()
    keys = []

    class Stop(Exception):
        pass

    class Probe(dict):
        def get(self, key, default=None):
            keys.append(key)
            raise Stop

        def clear(self):
            pass

    for on in (False, True):
        e = _engine(monkeypatch, case, on=on)
        monkeypatch.setattr(e, "_graphs_enabled", lambda: True)
        e._graphs = Probe()
        with pytest.raises(Stop):
            e.step(LR)
    assert keys[1] == keys[0] + ("confgrad",)


# ---------------------------------------------------------------- two gloo ranks (ev flavour, supervised points)
def _ev_solver(monkeypatch=None):
    import confgrad_fakes
    confgrad_fakes.install(monkeypatch)
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
    P.set_conflict_free_gradients(True)
    return P


def _ev_train(P, n=20):
    from nsfnet_amd.pinn_solver import AdamHandle
    P.set_optimizers(AdamHandle(LR))
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=n, lr=LR)


def _gloo_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank,
                            world_size=world)
    try:
        import confgrad_fakes
        P = _ev_solver()
        assert P.is_distributed
        _ev_train(P)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=P.engine.net.params.numpy().copy(),
                 coef=P.engine._cfg.coef.numpy().copy(), rec=P.engine._cfg.rec.numpy().copy(),
                 gram_calls=confgrad_fakes.CALLS.count("confgrad_gram"),
                 fused_calls=confgrad_fakes.CALLS.count("grad_reduce_terms_gram"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_are_bit_identical_and_match_one_rank_on_the_union(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_gloo_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    for k in ("coef", "rec", "params"):
        np.testing.assert_array_equal(r0[k], r1[k])
    assert r0["gram_calls"] == 20 and r0["fused_calls"] == 0         # statistics of the all-reduced vectors, every step
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    P = _ev_solver(monkeypatch)
    _ev_train(P)
    rec = P.engine._cfg.rec.numpy()
    assert rec[10] == 20 and rec[11] == 0 and rec[12] == 0 and (rec[6:9] > 0).all()      # three terms, no guard
    # the ranks add fp32 shard vectors where one rank rounds the fp64 sum once: a few fp32 ulps per entry
    np.testing.assert_allclose(r0["rec"], rec, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r0["params"], P.engine.net.params.numpy(), rtol=0, atol=1e-6)


def test_solvers_expose_the_setter_and_log_the_record(monkeypatch):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    P = _ev_solver(monkeypatch)
    P.log_interval = 1
    out = io.StringIO()
    from nsfnet_amd.pinn_solver import AdamHandle
    P.set_optimizers(AdamHandle(LR))
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=2, lr=LR)
    assert "conflict-free: |g_r|=" in out.getvalue() and "fallbacks=0/" in out.getvalue()
    with pytest.raises(ValueError, match="conflict-free"):
        P.set_loss_balancing(every=3)

    from nsfnet_amd import pinn_solver as ps
    case = _case()
    Q = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=10, N_f=70, bc_weight=10, eq_weight=1)
    Q.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    Q.set_eq_training_data(X=(case["x"].reshape(-1, 1), case["y"].reshape(-1, 1)))
    Q.set_conflict_free_gradients()
    Q.set_optimizers(AdamHandle(LR))
    Q.log_every, Q.save_every = 1, 0
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        Q.train(num_epoch=2, lr=LR)
    assert "conflict-free: |g_r|=" in out.getvalue()
    assert Q.engine.conflict_info()["steps"] >= 2 and Q.lam_b() == 10
    with pytest.raises(ValueError, match="MSE"):
        Q.fwd_computing_loss_2d(loss_mode="L2")
    Q.set_conflict_free_gradients(False)
    assert Q.engine.conflict_info() is None and not Q._confgrad


# ---------------------------------------------------------------- ev drop-in YAML
def _config_module():
    path = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py")
    spec = importlib.util.spec_from_file_location("ev_dropin_config_confgrad", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_ev_config_parses_the_block_and_refuses_both_rules(tmp_path):
    cfg = _config_module()
    mgr = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml"))
    assert mgr.config.training.conflict_free_gradients.enabled is False
    assert cfg.AppConfig().training.conflict_free_gradients.enabled is False
    p = tmp_path / "cf.yaml"
    p.write_text("training:\n  conflict_free_gradients: {enabled: true}\n")
    mgr = cfg.ConfigManager.from_file(str(p))
    assert mgr.config.training.conflict_free_gradients.enabled is True
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mgr.print_config()
    assert "conflict-free gradients: on" in out.getvalue()
    p.write_text("training:\n  conflict_free_gradients: {enabled: true}\n  loss_balancing: {enabled: true}\n")
    with pytest.raises(ValueError, match="conflict_free_gradients and training.loss_balancing"):
        cfg.ConfigManager.from_file(str(p))
    p.write_text("training:\n  loss_balancing: {enabled: true}\n")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "conflict-free" not in out.getvalue()


# ---------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def test_confgrad_entry_points_are_declared_and_reject_bad_arguments(lib):
    from nsfnet_amd import _lib, engine as eng
    hdr = open(os.path.join(ROOT, "include", "nsfnet_pinn.h")).read()
    for name in ("pinn_confgrad_partials_count", "pinn_confgrad_gram", "pinn_confgrad_coef", "pinn_confgrad_combine",
                 "pinn_grad_reduce_terms_gram"):
        assert name in hdr and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define PINN_CONFGRAD_RECORD %d" % cm.RECORD in hdr and eng.CONFGRAD_RECORD == cm.RECORD
    assert lib.pinn_abi_version() == 3
    assert lib.pinn_confgrad_partials_count(1) == 6 and lib.pinn_confgrad_partials_count(65) == 12
    assert lib.pinn_confgrad_partials_count(0) == -1
    buf = ctypes.c_void_p(16)        # never dereferenced: every call below fails its argument check
    vec = (ctypes.c_void_p * 3)(16, 16, 16)
    assert lib.pinn_confgrad_gram(vec, 0, buf, None) != 0
    assert lib.pinn_confgrad_gram(vec, 10, None, None) != 0
    assert lib.pinn_confgrad_coef(buf, 10, 2, buf, None, None) != 0             # NULL record
    assert b"null" in lib.pinn_last_error()
    assert lib.pinn_confgrad_coef(buf, 0, 2, buf, buf, None) != 0
    assert lib.pinn_confgrad_coef(buf, -5, 2, buf, buf, None) != 0
    assert lib.pinn_confgrad_coef(buf, 10, 1, buf, buf, None) != 0
    assert b"nterms" in lib.pinn_last_error()
    assert lib.pinn_confgrad_coef(buf, 10, 4, buf, buf, None) != 0
    assert lib.pinn_confgrad_combine(buf, buf, None, None, buf, 10, None) != 0
    assert lib.pinn_confgrad_combine(buf, buf, buf, None, buf, 0, None) != 0
    h = ctypes.c_void_p()
    assert lib.pinn_net_create(3, 2, 16, ctypes.byref(h)) == 0
    try:
        ns = (ctypes.c_int * 3)(0, 0, 0)
        outs = (ctypes.c_void_p * 3)(16, None, None)
        plans = (ctypes.c_void_p * 1)(None)
        assert lib.pinn_grad_reduce_terms_gram(h, ns, plans, plans, outs, 0, None, buf, None) != 0    # no source
        ns = (ctypes.c_int * 3)(0, 1, 0)
        assert lib.pinn_grad_reduce_terms_gram(h, ns, plans, plans, outs, 0, None, buf, None) != 0    # group 1: no output
        assert b"pinn_grad_reduce_terms_gram" in lib.pinn_last_error() and b"output" in lib.pinn_last_error()
    finally:
        lib.pinn_net_destroy(h)


# ---------------------------------------------------------------- the fold model both statistics models are built on
def test_fold_model_orders_against_scalar_loops():
    """tests/fold_model.py against the device orders written out as scalar loops, at sizes with a ragged last wave,
    block and stride, and against np.sum, from which the fixed order must differ somewhere (or a bitwise test on it
    would pin nothing)."""
    from fractions import Fraction
    import fold_model as fm
    rng = np.random.RandomState(0)
    vec = lambda n: rng.randn(n) * 10.0 ** rng.uniform(-4, 1, size=n)
    v = vec(64)
    lanes = list(v)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[i] + lanes[i + off] if i + off < 64 else lanes[i] for i in range(64)]
    assert fm.wave_fold(v) == lanes[0]
    p = vec(601)
    acc = [0.0] * 256
    for b in range(601):
        acc[b % 256] += p[b]
    half = 128
    while half:
        acc = [acc[i] + acc[i + half] for i in range(half)]
        half //= 2
    assert fm.strided_tree_fold(p[:, None], [fm.SUM])[0] == acc[0]
    chunks = [0.0] * 256
    for b in range(601):
        chunks[b // 3] += p[b]                          # ceil(601 / 256) = 3 per thread
    tot = 0.0
    for c in chunks:
        tot += c
    assert fm.chunk_fold(p) == tot
    pm = np.abs(p); pm[77] = np.nan
    assert np.isnan(fm.strided_tree_fold(pm[:, None], [fm.NANMAX])[0]) and np.isnan(fm.chunk_fold(pm, fm.NANMAX))
    assert fm.strided_tree_fold(p[:, None], [fm.MIN])[0] == p.min() and fm.strided_tree_fold(p[:, None], [fm.MAX])[0] == p.max()
    n, nblk = 2 * 2 * 256 * 4 + 5, 2                    # the stride repeats, the last pass is ragged
    v = vec(n)
    parts = []
    for b in range(nblk):
        th = [0.0] * 256
        for t in range(256):
            for base in range((b * 256 + t) * 4, n, nblk * 1024):
                for j in range(4):
                    if base + j < n:
                        th[t] += v[base + j]
        waves = [fm.wave_fold(np.array(th[w * 64:(w + 1) * 64])) for w in range(4)]
        parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    np.testing.assert_array_equal(fm.grid_partials(v, nblk), parts)
    assert fm.grid_fold(v, nblk) == parts[0] + parts[1]
    assert any(fm.grid_fold(v, min(-(-v.size // 1024), 512)) != np.sum(v) for v in map(vec, (1003, 70001, 330499)))
    a, b, c = vec(500), vec(500), vec(500)
    c[:250] = -(a * b)[:250]                            # cancellation: what is left is the product's rounding error
    want = [float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)]
    np.testing.assert_array_equal(fm.fma(a, b, c), want)
    assert (fm.fma(a, b, c) != a * b + c).any()
    th = np.zeros(256)                                  # one block of 256 threads x 4 entries over 500 products
    for i in range(500):
        th[i // 4] = fm.fma(a[i:i + 1], b[i:i + 1], th[i // 4:i // 4 + 1])[0]
    assert fm.same_bits(fm.grid_partials((a, b), 1), fm.block_fold(th))
