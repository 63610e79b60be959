"""CPU checks of residual-based resampling of the collocation points: the C ABI entry points (declared, exported,
bound; bad arguments rejected before any HIP call), the numpy replay of the selection math, the per-rank
semantics under a two-rank gloo run with numpy stand-ins for the two device primitives, the solvers' schedule,
and the ev drop-in's configuration.  The device kernels themselves are covered by test_resample_gpu.py."""
import ctypes
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
import resample_replay as rr  # noqa: E402

NAMES = ("pinn_resample_scratch_bytes", "pinn_resample_select", "pinn_resample_gather")


@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def test_resample_entry_points_are_declared_exported_and_bound(lib):
    from nsfnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "nsfnet_pinn.h")).read()
    for n in NAMES:
        assert n + "(" in header, n
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.pinn_abi_version() == 3


def test_resample_entry_points_reject_bad_arguments(lib):
    P = ctypes.c_void_p
    fld, scr, out = P(256), P(512), P(1024)          # never dereferenced: every case fails validation first
    assert lib.pinn_resample_scratch_bytes(0) == -1
    nb = (1000003 + 1023) // 1024
    assert lib.pinn_resample_scratch_bytes(1000003) >= 16 * nb

    def sel(n=100, f=fld, npad=128, w4=0.0, k=1.0, c=1.0, u=0.5, m=10, s=scr, o=out):
        return lib.pinn_resample_select(n, f, npad, w4, k, c, u, m, s, o, None)

    for kw, msg in ((dict(f=None), b"null argument"), (dict(s=None), b"null argument"), (dict(o=None), b"null argument"),
                    (dict(n=0), b"pool size"), (dict(m=0), b"m must be"), (dict(npad=64), b"npad"),
                    (dict(npad=130), b"npad"), (dict(f=P(260)), b"aligned"),
                    (dict(k=-1.0), b"k must be"), (dict(k=float("nan")), b"k must be"), (dict(k=float("inf")), b"k must be"),
                    (dict(c=-0.5), b"c must be"), (dict(c=float("nan")), b"c must be"),
                    (dict(w4=-0.1), b"w4 must be"), (dict(u=1.0), b"u must be"), (dict(u=-1e-3), b"u must be"),
                    (dict(u=float("nan")), b"u must be")):
        assert sel(**kw) < 0, kw
        assert msg in lib.pinn_last_error(), (kw, lib.pinn_last_error())

    def gat(idx=out, lo=0, hi=10, n=100, sx=fld, sy=fld, sw=None, sv=None, dx=fld, dy=fld, dw=None, dv=None, s=scr, ws=None):
        return lib.pinn_resample_gather(idx, lo, hi, n, sx, sy, sw, sv, dx, dy, dw, dv, s, ws, None)

    for kw, msg in ((dict(idx=None), b"null argument"), (dict(sx=None), b"null argument"), (dict(dy=None), b"null argument"),
                    (dict(s=None), b"null argument"), (dict(n=0), b"pool size"), (dict(lo=-1), b"lo < hi"),
                    (dict(lo=5, hi=5), b"lo < hi"), (dict(sw=fld), b"src_w and dst_w"), (dict(dv=fld), b"src_vtm and dst_vtm"),
                    (dict(ws=scr), b"w_sum needs")):
        assert gat(**kw) < 0, kw
        assert msg in lib.pinn_last_error(), (kw, lib.pinn_last_error())


# ---------------------------------------------------------------- the selection math (numpy replay)
# These check the oracle itself (tests/resample_replay.py), which test_resample_gpu.py holds the kernels to; the
# feature's own CPU coverage is the ABI, gloo and schedule tests below.
def _eq(n, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((4, n)) * scale).astype(np.float32)


@pytest.mark.parametrize("k,c", [(0.0, 0.0), (1.0, 1.0), (2.0, 0.0), (1.5, 0.3)])
def test_selection_counts_sum_to_m_and_indices_ascend(k, c):
    eq = _eq(5003)
    for u in (0.0, 0.37, 0.999):
        idx, S = rr.select(eq, 0.1, k, c, u, 1777)
        assert idx.size == 1777 and S > 0
        assert np.all(np.diff(idx) >= 0) and idx[0] >= 0 and idx[-1] < 5003
        o = rr.offsets_of(idx, 5003)
        assert o[-1] == 1777 and np.array_equal(o, rr.offsets(eq, 0.1, k, c, u, 1777)[0])


def test_k0_takes_every_n_over_m_th_point():
    eq = _eq(1000, scale=1e3)
    idx, _ = rr.select(eq, 0.1, 0.0, 1.0, 0.0, 100)
    assert np.array_equal(idx, np.arange(9, 1000, 10))
    idx, _ = rr.select(eq, 0.1, 0.0, 0.0, 0.55, 100)
    assert np.array_equal(np.diff(idx), np.full(99, 10))


def test_frequencies_follow_the_density():
    """Systematic resampling: every point's count is within one of M b_i / T."""
    eq = _eq(50, seed=3)
    eq[:, 7] = 0.0                                          # a point with no residual: only c keeps it alive
    for k, c in ((1.0, 1.0), (2.0, 0.0), (1.0, 0.0)):
        M = 1_000_000
        idx, _ = rr.select(eq, 0.1, k, c, 0.25, M)
        counts = np.bincount(idx, minlength=50)
        b, _ = rr.density(eq, 0.1, k, c)
        expect = M * b / b.sum()
        assert np.all(np.abs(counts - expect) < 1.0), (k, c)
        if c == 0.0:
            assert counts[7] == 0


def test_w4_weights_eq4_and_zero_residual_is_uniform():
    eq = _eq(64)
    eq4_only = np.zeros_like(eq)
    eq4_only[3] = eq[3]
    idx, S = rr.select(eq4_only, 0.0, 1.0, 0.0, 0.5, 64)      # w4 = 0 (plain flavour): every residual is 0
    assert S == 0.0 and np.array_equal(idx, np.arange(64))
    e2 = rr.residual_sq(eq4_only, 0.1)
    assert np.allclose(e2, 0.1 * eq[3].astype(np.float64) ** 2, rtol=1e-15, atol=0)


# ---------------------------------------------------------------- numpy stand-ins for the device primitives
def fake_resample_scratch(n_pool, device):
    return torch.zeros(8, dtype=torch.uint8)


def fake_resample_select(pool, w4, k, c, u, m, scratch):
    eq = pool.fields.numpy()[6:10, :pool.n]
    S = rr.density(eq, w4, k, c)[1]
    if not np.isfinite(S):               # (the device call, too, returns S and leaves the judgement to the caller)
        return torch.zeros(m, dtype=torch.int64), S
    return torch.as_tensor(rr.select(eq, w4, k, c, u, m)[0]), S


def fake_resample_gather(idx, lo, hi, n_pool, src, dst, scratch, w_sum=None):
    sel = idx[lo:hi]
    for name in ("x", "y", "w", "vtm"):
        if src.get(name) is not None and dst.get(name) is not None:
            dst[name].copy_(src[name][sel])
    if w_sum is not None:
        s = 0.0
        for v in src["w"][sel].numpy().astype(np.float64):
            s += v
        w_sum[0] = s


def install_fakes(monkeypatch=None):
    import fakes
    from nsfnet_amd import engine as eng
    fakes.install(monkeypatch)
    for name, val in (("resample_scratch", fake_resample_scratch), ("resample_select", fake_resample_select),
                      ("resample_gather", fake_resample_gather)):
        if monkeypatch is not None:
            monkeypatch.setattr(eng, name, val)
        else:
            setattr(eng, name, val)


def _case():
    rng = np.random.RandomState(7)
    N, NP = 70, 203
    from oracle import autograd_ref as ar
    xb, yb, ub, vb = (a[::63][:33] for a in ar.cavity_boundary())
    return dict(x=rng.rand(N, 1), y=rng.rand(N, 1), w=(0.5 + rng.rand(N)).astype(np.float32),
                xp=rng.rand(NP, 1), yp=rng.rand(NP, 1), wp=(0.5 + rng.rand(NP)).astype(np.float32),
                xb=xb, yb=yb, ub=ub, vb=vb)


def _ev_solver(case, monkeypatch=None):
    install_fakes(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(3)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]), weights=case["w"])
    P.set_resample_pool(X=(case["xp"], case["yp"]), weights=case["wp"])
    P.log_interval = 1000
    P.save = lambda *a, **k: None
    return P


def _run_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        P = _ev_solver(_case())
        assert P.is_distributed
        params = P.engine.net.params.numpy().copy()
        idx = P.resample_collocation(k=1.0, c=1.0, seed=11).numpy().copy()
        rec = dict(idx=idx, x=P.x_f.numpy().reshape(-1), y=P.y_f.numpy().reshape(-1), w=P.eq_weights.numpy().copy(),
                   vtm=P.vis_t_minus.numpy().reshape(-1), params=params, n_f_global=P.engine.n_f_global)
        with contextlib.redirect_stdout(io.StringIO()):
            P.train(num_epoch=2, lr=1e-3)
        rec["params_after"] = P.engine.net.params.numpy().copy()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **rec)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_resampling_matches_single_process(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_run_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r = [np.load(tmp_path / ("rank%d.npz" % k)) for k in range(world)]
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    case = _case()
    P = _ev_solver(case, monkeypatch)
    assert not P.is_distributed
    np.testing.assert_array_equal(P.engine.net.params.numpy(), r[0]["params"])
    import fakes
    E = P.engine
    xp, yp, wp = (np.asarray(case[k], dtype=np.float32).reshape(-1) for k in ("xp", "yp", "wp"))
    want, wsums = [], []
    for rank, (lo, hi) in enumerate(((0, 101), (101, 203))):           # pool shards: contiguous, last takes the remainder
        pe = fakes.FakeValuePlan(E.net_e, xp[lo:hi], yp[lo:hi])
        pe.forward()
        e = pe.pred[0]
        pool = fakes.FakeResidualPlan(E.net, xp[lo:hi], yp[lo:hi])
        vtm0 = (E.alpha_evm * e.abs()).contiguous()
        pool.vis_t_minus = vtm0.clone()
        pool.forward(E.Re, e=e, vis_t0=E.vis_t0, alpha_evm=E.alpha_evm, scale=E.scale, save=False)
        u = np.random.default_rng([11, 0, rank]).random()
        idx, _ = rr.select(pool.fields.numpy()[6:10, :pool.n], 0.1, 1.0, 1.0, u, 35)
        s = 0.0
        for v in wp[lo:hi][idx].astype(np.float64):
            s += v
        wsums.append(s)
        want.append((idx, xp[lo:hi][idx], yp[lo:hi][idx], wp[lo:hi][idx], vtm0.numpy()[idx]))
    mean = (wsums[0] + wsums[1]) / 70
    for rank in range(world):
        idx, x, y, w, vtm = want[rank]
        assert int(r[rank]["n_f_global"]) == 70
        np.testing.assert_array_equal(r[rank]["idx"], idx)
        np.testing.assert_array_equal(r[rank]["x"], x)
        np.testing.assert_array_equal(r[rank]["y"], y)
        np.testing.assert_array_equal(r[rank]["vtm"], vtm)
        np.testing.assert_array_equal(r[rank]["w"], (w.astype(np.float64) / mean).astype(np.float32))
    w_all = np.concatenate([r[0]["w"], r[1]["w"]]).astype(np.float64)
    assert abs(w_all.mean() - 1.0) < 1e-6
    assert not np.array_equal(r[0]["idx"], r[1]["idx"])
    np.testing.assert_array_equal(r[0]["params_after"], r[1]["params_after"])


def test_resample_leaves_parameters_and_other_plans_alone(monkeypatch):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    P = _ev_solver(_case(), monkeypatch)
    E = P.engine
    before = [t.clone() for t in (E.net.params, E.net.m, E.net.v, E.net_e.params, E.plan_b.x, E.plan_b.y)]
    plan_b, n_global = E.plan_b, E.n_f_global
    P.resample_collocation(seed=1)
    after = (E.net.params, E.net.m, E.net.v, E.net_e.params, E.plan_b.x, E.plan_b.y)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert E.plan_b is plan_b and E.n_f_global == n_global
    np.testing.assert_array_equal(E.plan_e.x.numpy(), E.plan_f.x.numpy())
    # a NaN in the pool raises before the live set is touched
    case = _case()
    case["xp"][17, 0] = np.nan
    x0 = E.plan_f.x.clone()
    P.set_resample_pool(X=(case["xp"], case["yp"]), weights=case["wp"])
    calls = E._resample_calls
    assert calls == 1                                  # a new pool keeps counting the draws
    for k in (1.0, 0.0):                               # k = 0 too: a NaN residual still shows in S
        with pytest.raises(FloatingPointError, match="unchanged"):
            P.resample_collocation(k=k, seed=2)
    assert torch.equal(E.plan_f.x, x0)
    # weights exactly when the live set has them
    with pytest.raises(ValueError, match="weights"):
        P.set_resample_pool(X=(case["xp"], case["yp"]))


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_solver_schedule_equals_manual_resample_and_step(monkeypatch, flavour):
    """set_resampling(every=R): train(n) resamples before steps R, 2R, ... - the same as a hand-written loop."""
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)

    def build():
        case = _case()        # fresh arrays: the CPU stand-in plans keep zero-copy views of float32 inputs
        install_fakes(monkeypatch)
        if flavour == "ev":
            P = _ev_solver(case, monkeypatch)
        else:
            from nsfnet_amd import pinn_solver as ps
            torch.manual_seed(3)
            P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=8, N_f=70, device="cpu")
            P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
            P.set_eq_training_data(X=(case["x"], case["y"]))
            P.set_resample_pool(X=(case["xp"], case["yp"]))
            P.log_every = P.save_every = 0
        return P

    A = build()
    A.set_resampling(every=2, k=2.0, c=0.5, seed=4)
    with contextlib.redirect_stdout(io.StringIO()):
        A.train(num_epoch=5, lr=1e-3)
    B = build()
    if flavour == "ev":
        B.freeze_evm_net(0)
    for i in range(5):
        if i in (2, 4):
            B.engine.resample(k=2.0, c=0.5, seed=4)
        if flavour == "ev":
            B._apply_freeze_schedule(i)           # (the ev loop re-creates Adam after step 0)
        B.engine.step(1e-3)
    np.testing.assert_array_equal(A.engine.net.params.numpy(), B.engine.net.params.numpy())
    np.testing.assert_array_equal(A.x_f.numpy().reshape(-1), B.engine.plan_f.x.numpy())
    assert A.engine._resample_calls == 2


# ---------------------------------------------------------------- ev drop-in configuration
def test_ev_config_has_resampling_off_by_default(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ev_dropin_config",
                                                  os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    config = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = config            # (dataclasses look their module up while the file executes)
    spec.loader.exec_module(config)
    mgr = config.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml"))
    rs = mgr.config.training.resampling
    assert rs.enabled is False and rs.every == 5000 and rs.pool_points == 1000000 and rs.k == 1.0 and rs.c == 1.0
    p = tmp_path / "rs.yaml"
    p.write_text("training:\n  resampling: {enabled: true, every: 200, pool_points: 50000, k: 2, c: 0.5, seed: 3}\n")
    rs = config.ConfigManager.from_file(str(p)).config.training.resampling
    assert (rs.enabled, rs.every, rs.pool_points, rs.k, rs.c, rs.seed) == (True, 200, 50000, 2.0, 0.5, 3)
    p.write_text("training:\n  resampling: {enabled: true, every: 0}\n")
    with pytest.raises(ValueError, match="resampling"):
        config.ConfigManager.from_file(str(p))
