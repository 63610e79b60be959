"""CPU tests of the residual-based attention weights on the collocation points: the fp64 model
(bounds, skipped updates), the engine's host logic on the oracle-backed fakes (the update follows the published field
planes with one evaluation of lag, the feature changes nothing but w, batching, frozen evaluations, resampling, the
refusals, the graph key), two gloo ranks, the solvers, the ev drop-in's YAML block and the C ABI.  The kernels are
checked against the model in test_rba_gpu.py."""
import contextlib
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

import batch_model as bm  # noqa: E402
import rba_model as rm  # noqa: E402


# ------------------------------------------------------------------ the model
def test_model_definition_on_a_hand_example():
    eq = np.array([[3.0, 0.0], [4.0, 0.0], [0.0, 1.0], [0.0, 10.0]], dtype=np.float32)
    np.testing.assert_array_equal(rm.norms(eq, 0.0), [5.0, 1.0])
    r = rm.norms(eq, 0.1)
    assert r[0] == 5.0 and r[1] == np.sqrt(1.0 + 0.1 * 100.0)
    rmax, sums = rm.stats(eq, 0.1)
    assert rmax == 5.0 and sums == [9.0, 16.0, 1.0, 100.0]
    assert rm.stats(eq, 0.0)[1][3] == 0.0
    lam, w, rec = rm.apply(eq, 0.0, 0.5, 0.25, np.ones(2, np.float32), s=np.array([2.0, 3.0], np.float32))
    np.testing.assert_array_equal(lam, np.float32([0.75, 0.55]))
    np.testing.assert_array_equal(w, (np.float64([2.0, 3.0]) * (lam.astype(np.float64) ** 2)).astype(np.float32))
    assert rec[rm.R_RMAX] == 5.0 and rec[rm.R_UPDATES] == 1 and rec[rm.R_SKIPPED] == 0 and rec[rm.R_COUNT] == 2
    assert rec[rm.R_MIN] == float(lam[1]) and rec[rm.R_MAX] == 0.75


@pytest.mark.parametrize("init,gamma,eta", [(1.0, 0.999, 0.01), (0.0, 0.9, 0.5), (20.0, 0.99, 0.01), (1.0, 0.5, 0.0)])
def test_model_lam_stays_within_its_bound(init, gamma, eta):
    rng = np.random.RandomState(3)
    n = 64
    lam, w = rm.fill(n, init)
    hi = rm.bound(init, gamma, eta)
    for k in range(3000):
        eq = (rng.randn(4, n) * 10.0 ** rng.uniform(-6, 2)).astype(np.float32)
        eq[:, 0] = 1.0e4              # one point is always the maximum: its lam climbs to the bound
        lam, w, _ = rm.apply(eq, 0.1, gamma, eta, lam)
        assert (lam >= 0.0).all() and (lam <= hi * (1 + 1e-6)).all(), k
    if eta > 0:
        g = gamma ** 3000         # the point with r = rmax every time: the closed form of the recursion
        assert abs(lam[0] - (g * init + eta / (1 - gamma) * (1 - g))) <= 1e-4 * hi
    np.testing.assert_array_equal(w, rm.weights(None, lam))


def test_model_skips_a_nan_or_all_zero_residual_and_counts_it():
    rng = np.random.RandomState(4)
    eq = rng.randn(4, 10).astype(np.float32)
    lam0, w0 = rm.fill(10, 1.0, s=np.arange(1, 11, dtype=np.float32))
    bad = eq.copy(); bad[1, 7] = np.nan
    inf = eq.copy(); inf[0, 2] = np.inf
    rec = None
    for k, planes in enumerate((bad, np.zeros_like(eq), inf)):
        lam, w, rec = rm.apply(planes, 0.1, 0.9, 0.1, lam0, s=np.arange(1, 11, dtype=np.float32), record=rec)
        np.testing.assert_array_equal(lam, lam0)
        np.testing.assert_array_equal(w, w0)
        assert rec[rm.R_SKIPPED] == k + 1 and rec[rm.R_UPDATES] == 0
    assert np.isnan(rm.stats(bad, 0.1)[0]) and rm.stats(np.zeros_like(eq), 0.1)[0] == 0.0 and np.isinf(rec[rm.R_RMAX])
    bad4 = eq.copy(); bad4[3, 0] = np.nan           # plain NSFnet (w4 = 0) does not read eq4
    assert rm.apply(bad4, 0.0, 0.9, 0.1, lam0)[2][rm.R_UPDATES] == 1


def test_model_idx_scatter_and_out_of_range_entries():
    rng = np.random.RandomState(5)
    eq = rng.randn(4, 4).astype(np.float32)
    lam0, _ = rm.fill(9, 2.0)
    idx = np.array([7, -1, 2, 9])
    lam, w, rec = rm.apply(eq, 0.1, 0.9, 0.1, lam0, idx=idx)
    changed = np.flatnonzero(lam != lam0)
    np.testing.assert_array_equal(changed, [2, 7])
    assert rec[rm.R_COUNT] == 2
    r = rm.norms(eq, 0.1)
    assert lam[7] == np.float32(0.9 * 2.0 + 0.1 * r[0] / r.max())       # rmax is over all four rows of the call


# ------------------------------------------------------------------ the engine on the fakes
L, H, RE = 2, 10, 400.0


def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    w = (0.5 + rng.rand(N)).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, w=w, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", weights=True, sel=None, w=None, **kw):
    import rba_fakes
    rba_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=2, hidden_e=6, alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev, **kw)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    sel = slice(None) if sel is None else sel
    if w is None:
        w = case["w"][sel] if weights else None
    e.set_collocation(case["x"][sel], case["y"][sel], weights=w)
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    return e


def _eq(plan):
    from nsfnet_amd import engine as eng
    return plan.fields[eng.FLD["eq1"]:eng.FLD["eq4"] + 1, :plan.n].numpy().copy()


def _w4(e):
    return e.eq4_weight if e.net_e is not None else 0.0


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_lam_follows_the_published_planes_and_only_w_changes(monkeypatch, flavour, weights):
    """Over six steps: after each step lam is the model applied to the field planes that step published; the gradient
    and the loss sums of step k are, bit for bit, those of a fresh engine that was given s lam_{k-1}^2 as plain
    static weights at the same parameters (and the same lagged viscosity)."""
    case = _case()
    eta, gamma, init = 0.3, 0.9, 1.0
    e = _engine(monkeypatch, case, flavour, weights)
    s = case["w"] if weights else None
    e.set_residual_attention(eta, gamma, init)
    lam, w = rm.fill(70, init, s)
    np.testing.assert_array_equal(e.attention().numpy(), lam)
    np.testing.assert_array_equal(e.plan_f.w.numpy(), w)
    rec = np.zeros(rm.RECORD)
    for k in range(6):
        ref = _engine(monkeypatch, case, flavour, w=w.copy())
        ref.net.set_flat(e.net.params.clone())
        if flavour == "ev":
            ref.net_e.set_flat(e.net_e.params.clone())
            ref.plan_f.vis_t_minus = e.plan_f.vis_t_minus.clone()
        assert ref.attention() is None and ref.attention_info() is None
        ref.loss_and_grad()
        e.loss_and_grad()
        np.testing.assert_array_equal(e.grads.numpy(), ref.grads.numpy())
        np.testing.assert_array_equal(e.sums.numpy(), ref.sums.numpy())
        assert {k_: float(v) for k_, v in e.loss_terms().items()} == {k_: float(v) for k_, v in ref.loss_terms().items()}
        eq = _eq(e.eval_plans()[0])
        np.testing.assert_array_equal(eq, _eq(ref.plan_f))
        lam, w, rec = rm.apply(eq, _w4(e), gamma, eta, lam, s, record=rec)
        np.testing.assert_array_equal(e.attention().numpy(), lam)
        np.testing.assert_array_equal(e.plan_f.w.numpy(), w)
        np.testing.assert_array_equal(e.plan_f.w.numpy(), rm.weights(s, e.attention().numpy()))
        e.adam_step(1e-2)
    assert (lam != init).all()
    info = e.attention_info()
    assert info["updates"] == 6 and info["skipped"] == 0 and info["rmax"] == rec[rm.R_RMAX]
    assert info["lam_min"] == lam.min() and info["lam_max"] == lam.max()
    np.testing.assert_allclose(info["lam_mean"], lam.astype(np.float64).mean(), rtol=1e-14)
    q = eq.astype(np.float64)
    for c in range(4 if flavour == "ev" else 3):
        np.testing.assert_allclose(info["loss_eq%d" % (c + 1)], np.sum(q[c] ** 2) / 70, rtol=1e-13)
    if weights:      # loss_terms stays the weighted loss Adam minimises
        assert float(e.loss_terms()["loss_eq1"]) != pytest.approx(info["loss_eq1"], rel=1e-3)


def test_step_and_set_zero_restore_the_plain_engine(monkeypatch):
    case = _case()
    a = _engine(monkeypatch, case, "ev")
    b = _engine(monkeypatch, case, "ev")
    static = b.plan_f.w
    b.set_residual_attention(0.2, 0.9)
    assert b.plan_f.w is not static and b._rba.s is static
    b.set_residual_attention(0.0)
    assert b.plan_f.w is static and b.attention() is None and b.attention_info() is None
    for _ in range(2):
        a.step(1e-3); b.step(1e-3)
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    np.testing.assert_array_equal(a.grads.numpy(), b.grads.numpy())
    c = _engine(monkeypatch, case, weights=False)
    c.set_residual_attention(0.2)
    assert c.plan_f.w is not None
    c.set_residual_attention(0.0)
    assert c.plan_f.w is None


def test_a_call_and_set_collocation_restart_lam_at_init(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    e.set_residual_attention(0.3, 0.9, 1.0)
    e.step(1e-3)
    assert (e.attention().numpy() != 1.0).any() and e.attention_info()["updates"] == 1
    e.set_residual_attention(0.3, 0.9, 2.0)
    np.testing.assert_array_equal(e.attention().numpy(), np.full(70, 2.0, np.float32))
    np.testing.assert_array_equal(e.plan_f.w.numpy(), case["w"] * np.float32(4.0))
    assert e.attention_info()["updates"] == 0
    e.step(1e-3)
    e.set_collocation(case["x"][:50], case["y"][:50])                 # a new set without weights: s is gone
    assert e._rba.s is None and e.attention().numel() == 50
    np.testing.assert_array_equal(e.plan_f.w.numpy(), np.full(50, 4.0, np.float32))
    e.step(1e-3)
    assert e.attention_info()["updates"] == 1


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_batching_updates_only_the_drawn_points_with_the_batch_rmax(monkeypatch, flavour):
    case = _case()
    N, B, eta, gamma = 70, 20, 0.3, 0.9
    e = _engine(monkeypatch, case, flavour)
    e.set_batching(B, seed=1)
    e.set_residual_attention(eta, gamma)
    assert e._batch.f.w is not None
    lam, w = rm.fill(N, 1.0, case["w"])
    for t in range(3):
        vtm = None if flavour != "ev" else e.plan_f.vis_t_minus.numpy().copy()
        e.loss_and_grad()
        idx = e.batch_indices().numpy()
        np.testing.assert_array_equal(idx, bm.draw(N, B, t, seed=1))
        np.testing.assert_array_equal(e._batch.f.w.numpy(), w[idx])          # gathered before the update: the lag
        f = e.eval_plans()[0]
        assert f.n == B
        eq = _eq(f)
        new, w, _ = rm.apply(eq, _w4(e), gamma, eta, lam, case["w"], idx=idx)
        got = e.attention().numpy()
        np.testing.assert_array_equal(got, new)
        np.testing.assert_array_equal(np.flatnonzero(got != lam), idx)
        assert e.attention_info()["rmax"] == rm.stats(eq, _w4(e))[0]
        np.testing.assert_array_equal(e.plan_f.w.numpy(), w)
        if flavour == "ev":       # the scatter of the lagged viscosity still works
            now = e.plan_f.vis_t_minus.numpy()
            rest = np.setdiff1d(np.arange(N), idx)
            np.testing.assert_array_equal(now[rest], vtm[rest])
            np.testing.assert_array_equal(now[idx], f.vis_t_minus.numpy())
        lam = new
        e.adam_step(1e-2)
    # switching the feature off under batching: the batch plan loses its weight buffer with the store
    c = _engine(monkeypatch, case, flavour, weights=False)
    c.set_batching(B)
    c.set_residual_attention(eta)
    assert c._batch.f.w is not None
    c.set_residual_attention(0.0)
    assert c._batch.f.w is None and c.plan_f.w is None
    c.step(1e-3)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_lbfgs_and_full_batch_evaluations_leave_lam_untouched(monkeypatch, flavour):
    case = _case()
    e = _engine(monkeypatch, case, flavour)
    e.set_residual_attention(0.3, 0.9)
    e.step(1e-3)
    lam, w, n = e.attention().numpy().copy(), e.plan_f.w.numpy().copy(), e.attention_info()["updates"]
    e.lbfgs_step(max_iter=3, line_search_fn="strong_wolfe")
    e.loss_and_grad(full_batch=True)
    np.testing.assert_array_equal(e.attention().numpy(), lam)
    np.testing.assert_array_equal(e.plan_f.w.numpy(), w)
    assert e.attention_info()["updates"] == n and not e._rba_frozen
    # the L-BFGS objective used the current weights: the same steps as an engine given them as static weights
    ref = _engine(monkeypatch, case, flavour, w=w)
    ref.net.set_flat(e.net.params.clone())
    if flavour == "ev":
        ref.net_e.set_flat(e.net_e.params.clone())
    assert e.lbfgs_step(max_iter=2, line_search_fn="strong_wolfe", owner="a") \
        == ref.lbfgs_step(max_iter=2, line_search_fn="strong_wolfe", owner="a")
    np.testing.assert_array_equal(e.net.params.numpy(), ref.net.params.numpy())
    e.loss_and_grad()
    assert e.attention_info()["updates"] == n + 1


@pytest.mark.parametrize("weights", [False, True])
def test_resample_renormalises_s_and_resets_lam(monkeypatch, weights):
    case = _case()
    N = 70
    e = _engine(monkeypatch, case, weights=weights)
    e.set_residual_attention(0.3, 0.9, 1.5)
    e.step(1e-3)
    rng = np.random.RandomState(11)
    xp, yp = rng.rand(200).astype(np.float32), rng.rand(200).astype(np.float32)
    wp = (0.5 + rng.rand(200)).astype(np.float32)
    chosen = np.sort(rng.choice(200, N, replace=False))
    from nsfnet_amd import engine as eng

    def fake_gather(idx, lo, hi, n_pool, src, dst, scratch, w_sum=None):
        for k in ("x", "y", "w"):
            assert (src.get(k) is None) == (dst.get(k) is None), k
            if src.get(k) is not None:
                dst[k].copy_(src[k][idx[lo:hi]])
        if w_sum is not None:
            w_sum[0] = float(dst["w"].double().sum())

    monkeypatch.setattr(eng, "resample_select", lambda pool, w4, k, c, u, m, scratch: (torch.as_tensor(chosen), 1.0))
    monkeypatch.setattr(eng, "resample_gather", fake_gather)
    monkeypatch.setattr(eng, "resample_scratch", lambda n, dev: torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError):      # pool weights exactly when the set has STATIC weights
        e.set_resample_pool(xp, yp, weights=None if weights else wp)
    e.set_resample_pool(xp, yp, weights=wp if weights else None)
    w_buf, lam_buf = e.plan_f.w, e.attention()
    e.resample(seed=1)
    assert e.plan_f.w is w_buf and e.attention() is lam_buf       # in place
    np.testing.assert_array_equal(e.attention().numpy(), np.full(N, 1.5, np.float32))
    if weights:
        s = e._rba.s.numpy()
        np.testing.assert_allclose(s.astype(np.float64).mean(), 1.0, rtol=1e-6)
        np.testing.assert_allclose(s, wp[chosen] / wp[chosen].astype(np.float64).mean(), rtol=1e-6)
    else:
        assert e._rba.s is None
    np.testing.assert_array_equal(e.plan_f.w.numpy(), rm.weights(None if not weights else e._rba.s.numpy(),
                                                                e.attention().numpy()))
    np.testing.assert_array_equal(e.collocation_points()[0].numpy(), xp[chosen])


def test_refusals_come_before_any_stream_switch(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, weights=False)
    switched = []
    monkeypatch.setattr(torch.cuda, "set_stream", lambda s: switched.append(s))
    for bad in (dict(eta=-0.1), dict(eta=float("nan")), dict(eta=0.1, gamma=0.0), dict(eta=0.1, gamma=1.5),
                dict(eta=0.1, gamma=float("nan")), dict(eta=0.1, init=-1.0), dict(eta=0.1, init=float("inf"))):
        with pytest.raises(ValueError):
            e.set_residual_attention(**bad)
    assert e.attention() is None and e.plan_f.w is None
    c = _engine(monkeypatch, case, weights=False)
    c.set_collocation(case["x"], case["y"], chunk_points=32)
    from nsfnet_amd import engine as eng
    assert isinstance(c.plan_f, eng.ChunkedResidual)
    with pytest.raises(ValueError):
        c.set_residual_attention(0.1)                     # a chunked store
    assert c.attention() is None
    import rba_fakes
    rba_fakes.install(monkeypatch)
    fresh = eng.PinnEngine("cpu", L, H, RE)
    with pytest.raises(RuntimeError):
        fresh.set_residual_attention(0.1)                 # before set_collocation
    fresh.set_residual_attention(0.0)                     # switching off needs nothing
    e.set_residual_attention(0.1)
    plan = e.plan_f
    with pytest.raises(ValueError):
        e.set_collocation(case["x"], case["y"], chunk_points=32)      # chunking under attention
    assert e.plan_f is plan
    with pytest.raises(ValueError):
        e.loss_and_grad("L2")                             # loss mode L2 with attention
    assert e.attention_info()["updates"] == 0 and switched == []
    e.set_residual_attention(0.0)
    e.loss_and_grad("L2")                                 # ... and without


def test_graph_key_and_setters_clear_captured_steps(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, weights=False)
    e._graphs["stale"] = object()
    e.set_residual_attention(0.1)
    assert not e._graphs
    e._graphs["stale"] = object()
    e.set_residual_attention(0.0)
    assert not e._graphs
    # on / off, gamma and eta are launch scalars of a captured step: they are part of its key
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
    e._graphs = Probe()
    for args in ((0.0,), (0.1, 0.9), (0.2, 0.9), (0.2, 0.99), (0.2, 0.99, 3.0)):
        e.set_residual_attention(*args)
        with pytest.raises(Stop):
            e.step(1e-3)
    assert len(set(keys[:4])) == 4 and keys[3] == keys[4]       # init is device state, not a launch scalar


# ------------------------------------------------------------------ the solvers
def _ev_solver(monkeypatch, n=60):
    import rba_fakes
    rba_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    from oracle import autograd_ref as ar
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "NSFNET_CHUNK_POINTS"):
        monkeypatch.delenv(k, raising=False)
    rng = np.random.RandomState(7)
    x, y = rng.rand(n, 1), rng.rand(n, 1)
    w = (0.5 + rng.rand(n)).astype(np.float32)
    xb, yb, ub, vb = (a[::63][:33] for a in ar.cavity_boundary())
    torch.manual_seed(3)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=n,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(xb, yb, ub, vb))
    P.set_eq_training_data(X=(x, y), weights=w)
    P.log_interval = 2
    P.save = lambda *a, **k: None
    return P


def test_ev_solver_trains_with_attention_and_marks_the_log(monkeypatch):
    P = _ev_solver(monkeypatch)
    P.set_residual_attention(eta=0.2, gamma=0.9)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=4, lr=1e-3)
    info = P.engine.attention_info()
    assert info["updates"] == 4 and info["lam_max"] > 1.0
    assert "attention lam: min=" in out.getvalue() and "unweighted loss_e=" in out.getvalue()
    sd = P.net.state_dict() if hasattr(P.net, "state_dict") else {}
    assert not any("lam" in k or "attention" in k for k in sd)      # checkpoints stay in the reference's format
    P.set_residual_attention(0.0)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=2, lr=1e-3)
    assert "attention" not in out.getvalue() and P.engine.attention() is None


def test_plain_solver_set_residual_attention_and_lbfgs_stage_keeps_the_weights(monkeypatch):
    import rba_fakes
    rba_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    case = _case()
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=10, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.save = lambda *a, **k: None
    P.set_residual_attention(eta=0.2, gamma=0.9)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        P.train(num_epoch=3, lr=1e-3)
    assert P.engine.attention_info()["updates"] == 3
    assert "attention lam: min=" in out.getvalue()
    lam = P.engine.attention().numpy().copy()
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=2, line_search_fn="strong_wolfe")
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=2, lr=1.0, optimizer=opt)
    np.testing.assert_array_equal(P.engine.attention().numpy(), lam)
    assert P.engine.attention_info()["updates"] == 3


# ------------------------------------------------------------------ two gloo ranks
def _run_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank,
                            world_size=world)
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        import rba_fakes
        rba_fakes.install(None)
        from nsfnet_amd import engine as eng
        case = _case()
        lo, hi = (0, 35) if rank == 0 else (35, 70)
        e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, process_group=dist.group.WORLD, world_size=world)
        rng = np.random.RandomState(5)
        e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
        e.set_collocation(case["x"][lo:hi], case["y"][lo:hi], weights=case["w"][lo:hi], n_global=70)
        blo, bhi = (0, 16) if rank == 0 else (16, 33)
        e.set_boundary(*(case[k][blo:bhi] for k in ("xb", "yb", "ub", "vb")), n_global=33)
        e.set_residual_attention(0.3, 0.9)
        e.loss_and_grad()
        own = rm.stats(e.plan_f.fields[eng.FLD["eq1"]:eng.FLD["eq4"] + 1, :e.plan_f.n].numpy(), 0.0)[0]
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), lam=e.attention().numpy(), w=e.plan_f.w.numpy(),
                 rmax=e.attention_info()["rmax"], own=own)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_divide_by_the_global_rmax(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_run_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    assert float(r0["rmax"]) == float(r1["rmax"]) == max(float(r0["own"]), float(r1["own"]))
    assert float(r0["own"]) != float(r1["own"])
    # one rank on the union of the points
    case = _case()
    ref = _engine(monkeypatch, case)
    ref.set_residual_attention(0.3, 0.9)
    ref.loss_and_grad()
    assert ref.attention_info()["rmax"] == float(r0["rmax"])
    np.testing.assert_array_equal(np.concatenate([r0["lam"], r1["lam"]]), ref.attention().numpy())
    np.testing.assert_array_equal(np.concatenate([r0["w"], r1["w"]]), ref.plan_f.w.numpy())


def test_nan_rmax_survives_the_integer_max():
    """The multi-rank reduction of rmax is an int64 MAX of the doubles' bytes: for non-negative values, +inf and the
    positive quiet NaN that order is the NaN-propagating order of the values."""
    vals = np.array([0.0, 1e-300, 1.0, 3.5, 1e300, np.inf, np.nan])
    bits = vals.view(np.int64)
    assert (np.diff(bits) > 0).all()


# ------------------------------------------------------------------ YAML, drop-in, C ABI
def _config_module():
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_rba", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_ev_config_parses_validates_and_prints_residual_attention(tmp_path, capsys):
    cfg = _config_module()
    mgr = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                   "production.yaml"))
    ra = mgr.config.training.residual_attention
    assert (ra.eta, ra.gamma, ra.init) == (0.0, 0.999, 1.0)           # off by default
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  N_f: 10\n")
    assert cfg.ConfigManager.from_file(str(p)).config.training.residual_attention.eta == 0.0
    p.write_text("training:\n  residual_attention: {eta: 0.01, gamma: 0.99, init: 2}\n")
    mgr = cfg.ConfigManager.from_file(str(p))
    ra = mgr.config.training.residual_attention
    assert (ra.eta, ra.gamma, ra.init) == (0.01, 0.99, 2.0)
    mgr.print_config()
    assert "eta=0.01 gamma=0.99" in capsys.readouterr().out
    for bad in ("{eta: -0.01}", "{eta: 0.01, gamma: 0.0}", "{eta: 0.01, gamma: 1.5}", "{eta: 0.01, init: -1}",
                "{eta: .nan}"):
        p.write_text("training:\n  residual_attention: %s\n" % bad)
        with pytest.raises(ValueError):
            cfg.ConfigManager.from_file(str(p))


def test_dropin_train_script_calls_set_residual_attention():
    src = open(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "train.py")).read()
    assert re.search(r"PINN\.set_residual_attention\(eta=\w+\.eta, gamma=\w+\.gamma, init=\w+\.init\)", src)
    assert src.index("PINN.set_eq_training_data") < src.index("PINN.set_residual_attention")


def test_header_declares_and_lib_binds_the_calls():
    hdr = open(os.path.join(ROOT, "include", "nsfnet_pinn.h")).read()
    from nsfnet_amd import _lib, build
    assert "rba.hip" in build.SOURCES
    for name, nargs in (("pinn_rba_scratch_bytes", 1), ("pinn_rba_stats", 6), ("pinn_rba_apply", 14),
                        ("pinn_rba_fill", 6)):
        assert re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert "#define PINN_RBA_RECORD %d" % rm.RECORD in hdr
    from nsfnet_amd import engine as eng
    assert eng.RBA_RECORD == rm.RECORD
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.pinn_abi_version() == 3
        assert lib.pinn_rba_scratch_bytes(0) == -1 and lib.pinn_rba_scratch_bytes(360000) > 0
        # argument checks happen on the host, before any launch
        assert lib.pinn_rba_stats(10, None, 12, 0.1, None, None) != 0
        assert b"pinn_rba_stats" in lib.pinn_last_error()
        assert lib.pinn_rba_stats(10, 16, 10, 0.1, 8, None) != 0 and b"multiple of 4" in lib.pinn_last_error()
        assert lib.pinn_rba_apply(10, 16, 12, 0.1, 0.0, 0.1, None, 10, None, 16, 32, 8, 8, None) != 0
        assert b"gamma" in lib.pinn_last_error()
        assert lib.pinn_rba_apply(10, 16, 12, 0.1, 0.9, -1.0, None, 10, None, 16, 32, 8, 8, None) != 0
        assert lib.pinn_rba_apply(10, 16, 12, 0.1, 0.9, 0.1, None, 9, None, 16, 32, 8, 8, None) != 0
        assert b"n_store" in lib.pinn_last_error()
        assert lib.pinn_rba_apply(10, 16, 12, 0.1, 0.9, 0.1, None, 10, None, 16, 36, 8, 8, None) != 0
        assert b"aligned" in lib.pinn_last_error()
        assert lib.pinn_rba_fill(10, -1.0, None, 16, 32, None) != 0 and lib.pinn_rba_fill(0, 1.0, None, 16, 32, None) != 0
