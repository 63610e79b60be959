"""CPU tests of the stochastic mini-batching of the collocation term: the integer model of the
draw (Philox4x32-10 known answers, strata, coverage), the engine's host logic on the oracle-backed fakes (a batch step
is the oracle's step on store[idx] with normalisation B, the lagged viscosity's gather -> step -> scatter, the store
stays what L-BFGS and resampling see, the refusals), two gloo ranks, the ev drop-in's YAML block and the C ABI.  The
kernels are checked against the model in test_minibatch_gpu.py."""
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
from oracle import fwdmode_ref as fr  # noqa: E402

SHAPES = [(1000, 384), (1000, 100), (360000, 36000), (7, 7), (5, 1)]


# ------------------------------------------------------------------ the integer model
def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox4x32_10_known_answers():
    assert _hex(bm.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(bm.philox4x32_10((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(bm.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) \
        == "d16cfe09 94fdcceb 5001e420 24126ea1"


@pytest.mark.parametrize("n,b", SHAPES)
def test_model_draw_properties(n, b):
    lo, hi = bm.strata(n, b)
    assert lo[0] == 0 and hi[-1] == n and (hi > lo).all() and (lo[1:] == hi[:-1]).all()
    for t, seed, rank in ((0, 0, 0), (1, 0, 0), (12345678901, 7, 3)):
        idx = bm.draw(n, b, t, seed, rank)
        assert idx.dtype == np.int64 and idx.shape == (b,)
        assert (idx >= lo).all() and (idx < hi).all()
        assert (np.diff(idx) > 0).all()
        if b == n:
            assert (idx == np.arange(n)).all()
    if b < n and n // b >= 2 and b > 1:      # (5, 1): a single slot of 5 values may repeat
        base = bm.draw(n, b, 0, 0, 0)
        assert (bm.draw(n, b, 1, 0, 0) != base).any()
        assert (bm.draw(n, b, 0, 1, 0) != base).any()
        assert (bm.draw(n, b, 0, 0, 1) != base).any()
        assert (bm.draw(n, b, 1 << 32, 0, 0) != base).any()      # the high word of t is in the counter


def test_model_single_slot_varies_with_t_seed_and_rank():
    assert len({int(bm.draw(5, 1, t)[0]) for t in range(64)}) == 5
    assert len({int(bm.draw(5, 1, 0, seed=s)[0]) for s in range(64)}) == 5
    assert len({int(bm.draw(5, 1, 0, rank=r)[0]) for r in range(64)}) == 5


def test_model_coverage():
    seen = set()
    for t in range(200):
        seen |= set(bm.draw(1000, 100, t, seed=1).tolist())
    assert seen == set(range(1000))


def test_model_refuses_bad_sizes():
    for n, b in ((5, 0), (5, 6)):
        with pytest.raises(ValueError):
            bm.draw(n, b, 0)


# ------------------------------------------------------------------ the engine on the fakes
L, H, RE = 2, 10, 400.0


def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    w = (0.5 + rng.rand(N)).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, w=w, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", weights=True, sel=None, **kw):
    """Engine on the fakes; sel: only these collocation points (the reference engine of a batch)."""
    import batch_fakes
    batch_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=2, hidden_e=6, alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev, **kw)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    sel = slice(None) if sel is None else sel
    e.set_collocation(case["x"][sel], case["y"][sel], weights=case["w"][sel] if weights else None)
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    return e


def _terms(e):
    return {k: float(v) for k, v in e.loss_terms().items()}


def _close(a, b, rtol=2e-6):
    for k in a:
        assert abs(a[k] - b[k]) <= rtol * abs(a[k]) + 1e-12, (k, a[k], b[k])


def test_plain_batch_step_is_the_oracle_on_the_drawn_points(monkeypatch):
    case = _case()
    N, B, Nb = 70, 16, 33
    e = _engine(monkeypatch, case, weights=False)
    e.set_batching(B, seed=3)
    assert e.batch_info() == dict(batch_points=B, store_points=N, seed=3, draws=0)
    for t in range(2):
        e.loss_and_grad()
        idx = bm.draw(N, B, t, seed=3)
        np.testing.assert_array_equal(e.batch_indices().numpy(), idx)
        assert e.batch_info()["draws"] == t + 1
        pairs = fr.unflatten(e.net.params.numpy().astype(np.float64), 2, 3, L, H)
        xs, ys = case["x"][idx].astype(np.float64), case["y"][idx].astype(np.float64)
        r = fr.pde_loss_and_grad(pairs, xs, ys, RE, coef_eq=[2.0 / B] * 3 + [0.0])
        b = fr.bc_loss_and_grad(pairs, case["xb"], case["yb"], case["ub"], case["vb"], alpha_b=10.0, n_total=Nb)
        terms = _terms(e)
        np.testing.assert_allclose(terms["loss_e"], sum(r["sums"][:3]) / B, rtol=2e-6)
        np.testing.assert_allclose(terms["loss"], sum(r["sums"][:3]) / B + 10.0 * sum(b["sums"]) / Nb, rtol=2e-6)
        np.testing.assert_allclose(e.grads.numpy(), r["grad"] + b["grad"], rtol=2e-6, atol=2e-6 * np.abs(r["grad"]).max())
        f, _ = e.eval_plans()
        assert f.n == B and e.evaluated_batch
        e.adam_step(1e-3)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_batch_step_equals_a_plain_step_on_store_idx(monkeypatch, flavour):
    """Both flavours, with weights: loss terms and gradients of a batch step equal those of an engine whose collocation
    set is store[idx_model] (normalisation B), at the tolerance test_chunked_passes.py uses for the same fakes."""
    case = _case()
    N, B = 70, 20
    e = _engine(monkeypatch, case, flavour)
    e.e_trainable = flavour == "ev"
    store_vtm = None if flavour != "ev" else e.plan_f.vis_t_minus.numpy().copy()
    e.set_batching(B, seed=1)
    e.loss_and_grad()
    idx = bm.draw(N, B, 0, seed=1)
    np.testing.assert_array_equal(e.batch_indices().numpy(), idx)
    ref = _engine(monkeypatch, case, flavour, sel=idx)
    ref.e_trainable = e.e_trainable
    assert ref.n_f_global == B
    if flavour == "ev":
        np.testing.assert_array_equal(ref.plan_f.vis_t_minus.numpy(), store_vtm[idx])      # init_vis_t is pointwise
    ref.loss_and_grad()
    _close(_terms(ref), _terms(e))
    np.testing.assert_allclose(e.grads.numpy(), ref.grads.numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(e.grads_e.numpy(), ref.grads_e.numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_array_equal(e._batch.f.w.numpy(), case["w"][idx])      # gathered, not renormalised
    if flavour == "ev":
        got = e.plan_f.vis_t_minus.numpy()
        rest = np.setdiff1d(np.arange(N), idx)
        np.testing.assert_array_equal(got[rest], store_vtm[rest])
        np.testing.assert_allclose(got[idx], ref.plan_f.vis_t_minus.numpy(), rtol=1e-6)


def test_ev_three_steps_replay_gather_step_scatter(monkeypatch):
    case = _case()
    N, B, seed, alpha = 70, 20, 9, 0.05
    e = _engine(monkeypatch, case, "ev")
    e.set_batching(B, seed=seed)
    store = e.plan_f.vis_t_minus.numpy().copy()
    from fakes import FakeValuePlan
    for t in range(3):
        # the replay: gather -> step (the forward leaves alpha_evm |e| at the batch points) -> scatter
        idx = bm.draw(N, B, t, seed)
        batch = store[idx]
        pe = FakeValuePlan(e.net_e, case["x"][idx], case["y"][idx])
        pe.forward()
        vis_t_used = np.minimum(np.float32(e.vis_t0), batch)
        batch = (alpha * pe.pred[0].abs()).numpy()
        store[idx] = batch
        e.step(1e-3)
        np.testing.assert_array_equal(e.batch_indices().numpy(), idx)
        np.testing.assert_allclose(e.eval_plans()[0].vis_t.numpy(), vis_t_used, rtol=1e-6)
        np.testing.assert_allclose(e.plan_f.vis_t_minus.numpy(), store, rtol=1e-6)
        assert e.batch_info()["draws"] == t + 1
    assert e.plan_f.n == N and e.plan_e.n == N and e._batch.e.n == B


def test_counter_advances_once_per_evaluation_and_restarts_only_on_set_batching(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    e.set_batching(10, seed=2)
    e.loss_and_grad(); e.loss_and_grad(); e.adam_step(1e-3); e.step(1e-3)
    assert e.batch_info()["draws"] == 3
    np.testing.assert_array_equal(e.batch_indices().numpy(), bm.draw(70, 10, 2, seed=2))
    e.set_collocation(case["x"][:50], case["y"][:50], weights=case["w"][:50])      # a new store: the counter carries on
    assert e.batch_info() == dict(batch_points=10, store_points=50, seed=2, draws=3)
    e.loss_and_grad()
    np.testing.assert_array_equal(e.batch_indices().numpy(), bm.draw(50, 10, 3, seed=2))
    e.set_batching(10, seed=2)
    assert e.batch_info()["draws"] == 0


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_set_batching_zero_restores_full_batch_results(monkeypatch, flavour):
    case = _case()
    a = _engine(monkeypatch, case, flavour)
    b = _engine(monkeypatch, case, flavour)
    b.set_batching(12, seed=1)
    b.set_batching(0)
    assert b.batch_info() is None and b.batch_indices() is None
    for _ in range(2):
        a.step(1e-3); b.step(1e-3)
    assert _terms(a) == _terms(b)
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    np.testing.assert_array_equal(a.grads.numpy(), b.grads.numpy())
    if flavour == "ev":
        np.testing.assert_array_equal(a.plan_f.vis_t_minus.numpy(), b.plan_f.vis_t_minus.numpy())


def test_batch_of_all_points_is_the_full_step(monkeypatch):
    case = _case()
    a = _engine(monkeypatch, case, "ev")
    b = _engine(monkeypatch, case, "ev")
    b.set_batching(70, seed=4)
    for _ in range(3):
        a.step(1e-3); b.step(1e-3)
    np.testing.assert_array_equal(b.batch_indices().numpy(), np.arange(70))
    assert _terms(a) == _terms(b)
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    np.testing.assert_array_equal(a.plan_f.vis_t_minus.numpy(), b.plan_f.vis_t_minus.numpy())


def test_loss_balancing_works_on_the_batch_gradients(monkeypatch):
    case = _case()
    N, B = 70, 20
    e = _engine(monkeypatch, case)
    e.set_loss_balancing(2, 0.5)
    e.set_batching(B, seed=1)
    e.loss_and_grad()
    idx = bm.draw(N, B, 0, seed=1)
    ref = _engine(monkeypatch, case, sel=idx)
    ref.set_loss_balancing(2, 0.5)
    ref.loss_and_grad()
    assert e.balance_info()["updates"] == 1
    np.testing.assert_allclose(float(e.loss_weights()[0]), float(ref.loss_weights()[0]), rtol=2e-5)
    np.testing.assert_allclose(e.grads.numpy(), ref.grads.numpy(), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_lbfgs_step_sees_the_whole_store(monkeypatch, flavour):
    case = _case()
    a = _engine(monkeypatch, case, flavour)
    b = _engine(monkeypatch, case, flavour)
    b.set_batching(12, seed=1)
    la = a.lbfgs_step(max_iter=3, line_search_fn="strong_wolfe")
    lb = b.lbfgs_step(max_iter=3, line_search_fn="strong_wolfe")
    assert la == lb
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    assert b.batch_info()["draws"] == 0 and not b.evaluated_batch
    assert b.eval_plans()[0] is b.plan_f and _terms(a) == _terms(b)       # normalised by N again
    b.loss_and_grad(full_batch=True)
    assert b.batch_info()["draws"] == 0 and b.eval_plans()[0].n == 70
    b.step(1e-3)
    assert b.batch_info()["draws"] == 1 and b.evaluated_batch and b.eval_plans()[0].n == 12


def test_resample_rewrites_the_store_and_the_next_draw_sees_it(monkeypatch):
    case = _case()
    N, B = 70, 14
    e = _engine(monkeypatch, case, weights=False)
    e.set_batching(B, seed=6)
    e.step(1e-3)
    rng = np.random.RandomState(11)
    xp, yp = rng.rand(200).astype(np.float32), rng.rand(200).astype(np.float32)
    chosen = np.sort(rng.choice(200, N, replace=False))
    from nsfnet_amd import engine as eng

    def fake_select(pool, w4, k, c, u, m, scratch):
        assert m == N                                     # resample draws N points: the store, not the batch
        return torch.as_tensor(chosen), 1.0

    def fake_gather(idx, lo, hi, n_pool, src, dst, scratch, w_sum=None):
        for k in ("x", "y"):
            dst[k].copy_(src[k][idx[lo:hi]])

    monkeypatch.setattr(eng, "resample_select", fake_select)
    monkeypatch.setattr(eng, "resample_gather", fake_gather)
    monkeypatch.setattr(eng, "resample_scratch", lambda n, dev: torch.zeros(8, dtype=torch.uint8))
    e.set_resample_pool(xp, yp)
    e.resample(seed=1)
    x, y, _ = e.collocation_points()
    assert x.numel() == N
    np.testing.assert_array_equal(x.numpy(), xp[chosen])
    assert e.batch_info()["draws"] == 1                   # the counter is not restarted
    e.loss_and_grad()
    idx = bm.draw(N, B, 1, seed=6)
    f, _ = e.eval_plans()
    np.testing.assert_array_equal(f.x.numpy(), xp[chosen][idx])
    np.testing.assert_array_equal(f.y.numpy(), yp[chosen][idx])


def test_refusals_raise_value_error_and_leave_the_stream_alone(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, weights=False)
    switched = []
    monkeypatch.setattr(torch.cuda, "set_stream", lambda s: switched.append(s))
    with pytest.raises(ValueError):
        e.set_batching(71)                                # B > N
    with pytest.raises(ValueError):
        e.set_batching(-1)
    assert e.batch_info() is None
    c = _engine(monkeypatch, case, weights=False)
    c.set_collocation(case["x"], case["y"], chunk_points=32)
    from nsfnet_amd import engine as eng
    assert isinstance(c.plan_f, eng.ChunkedResidual)
    with pytest.raises(ValueError):
        c.set_batching(16)                                # a chunked store
    assert c.batch_info() is None
    e.set_batching(16)
    plan = e.plan_f
    with pytest.raises(ValueError):
        e.set_collocation(case["x"], case["y"], chunk_points=32)      # chunking under batching
    with pytest.raises(ValueError):
        e.set_collocation(case["x"][:8], case["y"][:8])               # the new store is smaller than B
    assert e.plan_f is plan
    with pytest.raises(ValueError):
        e.loss_and_grad("L2")                             # loss mode L2 with batching
    assert e.batch_info()["draws"] == 0 and switched == []
    e.set_batching(0)
    e.loss_and_grad("L2")                                 # ... and without


def test_graph_key_and_setters_clear_captured_steps(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, weights=False)
    e._graphs["stale"] = object()
    e.set_batching(8)
    assert not e._graphs
    e._graphs["stale"] = object()
    e.set_batching(0)
    assert not e._graphs


# ------------------------------------------------------------------ the solvers
def _ev_solver(monkeypatch, n=60):
    import batch_fakes
    batch_fakes.install(monkeypatch)
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


def test_ev_solver_trains_on_batches_and_marks_the_log(monkeypatch):
    P = _ev_solver(monkeypatch)
    P.set_batching(batch_points=15, seed=2)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=4, lr=1e-3, batchsize=7)        # batchsize stays accepted and ignored
    assert P.engine.batch_info()["draws"] == 4
    assert P.eq1_pred.shape == (15, 1) and P.evm.shape == (15, 1) and P.vis_t.shape == (15, 1)
    assert P.x_f.shape == (60, 1) and P.vis_t_minus.shape == (60, 1)
    assert "last batch: 15 of 60" in out.getvalue()
    P.set_batching(0)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=2, lr=1e-3)
    assert P.eq1_pred.shape == (60, 1) and "last batch" not in out.getvalue()


def test_plain_solver_set_batching_and_lbfgs_stage_ignores_it(monkeypatch):
    import batch_fakes
    batch_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    case = _case()
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=10, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.save = lambda *a, **k: None
    P.set_batching(batch_points=10, seed=1)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        P.train(num_epoch=3, lr=1e-3)
    assert P.engine.batch_info()["draws"] == 3 and P.eq1_pred.shape == (10, 1)
    assert "last batch of 10 points" in out.getvalue()
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=2, line_search_fn="strong_wolfe")
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=2, lr=1.0, optimizer=opt)
    assert P.engine.batch_info()["draws"] == 3 and P.eq1_pred.shape == (70, 1)


# ------------------------------------------------------------------ two gloo ranks
def _run_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank,
                            world_size=world)
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        import batch_fakes
        batch_fakes.install(None)
        from nsfnet_amd import engine as eng
        case = _case()
        lo, hi = (0, 35) if rank == 0 else (35, 70)
        e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, process_group=dist.group.WORLD, world_size=world)
        rng = np.random.RandomState(5)
        e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
        e.set_collocation(case["x"][lo:hi], case["y"][lo:hi], weights=case["w"][lo:hi], n_global=70)
        blo, bhi = (0, 16) if rank == 0 else (16, 33)
        e.set_boundary(*(case[k][blo:bhi] for k in ("xb", "yb", "ub", "vb")), n_global=33)
        e.set_batching(10, seed=5)
        e.loss_and_grad()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), idx=e.batch_indices().numpy(), grads=e.grads.numpy(),
                 loss_e=float(e.loss_terms()["loss_e"]), loss=float(e.loss_terms()["loss"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_draw_from_their_shards_and_reduce_over_2B(tmp_path, monkeypatch):
    world, B = 2, 10
    mp.spawn(_run_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    np.testing.assert_array_equal(r0["idx"], bm.draw(35, B, 0, seed=5, rank=0))
    np.testing.assert_array_equal(r1["idx"], bm.draw(35, B, 0, seed=5, rank=1))
    assert (r0["idx"] != r1["idx"]).any()
    np.testing.assert_array_equal(r0["grads"], r1["grads"])
    # one process on the union of the two batches: normalisation 2 B
    case = _case()
    union = np.concatenate([r0["idx"], 35 + r1["idx"]])
    ref = _engine(monkeypatch, case, sel=union)
    assert ref.n_f_global == 2 * B
    ref.loss_and_grad()
    np.testing.assert_allclose(r0["grads"], ref.grads.numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(float(r0["loss_e"]), float(ref.loss_terms()["loss_e"]), rtol=2e-6)
    np.testing.assert_allclose(float(r0["loss"]), float(ref.loss_terms()["loss"]), rtol=2e-6)


# ------------------------------------------------------------------ YAML, drop-in, C ABI
def _config_module():
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_batching", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_ev_config_parses_validates_and_prints_batching(tmp_path, capsys):
    cfg = _config_module()
    mgr = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                   "production.yaml"))
    bt = mgr.config.training.batching
    assert bt.enabled is False and bt.batch_points >= 1 and bt.seed == 0
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  batching: {enabled: true, batch_points: 12000, seed: 3}\n")
    mgr = cfg.ConfigManager.from_file(str(p))
    bt = mgr.config.training.batching
    assert (bt.enabled, bt.batch_points, bt.seed) == (True, 12000, 3)
    mgr.print_config()
    assert "batch_points=12000" in capsys.readouterr().out
    for bad in ("{enabled: true, batch_points: 0}", "{enabled: true, batch_points: -5}",
                "{enabled: true, batch_points: 10, seed: -1}"):
        p.write_text("training:\n  batching: %s\n" % bad)
        with pytest.raises(ValueError):
            cfg.ConfigManager.from_file(str(p))


def test_dropin_train_script_calls_set_batching():
    src = open(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "train.py")).read()
    assert re.search(r"PINN\.set_batching\(batch_points=\w+\.batch_points, seed=\w+\.seed\)", src)
    assert src.index("PINN.set_eq_training_data") < src.index("PINN.set_batching")


def test_header_declares_and_lib_binds_the_two_calls():
    hdr = open(os.path.join(ROOT, "include", "nsfnet_pinn.h")).read()
    from nsfnet_amd import _lib
    for name in ("pinn_batch_draw", "pinn_batch_scatter"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pinn_batch_draw"][1]) == 15
    assert len(_lib.SIGNATURES["pinn_batch_scatter"][1]) == 6
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.pinn_abi_version() == 3
        assert lib.pinn_batch_draw and lib.pinn_batch_scatter
        # argument checks happen on the host, before any launch
        assert lib.pinn_batch_draw(10, 11, 0, 0, None, None, None, None, None, None, None, None, None, None, None) != 0
        assert lib.pinn_batch_scatter(None, 1, 1, None, None, None) != 0


def test_build_compiles_batch_hip():
    from nsfnet_amd import build
    assert "batch.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "batch.hip")).read()
    assert "__umulhi" in src and "asm" not in src
