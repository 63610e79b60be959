"""GPU tests of the adaptive loss-weight balancing: the term-split assembly against the fp64
oracle's per-term gradients, the statistics / update / combine kernels against tests/balance_model.py, trajectories
against the fp64 model, chunked and graph-replayed steps, and the ev drop-in with the YAML block on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import balance_model as bm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402
from oracle import fwdmode_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bc(every=16):
    return tuple(a.reshape(-1)[::every].astype(np.float32) for a in ar.cavity_boundary())


def _rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _plain_engine(L, H, n, prec="fp32", alpha_b=10.0, seed=5, Re=400.0, chunk=None):
    from nsfnet_amd import engine as eng
    flat = ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().copy()
    E = eng.PinnEngine(DEV, L, H, Re, alpha_b=alpha_b, alpha_e=1.0, precision=prec)
    E.net.set_flat(torch.tensor(flat))
    rng = np.random.RandomState(seed)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    E.set_collocation(x, y, chunk_points=chunk)
    E.set_boundary(*_bc())
    return E, flat, x, y


def _oracle_terms(flat, L, H, x, y, Re=400.0):
    P = fr.unflatten(np.asarray(flat, np.float64), 2, 3, L, H)
    xb, yb, ub, vb = (a.astype(np.float64) for a in _bc())
    gr = fr.pde_loss_and_grad(P, x.astype(np.float64), y.astype(np.float64), Re, alpha_e=1.0)["grad"]
    gb = fr.bc_loss_and_grad(P, xb, yb, ub, vb, alpha_b=1.0)["grad"]
    return gr, gb


# ---------------------------------------------------------------- term-split assembly
@pytest.mark.parametrize("L,H,n", [(2, 16, 40000), (3, 64, 20000)])
def test_term_split_reduce_matches_oracle_terms(L, H, n):
    """fp32 mode at point counts where the sweeps' tile loops repeat (several tiles per workgroup)."""
    from nsfnet_amd import engine as eng
    E, flat, x, y = _plain_engine(L, H, n)
    E.set_loss_balancing(1, 0.1)
    E.loss_and_grad()
    gr_dev = torch.empty(E.P, device=DEV)
    gb_dev = torch.empty(E.P, device=DEV)
    parts = eng.balance_partials(E.P, DEV)
    eng.grad_reduce_terms(E.net, [[E.plan_f], [E.plan_b], []], [gr_dev, gb_dev, None], partials=parts)
    torch.cuda.synchronize()
    gr, gb = _oracle_terms(flat, L, H, x, y)
    assert _rel_max(gr_dev.cpu().numpy(), gr) < 2e-4
    assert _rel_max(gb_dev.cpu().numpy(), gb) < 2e-4
    assert torch.equal(gb_dev, E._bal.gb)
    # the partials of the assembly are those of the vectors it wrote
    ref = bm.block_partials([gr_dev.cpu().numpy(), gb_dev.cpu().numpy(), None], E.P)
    np.testing.assert_allclose(parts.cpu().numpy().reshape(-1, 6), ref, rtol=1e-12, atol=0)
    # the balance step's record: statistics of the oracle terms, lambda from the rule
    info = E.balance_info()
    mean_b = np.abs(gb).mean()
    assert abs(info["max_r"] - np.abs(gr).max()) <= 2e-4 * np.abs(gr).max()
    assert abs(info["mean_b"] - mean_b) <= 2e-4 * mean_b
    lhat = np.abs(gr).max() / mean_b
    assert abs(info["lambda_b"] - (0.9 * 10.0 + 0.1 * lhat)) <= 4e-4 * info["lambda_b"]
    g = E.grads.cpu().numpy().astype(np.float64)
    assert _rel_max(g, gr + np.float32(info["lambda_b"]) * gb) < 4e-4


def test_combined_gradient_equals_single_reduce_at_configured_weight():
    A, _, _, _ = _plain_engine(3, 24, 2000)
    B, _, _, _ = _plain_engine(3, 24, 2000)
    B.set_loss_balancing(10, 0.1)
    A.loss_and_grad()
    B._loss_and_grad(update=False)      # an evaluation that is not a balance step: lambda_b = alpha_b
    torch.cuda.synchronize()
    a, b = A.grads.cpu().numpy(), B.grads.cpu().numpy()
    assert float(B.loss_weights()[0]) == 10.0
    np.testing.assert_allclose(b, a, rtol=0, atol=4 * np.finfo(np.float32).eps * np.abs(a).max())
    ta, tb = A.loss_terms(), B.loss_terms()
    assert float(ta["loss"]) == pytest.approx(float(tb["loss"]), rel=1e-6)


# ---------------------------------------------------------------- statistics / update kernels vs the model
def _vectors(P, kind, rng):
    gr = (rng.randn(P) * 10.0 ** rng.uniform(-3, 1, P)).astype(np.float32)
    gb = (rng.randn(P) * 1e-2).astype(np.float32)
    gs = (rng.randn(P) * 1e-3).astype(np.float32)
    if kind == "zero_b":
        gb[:] = 0
    elif kind == "all_zero":
        gr[:] = 0; gb[:] = 0; gs[:] = 0
    elif kind == "nan_s":
        gs[P // 2] = np.nan
    return gr, gb, gs


@pytest.mark.parametrize("P", [1, 257, 330499, 1125203])
@pytest.mark.parametrize("kind", ["plain", "zero_b", "all_zero", "nan_s"])
def test_update_kernel_matches_model(P, kind):
    from nsfnet_amd import engine as eng
    rng = np.random.RandomState(P % 1000 + len(kind))
    vecs = _vectors(P, kind, rng)
    dv = [torch.tensor(v, device=DEV) for v in vecs]
    rec0 = bm.initial_record(10.0, 2.0)
    rec0[8] = 1                                              # a skip count carried from earlier steps

    def run():
        parts = eng.balance_partials(P, DEV)
        lam = torch.zeros(2, device=DEV)
        rec = torch.tensor(rec0, device=DEV)
        eng.balance_stats(dv, P, parts)
        eng.balance_update(parts, P, 3, 0.1, lam, rec)
        g = torch.empty(P, device=DEV)
        eng.balance_combine(g, dv[0], dv[1], dv[2], lam)
        torch.cuda.synchronize()
        return parts.cpu().numpy(), lam.cpu().numpy(), rec.cpu().numpy(), g.cpu().numpy()

    parts, lam, rec, g = run()
    parts2, lam2, rec2, g2 = run()
    for a, b in ((parts, parts2), (lam, lam2), (rec, rec2), (g, g2)):
        np.testing.assert_array_equal(a, b)                  # bit-reproducible
    ref_parts = bm.block_partials(vecs, P)
    np.testing.assert_allclose(parts.reshape(-1, 6), ref_parts, rtol=1e-12, atol=0)
    ref = bm.update(ref_parts, P, 3, 0.1, rec0)
    np.testing.assert_allclose(rec, ref, rtol=1e-12, atol=0)
    skips = {"plain": 0, "zero_b": 1, "all_zero": 2, "nan_s": 1}[kind]
    assert rec[8] == 1 + skips and rec[11] == 1
    if kind in ("zero_b", "all_zero"):
        assert rec[9] == 10.0
    if kind in ("nan_s", "all_zero"):
        assert rec[10] == 2.0
    assert lam[0] == np.float32(rec[9]) and lam[1] == np.float32(rec[10])
    ref_g = bm.combine(vecs[0], vecs[1], vecs[2], lam)
    fin = np.isfinite(ref_g)
    assert np.array_equal(np.isfinite(g), fin)
    if fin.any():
        np.testing.assert_allclose(g[fin], ref_g[fin], rtol=0, atol=1e-6 * np.abs(ref_g[fin]).max())


# ---------------------------------------------------------------- trajectories
def _ref_trajectory(flat, L, H, x, y, steps, every, beta, alpha_b, lr):
    p = np.asarray(flat, np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    rec, cad, lams = bm.initial_record(alpha_b, 0.0), bm.Cadence(every), []
    for n in range(steps):
        gr, gb = _oracle_terms(p, L, H, x, y)
        if cad.evaluate():
            rec = bm.update(bm.block_partials([gr, gb, None], p.size), p.size, 1, beta, rec)
        p, m, v = fr.adam_step(p, bm.combine(gr, gb, None, rec[9:11]), m, v, n + 1, lr)
        cad.adam()
        lams.append(rec[9])
    return p, np.array(lams)


def test_adam_trajectory_follows_the_model():
    L, H = 4, 24
    E, flat, x, y = _plain_engine(L, H, 2000)
    E.set_loss_balancing(10, 0.1)
    lams = []
    for _ in range(30):
        E.step(1e-3)
        lams.append(float(E.loss_weights()[0]))
    torch.cuda.synchronize()
    p_ref, lam_ref = _ref_trajectory(flat, L, H, x, y, 30, 10, 0.1, 10.0, 1e-3)
    assert E.balance_info()["updates"] == 3
    np.testing.assert_allclose(lams, lam_ref, rtol=1e-3)
    mine = E.net.params.cpu().numpy().astype(np.float64)
    assert np.linalg.norm((mine - flat) - (p_ref - flat)) / np.linalg.norm(p_ref - flat) < 2e-3


def test_bf16x3_hidden256_balance_step_matches_oracle_statistics():
    L, H = 6, 256
    E, flat, x, y = _plain_engine(L, H, 1024, prec="bf16x3")
    E.set_loss_balancing(5, 0.1)
    E.loss_and_grad()
    lam = E.balance_info()["lambda_b"]
    gr, gb = _oracle_terms(flat, L, H, x, y)
    want = 0.9 * 10.0 + 0.1 * np.abs(gr).max() / np.abs(gb).mean()
    assert abs(lam - want) <= 1e-4 * want


def test_ev_supervised_balance_step_matches_oracle_statistics():
    from nsfnet_amd import engine as eng
    L, H, Le, He, Re = 6, 80, 4, 40, 2000.0
    flat = ar.flat_params(ar.seeded_net(3, L, H, seed=11)).numpy().copy()
    flat_e = ar.flat_params(ar.seeded_net(1, Le, He, seed=12)).numpy().copy()
    E = eng.PinnEngine(DEV, L, H, Re, alpha_b=10.0, alpha_e=1.0, flavour="ev", n_hidden_e=Le, hidden_e=He,
                       alpha_evm=0.05, alpha_s=0.5, precision="fp32")
    E.net.set_flat(torch.tensor(flat))
    E.net_e.set_flat(torch.tensor(flat_e))
    rng = np.random.RandomState(3)
    n, ns = 1500, 40
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    w = (0.2 + rng.rand(n)).astype(np.float32)
    E.set_collocation(x, y, weights=w)
    xb, yb, ub, vb = _bc()
    E.set_boundary(xb, yb, ub, vb)
    xs, ys = rng.rand(ns).astype(np.float32), rng.rand(ns).astype(np.float32)
    us, vs, ps = np.sin(xs), np.cos(ys), (xs * ys).astype(np.float32)
    ps[:5] = np.nan
    E.set_supervised(xs, ys, us, vs, ps)
    E.set_loss_balancing(7, 0.25)
    E.loss_and_grad()
    info = E.balance_info()
    vt = E.plan_f.vis_t.cpu().numpy().astype(np.float64)
    ev = E.plan_e.pred[0].cpu().numpy().astype(np.float64)
    P = fr.unflatten(flat.astype(np.float64), 2, 3, L, H)
    gr = fr.pde_loss_and_grad(P, x.astype(np.float64), y.astype(np.float64), Re, vis_t=vt, e=ev,
                              w=w.astype(np.float64))["grad"]
    gb = fr.bc_loss_and_grad(P, *(a.astype(np.float64) for a in (xb, yb, ub, vb)), alpha_b=1.0)["grad"]
    out, saved = fr.forward1(P, xs.astype(np.float64), ys.astype(np.float64))
    ok = np.isfinite(ps)
    adj = np.zeros_like(out)
    adj[:, 0] = 2.0 * (out[:, 0] - us) / ns
    adj[:, 1] = 2.0 * (out[:, 1] - vs) / ns
    adj[:, 2] = np.where(ok, 2.0 * (out[:, 2] - np.where(ok, ps, 0.0)) / ok.sum(), 0.0)
    gs = fr.backward1(P, xs.astype(np.float64), ys.astype(np.float64), saved, adj)
    mr = np.abs(gr).max()
    for key, g, a0 in (("lambda_b", gb, 10.0), ("lambda_s", gs, 0.5)):
        want = 0.75 * a0 + 0.25 * mr / np.abs(g).mean()
        assert abs(info[key] - want) <= 1e-4 * want, key
    t = E.loss_terms()
    want = float(t["loss_e"]) + info["lambda_b"] * float(t["loss_b"]) + info["lambda_s"] * float(t["loss_s"])
    assert float(t["loss"]) == pytest.approx(want, rel=1e-5)


def test_chunked_equals_unchunked():
    A, _, _, _ = _plain_engine(3, 32, 5000)
    B, _, _, _ = _plain_engine(3, 32, 5000, chunk=2048)
    assert len(B.plan_f.chunks) == 3
    for E in (A, B):
        E.set_loss_balancing(2, 0.1)
        for _ in range(5):
            E.step(1e-3)
    torch.cuda.synchronize()
    assert _rel_max(B.loss_weights().cpu().numpy(), A.loss_weights().cpu().numpy()) < 2e-6
    assert _rel_max(B.net.params.cpu().numpy(), A.net.params.cpu().numpy()) < 2e-6


def test_graph_replay_is_bit_identical_to_eager(monkeypatch):
    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E, _, _, _ = _plain_engine(3, 24, 3000)
        E.set_loss_balancing(3, 0.2)
        for _ in range(10):                      # balance steps at 0, 3, 6, 9: the balance graph replays twice
            E.step(1e-3)
        torch.cuda.synchronize()
        if graph:
            assert len(E._graphs) == 2
        return E.net.params.cpu().numpy(), E._bal.rec.cpu().numpy(), E.loss_weights().cpu().numpy()

    eager, graph = run(False), run(True)
    for a, b in zip(eager, graph):
        np.testing.assert_array_equal(a, b)
    assert eager[1][11] == 4


# ---------------------------------------------------------------- ev drop-in
def test_ev_dropin_runs_with_loss_balancing(tmp_path):
    import scipy.io
    work = tmp_path / "ev"
    subprocess.run(["cp", "-r", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet"), str(work)], check=True)
    X, Y = np.meshgrid(np.linspace(0, 1, 33), np.linspace(0, 1, 33))
    dns = str(tmp_path / "dns.mat")
    scipy.io.savemat(dns, dict(X_ref=X, Y_ref=Y, U_ref=np.sin(np.pi * X) * Y, V_ref=-0.1 * np.cos(np.pi * Y) * X,
                               P_ref=X * Y))
    (work / "cfg.yaml").write_text(
        "experiment_name: t\nphysics: {Re: 2000, alpha_evm: 0.05, bc_weight: 10, eq_weight: 1}\n"
        "network: {layers: 3, layers_1: 2, hidden_size: 32, hidden_size_1: 16}\n"
        "training:\n  N_f: 2000\n  log_interval: 2\n  enable_tensorboard: false\n"
        "  loss_balancing: {enabled: true, every: 2, beta: 0.5}\n"
        "  training_stages:\n    - {alpha: 0.05, epochs: 4, lr: 1.0e-3, name: 'Stage 1'}\n"
        "    - {alpha: 0.03, epochs: 3, lr: 2.0e-4, name: 'Stage 2'}\n"
        "supervision: {enabled: true, num_samples: 30, loss_weight: 0.5}\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "train.py", "--config", "cfg.yaml", "--data", dns], cwd=str(work),
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "balancing  : every=2 beta=0.5" in out
    lams = [float(line.split("lambda_b=")[1].split()[0]) for line in out.splitlines() if "lambda_b=" in line]
    assert len(lams) >= 3 and lams[-1] != 10.0 and all(np.isfinite(lams))
    assert "lambda_s=" in out and out.count("Error p:") == 2
    assert list((work / "results").rglob("*lamB10*"))
