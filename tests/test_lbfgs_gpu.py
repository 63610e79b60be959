"""GPU tests of the L-BFGS optimizer: the direction kernels (csrc/lbfgs.hip) against the fp64 model, a device
trajectory against torch.optim.LBFGS on the autograd oracle, the headline and ev shapes, graph replay around an
L-BFGS stage, chunked passes, resets and the ev drop-in's lbfgs stage."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lbfgs_model import LbfgsModel  # noqa: E402

DEV = torch.device("cuda:0")


# ---------------------------------------------------------------- 5. kernels vs the model
@pytest.mark.parametrize("n", [1, 257, 330499, 1125203])
@pytest.mark.parametrize("m", [1, 7, 100])
def test_direction_kernels_match_the_model(n, m):
    """One push sequence fed to two device histories (bit-reproducibility) and to the fp64 model, compared push by
    push.  d_prev is set by the caller (random), so s and y stay O(1); every 4th pair has y's < 0 (rejected)."""
    from nsfnet_amd import engine as eng
    rng = np.random.RandomState(n + m)
    A = (1.0 + rng.rand(n)).astype(np.float32)
    h1, h2 = eng.LbfgsHistory(n, m, DEV), eng.LbfgsHistory(n, m, DEV)
    mod = LbfgsModel(n, m)
    g = rng.randn(n).astype(np.float32)
    t = 0.0
    wrapped, rejected = False, 0
    for k in range(m + 12 + (m + 12) // 3):
        if k > 0:
            t = 0.5
            dp = rng.randn(n).astype(np.float32)
            for h in (h1, h2):
                h.d.copy_(torch.from_numpy(dp))
            mod.d = dp.astype(np.float64)
            s = np.float32(t) * dp
            sign = -1.0 if k % 4 == 3 else 1.0
            g = (g + sign * A * s + np.float32(1e-3) * rng.randn(n).astype(np.float32) * np.abs(s)).astype(np.float32)
        gd = torch.from_numpy(g).to(DEV)
        r = h1.direction(gd, t).cpu().numpy().copy()
        r2 = h2.direction(gd, t).cpu().numpy().copy()
        g64 = g.astype(np.float64)
        rm = mod.direction(g64, t)
        d, d2 = h1.d.cpu().numpy(), h2.d.cpu().numpy()
        assert np.array_equal(d, d2) and np.array_equal(r, r2), k          # bit-reproducible
        assert r[4] == rm[4] and r[5] == rm[5], (k, r[4:6], rm[4:6])       # same accept / reject, same pair count
        wrapped |= r[5] == m and r[4] == 1
        rejected += r[4] == 0
        dm = mod.d
        assert np.linalg.norm(d - dm) <= 1e-5 * np.linalg.norm(dm), (k, np.linalg.norm(d - dm) / np.linalg.norm(dm))
        gtd = g64 @ d.astype(np.float64)
        assert abs(r[0] - gtd) <= 1e-6 * abs(gtd), k                       # the kernel's g'd of its own d
        assert abs(r[0] - g64 @ dm) <= 1e-5 * abs(g64 @ dm), k
        assert r[3] == np.abs(g64).max() and abs(r[2] - np.abs(g64).sum()) <= 1e-12 * np.abs(g64).sum()
    assert wrapped and rejected >= 3


# ---------------------------------------------------------------- 6. trajectory vs torch.optim.LBFGS (fp64 oracle)
def _record_losses(monkeypatch):
    from nsfnet_amd import engine as eng
    seen = []
    orig = eng._EngineSpace.evaluate

    def evaluate(self):
        v = orig(self)
        seen.append(v[0])
        return v
    monkeypatch.setattr(eng._EngineSpace, "evaluate", evaluate)
    return seen


def test_lbfgs_trajectory_tracks_torch_on_the_oracle(monkeypatch, tmp_path):
    from nsfnet_amd import pinn_solver as ps
    from oracle import autograd_ref as ar
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("NSFNET_PRECISION", "fp32")
    L, H, N, Re = 3, 24, 512, 100.0
    rng = np.random.RandomState(5)
    x, y = rng.rand(N, 1), rng.rand(N, 1)
    net = ar.seeded_net(3, L, H, seed=77)
    flat0 = ar.flat_params(net).numpy().copy()
    net = net.double()
    o = ar.NSFnetOracle(net, Re, alpha_b=10.0, alpha_e=1.0)
    o.set_data(x, y, *ar.cavity_boundary())
    ref_losses = []
    opt_ref = torch.optim.LBFGS(net.parameters(), lr=1, max_iter=10, history_size=10, line_search_fn="strong_wolfe")

    def closure():
        opt_ref.zero_grad()
        loss = o.loss()
        loss.backward()
        ref_losses.append(float(loss.detach()))
        return loss
    opt_ref.step(closure)

    P = ps.PysicsInformedNeuralNetwork(Re=Re, layers=L, hidden_size=H, N_f=N, bc_weight=10, eq_weight=1)
    P.net.dev_net.set_flat(torch.tensor(flat0))
    P.set_boundary_data(X=ar.cavity_boundary())
    P.set_eq_training_data(X=(x, y))
    P.save_every = 0; P.log_every = 0
    seen = _record_losses(monkeypatch)
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1, max_iter=10, history_size=10, line_search_fn="strong_wolfe")
    P.train(num_epoch=1, lr=1.0, optimizer=opt)
    assert len(seen) == len(ref_losses), (seen, ref_losses)
    np.testing.assert_allclose(seen, ref_losses, rtol=1e-3)
    with torch.no_grad():
        ref = net(torch.tensor(np.hstack([x, y]), dtype=torch.float64)).numpy()
    mine = torch.stack(P.engine.predict(x.astype(np.float32), y.astype(np.float32)), dim=1).cpu().numpy()
    for c in range(3):
        assert np.linalg.norm(mine[:, c] - ref[:, c]) < 2e-3 * np.linalg.norm(ref[:, c]), c
    assert ref_losses[-1] < 0.7 * ref_losses[0]      # it actually moved


def test_new_lbfgs_object_after_adam_tracks_torch(monkeypatch, tmp_path):
    """LBFGS(a) -> 3 Adam steps -> a NEW LBFGS(b), on the device and with two fresh torch.optim.LBFGS objects on the
    fp64 oracle: b starts from d = -g and its 1/|g|_1 step, as torch's does, so the evaluated losses agree."""
    from nsfnet_amd import pinn_solver as ps
    from oracle import autograd_ref as ar
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("NSFNET_PRECISION", "fp32")
    L, H, N, Re = 3, 24, 512, 100.0
    rng = np.random.RandomState(6)
    x, y = rng.rand(N, 1), rng.rand(N, 1)
    net = ar.seeded_net(3, L, H, seed=78)
    flat0 = ar.flat_params(net).numpy().copy()
    net = net.double()
    o = ar.NSFnetOracle(net, Re, alpha_b=10.0, alpha_e=1.0, lr=1e-3)
    o.set_data(x, y, *ar.cavity_boundary())
    ref_losses = []
    knobs = dict(lr=1, max_iter=5, history_size=10, line_search_fn="strong_wolfe")

    def run_ref():
        opt_ref = torch.optim.LBFGS(net.parameters(), **knobs)

        def closure():
            opt_ref.zero_grad()
            loss = o.loss()
            loss.backward()
            ref_losses.append(float(loss.detach()))
            return loss
        opt_ref.step(closure)
        opt_ref.zero_grad()
    run_ref()
    for _ in range(3):
        o.step(1e-3)
    run_ref()

    P = ps.PysicsInformedNeuralNetwork(Re=Re, layers=L, hidden_size=H, N_f=N, bc_weight=10, eq_weight=1)
    P.net.dev_net.set_flat(torch.tensor(flat0))
    P.set_boundary_data(X=ar.cavity_boundary())
    P.set_eq_training_data(X=(x, y))
    P.save_every = 0; P.log_every = 0
    seen = _record_losses(monkeypatch)
    P.train(num_epoch=1, lr=1.0, optimizer=torch.optim.LBFGS(P.net.parameters(), **knobs))
    P.set_optimizers(ps.AdamHandle(1e-3))
    P.train(num_epoch=3, lr=1e-3)
    P.train(num_epoch=1, lr=1.0, optimizer=torch.optim.LBFGS(P.net.parameters(), **knobs))
    assert len(seen) == len(ref_losses), (seen, ref_losses)
    np.testing.assert_allclose(seen, ref_losses, rtol=1e-3)


# ---------------------------------------------------------------- 7. headline and ev shapes
def _engine(flavour, n_pts, precision, seed=0, **kw):
    from nsfnet_amd import engine as eng
    from oracle import autograd_ref as ar
    rng = np.random.RandomState(seed)
    if flavour == "ev":
        E = eng.PinnEngine(DEV, 6, 80, 2000.0, alpha_b=10.0, alpha_e=1.0, flavour="ev", n_hidden_e=4, hidden_e=40,
                           alpha_evm=0.03, precision=precision)
        E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=seed + 1)))
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 80, seed=seed)))
        w = (0.2 + rng.rand(n_pts)).astype(np.float32)
    else:
        E = eng.PinnEngine(DEV, 6, 256, 100.0, alpha_b=10.0, alpha_e=1.0, precision=precision)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=seed)))
        w = None
    x, y = rng.rand(n_pts).astype(np.float32), rng.rand(n_pts).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1).astype(np.float32) for a in ar.cavity_boundary())
    E.set_collocation(x, y, weights=w, **kw)
    E.set_boundary(xb, yb, ub, vb)
    return E


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_lbfgs_after_adam_decreases_the_loss(flavour):
    E = _engine(flavour, 360000 if flavour == "nsfnet" else 120000, "bf16x3")
    for _ in range(200):
        E.step(1e-3)
    snap = {}
    if E.net_e is not None:
        snap = dict(pe=E.net_e.params.clone(), vtm=E.plan_f.vis_t_minus.clone())
        for k, net in (("", E.net), ("e", E.net_e)):
            snap.update({k + "m": net.m.clone(), k + "v": net.v.clone(), k + "td": net.adam_t_dev.clone()})
        t_host = (E.net.adam_t, E.net_e.adam_t)
    losses = [E.lbfgs_step(lr=1.0, max_iter=1, max_eval=25, history_size=100, line_search_fn="strong_wolfe")
              for _ in range(10)]
    E.loss_and_grad()
    losses.append(float(E.loss_terms()["loss"]))
    assert all(np.isfinite(losses)) and bool(torch.isfinite(E.net.params).all())
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    if E.net_e is not None:
        assert torch.equal(E.net_e.params, snap["pe"]) and torch.equal(E.plan_f.vis_t_minus, snap["vtm"])
        for k, net in (("", E.net), ("e", E.net_e)):
            assert torch.equal(net.m, snap[k + "m"]) and torch.equal(net.v, snap[k + "v"])
            assert torch.equal(net.adam_t_dev, snap[k + "td"])
        assert (E.net.adam_t, E.net_e.adam_t) == t_host


# ---------------------------------------------------------------- 8. graph replay around an L-BFGS stage
def _adam_lbfgs_adam(monkeypatch, graph):
    from nsfnet_amd import pinn_solver as ps
    from oracle import autograd_ref as ar
    monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
    torch.manual_seed(3)
    P = ps.PysicsInformedNeuralNetwork(Re=400.0, layers=3, hidden_size=40, N_f=900, bc_weight=10.0, eq_weight=1.0)
    x, y = ar.uniform_grid(30, 30)
    P.set_boundary_data(X=ar.cavity_boundary())
    P.set_eq_training_data(X=(x, y))
    P.log_every = 0; P.save_every = 0
    P.train(num_epoch=5, lr=1e-3)
    P.train(num_epoch=3, lr=1.0, optimizer=torch.optim.LBFGS(P.net.parameters(), max_iter=1, max_eval=25,
                                                             line_search_fn="strong_wolfe"))
    P.set_optimizers(ps.AdamHandle(1e-3))
    P.train(num_epoch=5, lr=1e-3)
    torch.cuda.synchronize()
    return P.engine.net.params.cpu().numpy().copy(), P.engine.net.adam_t


def test_graph_replay_around_lbfgs_is_bit_identical(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    p_e, t_e = _adam_lbfgs_adam(monkeypatch, False)
    p_g, t_g = _adam_lbfgs_adam(monkeypatch, True)
    assert t_e == t_g == 10
    assert np.array_equal(p_e, p_g)


# ---------------------------------------------------------------- 9. chunked passes
def test_chunked_passes_give_the_same_lbfgs_run(monkeypatch):
    N = 30000
    runs = []
    for chunk in (None, N // 3):
        E = _engine("nsfnet", N, "fp32", seed=4, chunk_points=chunk)
        seen = _record_losses(monkeypatch)
        E.lbfgs_step(lr=1.0, max_iter=5, history_size=10, line_search_fn="strong_wolfe")
        runs.append((list(seen), E.net.params.cpu().numpy().copy()))
        monkeypatch.undo()
    (l1, p1), (l2, p2) = runs
    assert len(l1) == len(l2)
    np.testing.assert_allclose(l2, l1, rtol=1e-6)
    assert np.linalg.norm(p2 - p1) <= 1e-5 * np.linalg.norm(p1)


# ---------------------------------------------------------------- 10. resets
def test_resample_resets_the_history():
    from oracle import autograd_ref as ar
    E = _engine("nsfnet", 4000, "fp32", seed=2)
    E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=2)))
    rng = np.random.RandomState(9)
    E.set_resample_pool(rng.rand(12000).astype(np.float32), rng.rand(12000).astype(np.float32))
    for _ in range(2):
        E.lbfgs_step(lr=1.0, max_iter=1, max_eval=25, history_size=5, line_search_fn="strong_wolfe")
    assert E._lbfgs_state.n_iter == 2 and E._lbfgs.result[4].item() != -1
    E.resample(k=1.0, c=1.0, seed=0)
    assert E._lbfgs_state.n_iter == 0
    E.lbfgs_step(lr=1.0, max_iter=1, history_size=5, line_search_fn="strong_wolfe")
    assert E._lbfgs.result[4].item() == -1 and E._lbfgs.result[5].item() == 0     # a first iteration
    E.lbfgs_step(lr=1.0, max_iter=1, history_size=7)                              # new history size: fresh state
    assert E._lbfgs_state.n_iter == 1 and E._lbfgs.history_size == 7


# ---------------------------------------------------------------- 11. ev drop-in with an lbfgs stage
def test_ev_dropin_runs_an_lbfgs_stage(tmp_path):
    import scipy.io
    work = tmp_path / "ev"
    subprocess.run(["cp", "-r", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet"), str(work)], check=True)
    X, Y = np.meshgrid(np.linspace(0, 1, 33), np.linspace(0, 1, 33))
    dns = str(tmp_path / "dns.mat")
    scipy.io.savemat(dns, dict(X_ref=X, Y_ref=Y, U_ref=np.sin(np.pi * X) * Y, V_ref=-0.1 * np.cos(np.pi * Y) * X,
                               P_ref=X * Y))
    (work / "cfg.yaml").write_text(
        "experiment_name: t\nphysics: {Re: 2000, alpha_evm: 0.05, bc_weight: 10, eq_weight: 1}\n"
        "network: {layers: 3, layers_1: 2, hidden_size: 48, hidden_size_1: 20}\n"
        "training:\n  N_f: 3000\n  log_interval: 2\n  enable_tensorboard: false\n"
        "  training_stages:\n    - {alpha: 0.05, epochs: 4000, lr: 1.0e-3, name: 'Stage 1'}\n"
        "    - {alpha: 0.05, epochs: 5000, lr: 1.0, name: 'Finish', optimizer: lbfgs, history_size: 20,"
        " line_search: strong_wolfe}\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "train.py", "--config", "cfg.yaml", "--data", dns, "--epochs-scale", "1e-3"],
                       cwd=str(work), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("Error p:") == 2
    cks = sorted(str(p) for p in (work / "results").rglob("model_cavity_loop0.pth"))
    assert len(cks) == 2 and any("Finish" in c for c in cks) and all(os.path.exists(c + "_evm") for c in cks)
