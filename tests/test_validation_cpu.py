"""CPU tests of the device validation monitor: the fp64 model against a direct evaluation of
the definitions, and the host logic around the entry points on the model-backed fakes - the cadence and t across
step(), loss_and_grad() + adam_step() and lbfgs_step(), the graph key, the off path, the snapshot and restore, the
solvers' surface (log, save, load_best, patience), the ev drop-in's YAML key and the convergence script's arguments.
The kernels are checked against the model in test_validation_gpu.py."""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rwf_model  # noqa: E402
import val_model as vm  # noqa: E402

L, H, RE = 2, 10, 400.0
SHAPE, SHAPE_E = (3, L, H), (1, 2, 6)
LR = 2.0 ** -10


# ------------------------------------------------------------------ the model
def _fields(n, seed, nan_frac=0.0):
    rng = np.random.RandomState(seed)
    tgt = [rng.randn(n).astype(np.float32) for _ in range(3)]
    pred = [(t + 0.1 * rng.randn(n)).astype(np.float32) for t in tgt]
    pred[2] = (pred[2] + np.float32(0.7)).astype(np.float32)
    if nan_frac:
        tgt[2][rng.rand(n) < nan_frac] = np.nan
    return pred, tgt


@pytest.mark.parametrize("n,nan_frac", [(1, 0.0), (7, 0.0), (501, 0.0), (501, 0.2), (501, 1.0)])
def test_model_matches_the_definitions(n, nan_frac):
    pred, tgt = _fields(n, n, nan_frac)
    S = vm.sums(pred, tgt)
    assert S[2] == S[5] == n and S[8] == np.sum(~np.isnan(tgt[2]))
    direct = vm.direct_errors(pred, tgt)
    for name, want in zip(("u", "v", "p", "p0", "uv"), direct):
        got = vm.errors(S, name)[4]
        if np.isnan(want) or (name == "p0" and S[8] < 2):
            assert np.isnan(got) or S[8] == 1, (name, got, want)
        else:
            assert abs(got - want) <= 1e-9 * abs(want), (name, got, want)
    if nan_frac == 1.0:        # no valid pressure target: its entries are NaN, the others intact
        e = vm.errors(S, "uv")
        assert np.isnan(e[2]) and np.isnan(e[3]) and np.isfinite(e[4]) and np.isnan(vm.errors(S, "p")[4])


def test_model_masks_nan_velocity_targets_and_removes_the_pressure_offset():
    pred, tgt = _fields(300, 3)
    tgt[0][::7] = np.nan
    S = vm.sums(pred, tgt)
    assert S[2] == 300 - len(range(0, 300, 7)) and S[5] == 300
    shifted = [pred[0], pred[1], (pred[2].astype(np.float64) + 5.0).astype(np.float32)]
    a, b = vm.errors(vm.sums(pred, tgt), "p0"), vm.errors(vm.sums(shifted, tgt), "p0")
    assert abs(a[3] - b[3]) <= 1e-5 * a[3] and b[2] > 3 * a[2]          # e_p0 ignores the constant, e_p does not


def test_model_state_and_ring():
    st, ring = vm.new_state(), np.zeros((4, vm.RECORD))
    S = lambda m: np.array([m * m, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])       # metric u = m
    imp = []
    for m in [0.5, 0.3, 0.4, float("nan"), 0.3, 0.1]:
        imp.append(vm.record(S(m), "u", -1.0, 3, st, ring)[vm.R_IMPROVED])
    assert imp == [1, 1, 0, 0, 0, 1]
    assert st[vm.S_RECORDS] == 6 and st[vm.S_BEST_T] == 18 and st[vm.S_STALE] == 0 and st[vm.S_NONFINITE] == 1
    np.testing.assert_array_equal(vm.history(st, ring)[:, vm.R_T], [9, 12, 15, 18])
    vm.record(S(0.2), "u", 40.0, 3, st, ring)
    assert vm.history(st, ring)[-1, vm.R_T] == 40.0 and st[vm.S_CADENCE] == 6 and st[vm.S_STALE] == 1
    assert vm.record(S(0.05), "u", -1.0, 3, st, ring)[vm.R_T] == 21.0       # an on-demand row does not shift the cadence


# ------------------------------------------------------------------ the engine on the fakes
def _case(seed=42, N=70, Nb=33, Nv=41):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    xv, yv = rng.rand(Nv).astype(np.float32), rng.rand(Nv).astype(np.float32)
    val = (xv, yv, np.sin(3 * xv) * yv, np.cos(2 * yv) * xv, 0.2 + xv * yv)
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb, val=tuple(a.astype(np.float32) for a in val))


def _engine(monkeypatch, case, flavour="nsfnet", **kw):
    import val_fakes
    val_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=SHAPE_E[1], hidden_e=SHAPE_E[2], alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev, **kw)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"])
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    return e


def _key(monkeypatch, e):
    """The graph key step() looks up (the probe of test_rba_cpu.py)."""
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
    with pytest.raises(Stop):
        e.step(LR)
    e._graphs = old
    monkeypatch.setattr(e, "_graphs_enabled", lambda: False)
    return keys[0]


def _planes(e, case):
    return [t.numpy().copy() for t in e.predict(case["val"][0], case["val"][1])]


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_off_makes_the_parents_calls(monkeypatch, flavour):
    """Never set, or set and switched off again (every = 0, x = None): the same call log step by step, with no
    validation entry point in it, and the parent's graph key."""
    import val_fakes
    case = _case()
    engines = [_engine(monkeypatch, case, flavour) for _ in range(3)]
    engines[1].set_validation(*case["val"], every=2)
    engines[1].set_validation(*case["val"], every=0)
    engines[2].set_validation(*case["val"], every=2)
    engines[2].set_validation(None, None)
    logs = []
    for e in engines:
        assert e.validation_info() is None and e.best_state_dict() is None
        del val_fakes.CALLS[:]
        for _ in range(3):
            e.step(LR)
        e.lbfgs_step(max_iter=1)
        logs.append(list(val_fakes.CALLS))
    assert logs[0] == logs[1] == logs[2] and logs[0]
    assert not any(c[0].startswith("val_") for c in logs[0])
    keys = [_key(monkeypatch, e) for e in engines]
    assert keys[0] == keys[1] == keys[2] and "validate" not in keys[0]
    for a, b in zip(engines[0].net.params, engines[1].net.params):
        assert a == b
    with pytest.raises(RuntimeError):
        engines[0].validate()
    with pytest.raises(RuntimeError):
        engines[0].restore_best()


def test_cadence_and_t_across_step_adam_step_and_lbfgs(monkeypatch):
    """every = 2: validations follow updates 2, 4, 6 whichever call made the update, each after the update's prepare,
    and record t describes the parameters after t updates."""
    import val_fakes
    case = _case()
    e, twin = _engine(monkeypatch, case), _engine(monkeypatch, case)
    e.set_validation(*case["val"], every=2, metric="uv", history=8)
    del val_fakes.CALLS[:]
    st, ring = vm.new_state(), np.zeros((8, vm.RECORD))
    tgt = list(case["val"][2:])

    mine = []                                           # the calls of the engine with the monitor

    def both(fn):
        k = len(val_fakes.CALLS)
        fn(e)
        mine.extend(val_fakes.CALLS[k:])
        fn(twin)

    both(lambda E: E.step(LR))                                           # update 1
    assert not any(c[0] == "val_stats" for c in mine)
    both(lambda E: (E.loss_and_grad(), E.adam_step(LR)))                # update 2: validated
    vm.validate(_planes(twin, case), tgt, "uv", -1.0, 2, st, ring)
    names = [c[0] for c in mine]
    assert names.count("val_stats") == 1 and names[-2:] == ["val_stats", "val_keep"]
    assert names.index("val_stats") > max(i for i, n in enumerate(names) if n == "adam_step")
    both(lambda E: E.lbfgs_step(max_iter=2))                             # update 3: one call, one update
    assert e._val.n == 3 and [c[0] for c in mine].count("val_stats") == 1
    both(lambda E: E.lbfgs_step(max_iter=2))                             # update 4: validated at the accepted point
    vm.validate(_planes(twin, case), tgt, "uv", -1.0, 2, st, ring)
    both(lambda E: E.step(LR)); both(lambda E: E.step(LR))               # updates 5, 6
    vm.validate(_planes(twin, case), tgt, "uv", -1.0, 2, st, ring)
    hist = e.validation_history()
    np.testing.assert_array_equal(hist[:, vm.R_T], [2.0, 4.0, 6.0])
    np.testing.assert_allclose(hist, vm.history(st, ring), rtol=1e-12)
    np.testing.assert_array_equal(e.net.params.numpy(), twin.net.params.numpy())      # the monitor only observes
    info = e.validation_info()
    assert info["records"] == 3 and info["every"] == 2 and info["metric"] == "uv" and info["points"] == 41
    assert info["best_t"] == st[vm.S_BEST_T] and info["stale"] == st[vm.S_STALE] and info["last"]["t"] == 6.0
    row = e.validate()                                                   # on demand: t = the updates counted
    assert row["t"] == 6.0 and e.validation_info()["records"] == 4 and row["improved"] == 0.0
    assert e.validate(t=99)["t"] == 99.0
    with pytest.raises(ValueError):
        e.validate(t=-1)                                                 # -1 is the cadence's own marker
    e.step(LR); e.step(LR)
    assert e.validation_history()[-1, vm.R_T] == 8.0                     # the cadence carries on


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_snapshot_restore_and_the_ring(monkeypatch, flavour):
    case = _case()
    e, twin = _engine(monkeypatch, case, flavour), _engine(monkeypatch, case, flavour)
    e.e_trainable = twin.e_trainable = flavour == "ev"
    assert e.validation_info() is None
    e.set_validation(*case["val"], every=1, metric="p0", history=3)
    assert e.best_state_dict() is None and e.validation_info()["last"] is None
    with pytest.raises(RuntimeError):
        e.restore_best()
    seen = []
    for _ in range(5):
        e.step(LR); twin.step(LR)
        seen.append(([n.trainable.numpy().copy() for _, n in twin._nets()], twin.net.state_dict(), _planes(twin, case)))
    hist = e.validation_history()
    assert hist.shape == (3, vm.RECORD)
    np.testing.assert_array_equal(hist[:, vm.R_T], [3.0, 4.0, 5.0])     # the ring keeps the newest `history` rows
    info = e.validation_info()
    best = int(info["best_t"]) - 1
    assert len(e._val.snap) == (2 if flavour == "ev" else 1)
    for snap, want in zip(e._val.snap, seen[best][0]):
        np.testing.assert_array_equal(snap.numpy(), want)
    for k, v in seen[best][1].items():
        assert torch.equal(e.best_state_dict()[k], v)
    assert (e.best_state_dict_e() is not None) == (flavour == "ev")
    e.restore_best()
    for got, want in zip(_planes(e, case), seen[best][2]):
        np.testing.assert_array_equal(got, want)
    e.set_validation(*case["val"], every=1, keep_best=False)
    e.step(LR)
    assert e.validation_info()["records"] == 1 and e.best_state_dict() is None


def test_graph_key_separates_plain_and_validating_steps(monkeypatch):
    case = _case()
    e, off = _engine(monkeypatch, case), _engine(monkeypatch, case)
    plain = _key(monkeypatch, off)
    e.set_validation(*case["val"], every=2, metric="u")
    k1 = _key(monkeypatch, e)                          # the next update is the first: plain
    assert k1 == plain
    e.step(LR)
    k2 = _key(monkeypatch, e)                          # the next update is the second: validating
    assert k2 != plain and k2[:len(plain)] == plain and k2[len(plain):] == ("validate", 2, "u", True, 41, True)
    e.set_validation(*case["val"][:4], every=1, metric="v", keep_best=False)
    assert _key(monkeypatch, e)[len(plain):] == ("validate", 1, "v", False, 41, False)
    e._graphs["x"] = 1
    e.set_validation(*case["val"], every=3)
    assert not e._graphs                               # a new monitor: the captured steps go


def test_refusals(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    x, y, u, v, p = case["val"]
    with pytest.raises(ValueError, match="metric"):
        e.set_validation(x, y, u, v, p, metric="w")
    with pytest.raises(ValueError, match="pressure"):
        e.set_validation(x, y, u, v, None, metric="p0")
    with pytest.raises(ValueError, match="every"):
        e.set_validation(x, y, u, v, p, every=-1)
    with pytest.raises(ValueError, match="history"):
        e.set_validation(x, y, u, v, p, history=0)
    with pytest.raises(ValueError, match="one entry per point"):
        e.set_validation(x, y, u[:-1], v, p)
    assert e.validation_info() is None


def test_weight_factorization_snapshot_is_theta_and_a_change_drops_the_best(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, "ev")
    e.set_weight_factorization(seed=3)
    e.set_validation(*case["val"], every=1)
    e.step(LR)
    theta = e.net.theta.numpy().copy()
    assert e._val.snap[0].numel() == e.P + rwf_model.num_rows(*SHAPE)
    np.testing.assert_array_equal(e._val.snap[0].numpy(), theta)
    flat = torch.cat([t.reshape(-1) for t in e.best_state_dict().values()]).numpy()
    np.testing.assert_array_equal(flat, rwf_model.compose(theta, SHAPE))             # the effective weights
    fac = e.best_factors()
    np.testing.assert_array_equal(torch.cat(fac["net"]).numpy(), theta[e.P:])
    e.step(LR); e.step(LR)
    e._val.snap[0].copy_(torch.tensor(theta))          # whichever was best: restore what the snapshot holds
    e.restore_best()
    np.testing.assert_array_equal(e.net.theta.numpy(), theta)
    np.testing.assert_array_equal(e.net.params.numpy(), rwf_model.compose(theta, SHAPE))
    e.set_weight_factorization(None)
    assert e.best_state_dict() is None and e.validation_info()["records"] == 0 and e._val.n == 0
    assert e._val.snap[0].numel() == e.P


# ------------------------------------------------------------------ the solvers
def _plain(monkeypatch, case):
    import val_fakes
    val_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=L, hidden_size=H, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_every = P.save_every = 0
    return P


def _ev(monkeypatch, case):
    import val_fakes
    val_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(0)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=L, layers_1=SHAPE_E[1], hidden_size=H, hidden_size_1=SHAPE_E[2],
                                       N_f=70, alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_interval = 1000
    return P


def _files(tmp_path, prefix):
    return sorted(f for _, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith(prefix))


def test_plain_solver_surface(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    case = _case()
    P = _plain(monkeypatch, case)
    P.save("off.pth", N_HLayer=L, N_neu=H, N_f=70)
    assert _files(tmp_path, "off.pth") == ["off.pth"]                   # nothing beside the checkpoint with it off
    x, y, u, v, p = case["val"]
    P.set_validation_data(x, y, u, v, every=2)                           # the plain flavour has no p
    assert P.validation_log() == "validation: no record yet" and P.best_state_dict() is None
    with pytest.raises(RuntimeError):
        P.load_best()
    P.log_every = 1
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=4, lr=1e-3)
    assert "validation (t=4): e_u=" in out.getvalue() and "best uv=" in out.getvalue()
    assert P.engine.validation_info()["records"] == 2
    assert np.isnan(P.validation_history()[:, vm.R_EP]).all()
    P.save("on.pth", N_HLayer=L, N_neu=H, N_f=70)
    assert _files(tmp_path, "on.pth") == ["on.pth", "on.pth_best"]
    ck = [os.path.join(d, "on.pth_best") for d, _, fs in os.walk(str(tmp_path)) if "on.pth_best" in fs][0]
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    assert list(sd) == [k for k, _ in P.net.dev_net.keys_and_shapes()]            # the reference's checkpoint format
    for k, t in P.best_state_dict().items():
        assert torch.equal(sd[k], t)
    P.load_best()
    np.testing.assert_array_equal(P.engine.net.params.numpy(), torch.cat([sd[k].reshape(-1) for k in sd]).numpy())
    P.set_validation_data(None, None, None, None)
    assert not P._validation and P.engine.validation_info() is None


def test_ev_solver_saves_both_nets_and_the_factors(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    case = _case()
    P = _ev(monkeypatch, case)
    P.set_weight_factorization(seed=9)
    P.set_validation_data(*case["val"], every=1, metric="p0")
    real_save, P.save = P.save, lambda *a, **k: None
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=3, lr=1e-3)
    assert "validation (t=3)" in out.getvalue() and "best p0=" in out.getvalue()
    real_save("ck.pth", N_HLayer=L, N_neu=H, N_f=70)
    assert _files(tmp_path, "ck.pth") == ["ck.pth", "ck.pth_best", "ck.pth_best_evm", "ck.pth_best_rwf", "ck.pth_evm",
                                          "ck.pth_rwf"]
    side = [os.path.join(d, "ck.pth_best_rwf") for d, _, fs in os.walk(str(tmp_path)) if "ck.pth_best_rwf" in fs][0]
    fac = torch.load(side, map_location="cpu", weights_only=True)
    assert sorted(fac) == ["net", "net_e"]
    np.testing.assert_array_equal(fac["net"].numpy(), P.engine._val.snap[0].numpy()[P.engine.P:])


@pytest.mark.parametrize("kind", ["adam", "lbfgs"])
def test_patience_ends_a_stage(monkeypatch, kind):
    case = _case()
    P = _plain(monkeypatch, case)
    x, y, u, v, p = case["val"]
    P.set_validation_data(x, y, u, v, every=1, patience=2)
    P.log_every = 1
    from nsfnet_amd import engine as eng
    real = eng.val_stats
    script = iter([0.5] + [0.9] * 50)

    def scripted(pred, tgt, n, with_p, metric, t, every, scratch, state, ring):     # first an improvement, then none
        m = next(script)
        pred[0, :n] = tgt[0, :n] * (1.0 + m); pred[1, :n] = tgt[1, :n] * (1.0 + m)
        real(pred, tgt, n, with_p, metric, t, every, scratch, state, ring)

    monkeypatch.setattr(eng, "val_stats", scripted)
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=1) if kind == "lbfgs" else None
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=20, lr=1e-3, optimizer=opt)
    info = P.engine.validation_info()
    assert info["records"] == 3 and info["stale"] == 2 and info["best_t"] == 1.0    # ended after 3 of 20 epochs
    with pytest.raises(ValueError, match="patience"):
        P.set_validation_data(x, y, u, v, patience=-1)


# ------------------------------------------------------------------ YAML and the script
def _config_module():
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_val", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_yaml_key_parses_and_is_validated(tmp_path):
    cfg = _config_module()
    prod = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                    "production.yaml"))
    va = prod.config.training.validation
    assert (va.enabled, va.every, va.metric, va.keep_best, va.patience) == (False, 1000, "uv", True, 0)
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  validation: {enabled: true, every: 500, metric: p0, keep_best: false, patience: 7}\n")
    va = cfg.ConfigManager.from_file(str(p)).config.training.validation
    assert (va.enabled, va.every, va.metric, va.keep_best, va.patience) == (True, 500, "p0", False, 7)
    for bad in ("every: 0", "metric: w", "patience: -1"):
        p.write_text("training:\n  validation: {enabled: true, %s}\n" % bad)
        with pytest.raises(ValueError, match="training.validation"):
            cfg.ConfigManager.from_file(str(p))
    p.write_text("training:\n  validation: {enabled: false, every: 0}\n")      # off: not looked at
    assert not cfg.ConfigManager.from_file(str(p)).config.training.validation.enabled
    out = io.StringIO()
    p.write_text("training:\n  validation: {enabled: true, every: 250}\n")
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "validation : every=250 metric=uv keep_best=True patience=0" in out.getvalue()


def test_converge_ev_wires_its_arguments(monkeypatch, tmp_path):
    """The script on the fakes, a 2 x 8 net and 40 points: 5 updates of stage 1 validated every 2 against the DNS file
    give two rows of validation.jsonl, the best weights of both nets and best_metric / best_t in the stage record."""
    import val_fakes
    val_fakes.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    spec = importlib.util.spec_from_file_location("converge_ev_val", os.path.join(ROOT, "scripts", "converge_ev.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    dns = os.path.join(ROOT, "tests", "golden", "dns", "cavity_Re3000_256_Uniform.mat")
    out = tmp_path / "run"
    monkeypatch.setattr(sys, "argv", ["converge_ev.py", "--dns", dns, "--out", str(out), "--first", "1", "--last", "1",
                                      "--epochs-scale", "1e-5", "--nf", "40", "--layers", "2", "--hidden", "8",
                                      "--validate-every", "2", "--val-metric", "u"])
    cwd = os.getcwd()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mod.main()
    finally:
        os.chdir(cwd)
    rows = [json.loads(l) for l in open(out / "validation.jsonl")]
    assert [r["t"] for r in rows] == [2.0, 4.0] and all(r["stage"] == 1 and r["metric"] == r["e_u"] for r in rows)
    assert all(r["n_p"] > 0 and np.isfinite(r["e_p0"]) for r in rows)
    rec = json.loads(open(out / "stages.jsonl").readline())
    assert rec["val_metric"] == "u" and rec["best_t"] in (2.0, 4.0)
    assert rec["best_metric"] == min(r["metric"] for r in rows)
    best = torch.load(out / "net_best.pth", map_location="cpu", weights_only=True)
    assert list(best) == list(torch.load(out / "net.pth", map_location="cpu", weights_only=True))
    assert os.path.exists(out / "net_best_evm.pth")
