"""CPU tests of the convergence monitor: the numpy model of tests/monitor_model.py on synthetic
sequences, the argument refusals of the C ABI (no device needed: they come before any launch), and the host logic
around the entry points on the model-backed fakes - the solvers' stage end, the ev drop-in's YAML key, the
training-state file with the monitor off and on, and two gloo ranks that must hold the same bits.  The kernels are
checked against the model in test_monitor_gpu.py."""
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

import fold_model as fm  # noqa: E402
import monitor_model as mm  # noqa: E402

L, H, RE = 2, 10, 400.0
SHAPE_E = (1, 2, 6)
LR = 2.0 ** -10


# ------------------------------------------------------------------ the model on synthetic sequences
def _run(cfg, losses, re=None):
    st, ring = mm.new_state(), mm.new_ring(cfg)
    for i, v in enumerate(losses):
        mm.observe_losses(cfg, st, ring, v, 1.0 if re is None else re[i])
    return st, ring


def _first_plateau(losses, window, patience, tol):
    """The rule, restated directly on the list of observed (finite) losses: the observation that sets the bit."""
    means = [np.mean(losses[k:k + window]) for k in range(0, len(losses) - window + 1, window)]
    stale = 0
    for j in range(1, len(means)):
        stale = stale + 1 if (means[j - 1] == 0 or (means[j - 1] - means[j]) / abs(means[j - 1]) < tol) else 0
        if stale >= patience:
            return (j + 1) * window
    return None


@pytest.mark.parametrize("window,patience", [(4, 2), (5, 3), (1, 1)])
def test_plateau_is_set_at_the_predicted_observation(window, patience):
    cfg = mm.Config(window=window, patience=patience, min_rel_improvement=1e-3, capacity=256)
    flat = [0.25] * 60
    st, ring = _run(cfg, flat)
    assert st[mm.S_T_PLATEAU] == (patience + 1) * window           # the first possible one
    decay = [0.5 ** k for k in range(3 * window + 1)]
    seq = decay + [decay[-1]] * (6 * window)
    want = _first_plateau(seq, window, patience, 1e-3)
    assert want is not None and want > (patience + 1) * window
    st, ring = _run(cfg, seq)
    assert st[mm.S_T_PLATEAU] == want and int(st[mm.S_STOP]) == mm.STOP_PLATEAU
    rows = mm.unwrap(st, ring)
    assert np.array_equal(rows[:, 0], np.arange(1, len(seq) + 1))
    assert np.array_equal(rows[:, 11], np.where(rows[:, 0] >= want, 1.0, 0.0))       # sticky from there on
    assert np.array_equal(rows[:, 1], np.asarray(seq))


def test_an_improving_window_restarts_the_count_and_a_zero_mean_is_stale():
    cfg = mm.Config(window=2, patience=2, min_rel_improvement=0.1, capacity=64)
    st, _ = _run(cfg, [1, 1, 1, 1, 0.5, 0.5, 0.5, 0.5])            # stale, improved, stale
    assert (st[mm.S_STALE], st[mm.S_STOP], st[mm.S_WINDOWS]) == (1.0, 0.0, 4.0)
    st, _ = _run(cfg, [1, 1, 0, 0, 0, 0, 0, 0])                    # improved to 0, then prev == 0 twice
    assert (st[mm.S_STALE], st[mm.S_T_PLATEAU]) == (2.0, 8.0)
    cfg = mm.Config(window=2, patience=1, min_rel_improvement=None, re_eff_tol=0.01, capacity=64, ev=True)
    st, _ = _run(cfg, [1.0] * 8, re=[100, 100, 200, 200, 201, 201, 300, 300])
    assert (st[mm.S_T_RE_EFF], st[mm.S_SETTLED], st[mm.S_T_PLATEAU]) == (6.0, 0.0, 0.0)


def test_min_updates_delays_the_bit():
    cfg = mm.Config(window=2, patience=1, min_rel_improvement=1e-3, min_updates=11, capacity=64)
    st, ring = _run(cfg, [3.0] * 20)
    assert st[mm.S_T_PLATEAU] == 11.0 and st[mm.S_STALE] >= 1.0
    assert np.array_equal(mm.unwrap(st, ring)[:, 11], np.where(np.arange(1, 21) >= 11, 1.0, 0.0))


def test_a_nan_sets_nonfinite_at_once_and_stays_out_of_the_window():
    cfg = mm.Config(window=3, patience=1, min_rel_improvement=1e-3, capacity=64)
    clean, _ = _run(cfg, [2.0, 2.0])
    st, ring = _run(cfg, [2.0, 2.0, np.nan])
    assert int(st[mm.S_STOP]) == mm.STOP_NONFINITE and st[mm.S_T_NONFINITE] == 3.0 and st[mm.S_NONFINITE] == 1.0
    for k in (mm.S_FILL, mm.S_SUM_Q, mm.S_SUM_RE, mm.S_WINDOWS, mm.S_PREV_Q, mm.S_STALE):
        assert st[k] == clean[k]
    assert st[mm.S_OBS] == 3.0 and np.isnan(ring[2, 1]) and ring[2, 11] == 4.0
    st2, _ = _run(cfg, [2.0, 2.0, np.inf, 2.0])                      # the window goes on where it was
    assert st2[mm.S_WINDOWS] == 1.0 and st2[mm.S_PREV_Q] == 2.0 and st2[mm.S_NONFINITE] == 1.0


def test_every_three_observes_updates_3_6_and_the_ring_wraps():
    cfg = mm.Config(every=3, window=2, patience=1, min_rel_improvement=1e-3, capacity=4)
    st, ring = mm.new_state(), mm.new_ring(cfg)
    seen = [mm.observe_losses(cfg, st, ring, float(i)) for i in range(1, 22)]
    assert [i + 1 for i, s in enumerate(seen) if s] == [3, 6, 9, 12, 15, 18, 21]
    assert (st[mm.S_UPDATES], st[mm.S_OBS]) == (21.0, 7.0)
    rows = mm.unwrap(st, ring)
    assert rows.shape == (4, mm.RECORD) and list(rows[:, 0]) == [12.0, 15.0, 18.0, 21.0]      # the newest four, in order
    assert list(rows[:, 1]) == [12.0, 15.0, 18.0, 21.0]
    assert np.array_equal(mm.new_state(), np.zeros(mm.STATE))


def test_terms_follow_the_header_order():
    eq = np.array([3.0, 5.0, 7.0, 11.0, 13.0, 0, 0, 0], dtype=np.float32)
    bc = np.array([2.0, 4.0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    sup = np.array([1.0, 2.0, 3.0, 5.0, 0, 0, 0, 0], dtype=np.float32)
    t = mm.terms(eq, bc, sup, None, 10.0, 0.5, 2.0, 0.1, 7.0, 3.0, 4.0, 5.0, 100.0, True)
    e = eq[:4].astype(np.float64) / 7.0
    loss_e = ((e[0] + e[1]) + e[2]) + 0.1 * e[3]
    loss_b, loss_s = 6.0 / 3.0, 3.0 / 4.0 + 3.0 / 5.0
    assert t[1] == loss_e and t[2] == loss_b and t[3] == loss_s
    assert t[0] == ((10.0 * loss_b) + (2.0 * loss_e)) + (0.5 * loss_s)
    assert t[8] == np.float64(13.0) / 7.0 and t[9] == 1.0 / (1.0 / 100.0 + t[8])
    plain = mm.terms(eq, bc, None, np.array([4.0, 9.0], np.float32), 10.0, 0.5, 2.0, 0.1, 7.0, 3.0, 0.0, 0.0, 100.0, False)
    assert plain[1] == (e[0] + e[1]) + e[2] and plain[3] == 0.0 and plain[8] == 0.0 and plain[9] == 100.0
    assert plain[0] == ((4.0 * loss_b) + (2.0 * plain[1])) + 0.0


@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 4099])
def test_vis_stats_model_against_a_direct_sum(n):
    rng = np.random.RandomState(n)
    v = (rng.rand(n) * 0.05).astype(np.float32)
    v[rng.rand(n) < 0.3] = np.float32(0.05)
    slot, info = mm.vis_stats(v, 0.05)
    assert abs(info[2] - np.sum(v.astype(np.float64))) <= 1e-13 * n and slot == np.float32(info[2])
    assert info[0] == v.max() and info[1] == np.sum(v >= np.float32(0.05)) and info[3] == n
    v[n // 2] = np.nan
    slot, info = mm.vis_stats(v, 0.05)
    assert np.isnan(slot) and np.isnan(info[0]) and np.isnan(info[2])


# ------------------------------------------------------------------ the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def test_abi_refuses_bad_configurations_by_name(lib):
    from nsfnet_amd import _lib
    assert lib.pinn_abi_version() == 3 and lib.pinn_monitor_scratch_bytes() > 0
    good = dict(every=1, window=4, patience=2, min_updates=0, capacity=8, quantity=0, ev=0, plateau_on=1, re_eff_on=0,
                min_rel_improvement=1e-3, re_eff_tol=0.0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        cfg = _lib.MonitorConfigStruct(**dict(good, **kw))
        return lib.pinn_monitor_observe(p, p, None, None, 1.0, 0.0, 1.0, 0.1, 10.0, 5.0, 0.0, 0.0, 100.0, ctypes.byref(cfg),
                                        p, p, None)

    for kw, word in ((dict(every=0), b"every"), (dict(window=0), b"window"), (dict(patience=0), b"patience"),
                     (dict(capacity=0), b"capacity"), (dict(min_updates=-1), b"min_updates"), (dict(quantity=3), b"quantity"),
                     (dict(min_rel_improvement=-1e-3), b"min_rel_improvement"),
                     (dict(min_rel_improvement=float("nan")), b"min_rel_improvement"),
                     (dict(re_eff_on=1, ev=1, re_eff_tol=float("inf")), b"re_eff_tol"),
                     (dict(re_eff_on=1, ev=1, re_eff_tol=-1.0), b"re_eff_tol"),
                     (dict(re_eff_on=1, ev=0, re_eff_tol=0.1), b"ev flavour")):
        assert call(**kw) == -22, kw
        assert word in lib.pinn_last_error(), (kw, lib.pinn_last_error())
    cfg = _lib.MonitorConfigStruct(**good)
    assert lib.pinn_monitor_observe(None, p, None, None, 1.0, 0.0, 1.0, 0.1, 10.0, 5.0, 0.0, 0.0, 100.0, ctypes.byref(cfg),
                                    p, p, None) == -22 and b"null argument" in lib.pinn_last_error()
    assert lib.pinn_monitor_observe(p, p, None, None, 1.0, 0.0, 1.0, 0.1, 0.0, 5.0, 0.0, 0.0, 100.0, ctypes.byref(cfg),
                                    p, p, None) == -22 and b"n_eq" in lib.pinn_last_error()
    assert lib.pinn_monitor_vis_stats(0, p, 0.05, p, p, p, None) == -22 and b"n must be" in lib.pinn_last_error()
    assert lib.pinn_monitor_vis_stats(4, None, 0.05, p, p, p, None) == -22 and b"null argument" in lib.pinn_last_error()
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.pinn_monitor_vis_stats(4, odd, 0.05, p, p, p, None) == -22 and b"16-byte" in lib.pinn_last_error()


# ------------------------------------------------------------------ the engine and the solvers on the fakes
def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", seed=5, setup=None):
    import monitor_fakes
    monitor_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=SHAPE_E[1], hidden_e=SHAPE_E[2], alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev)
    rng = np.random.RandomState(seed)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"])
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    if setup is not None:
        setup(e)
    return e


def _plain(monkeypatch, case):
    import monitor_fakes
    monitor_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=L, hidden_size=H, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_every = P.save_every = 0
    return P


def _ev(monkeypatch, case):
    import monitor_fakes
    monitor_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(0)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=L, layers_1=SHAPE_E[1], hidden_size=H, hidden_size_1=SHAPE_E[2],
                                       N_f=70, alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_interval = 1000
    P.save = lambda *a, **k: None
    return P


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_engine_rows_are_the_model_on_the_sums_and_agree_with_loss_terms(monkeypatch, flavour):
    import monitor_fakes
    case = _case()
    e = _engine(monkeypatch, case, flavour)
    e.set_convergence_monitor(window=2, patience=1, re_eff_tol=0.5 if flavour == "ev" else None, history=8)
    assert e.monitor_info()["last"] is None and not e.should_stop() and e.monitor_history().shape == (0, mm.RECORD)
    del monitor_fakes.CALLS[:]
    cfg = mm.Config(window=2, patience=1, re_eff_tol=0.5 if flavour == "ev" else None, capacity=8, ev=flavour == "ev")
    st, ring = mm.new_state(), mm.new_ring(cfg)
    for i in range(5):
        e.step(LR)
        s = e.sums.numpy().copy()
        if flavour == "ev":
            slot, info = mm.vis_stats(e.plan_f.vis_t.numpy(), np.float32(e.vis_t0))
            assert s[4] == slot and fm.same_bits(e._mon.info.numpy(), info)
        else:
            assert s[4] == 0.0
        mm.observe(cfg, st, ring, s[0:8], s[8:16], None, None, 10.0, 0.0, 1.0, 0.1, 70, 33, 0, 0, RE)
        assert fm.same_bits(e._mon.state.numpy(), st) and fm.same_bits(e._mon.ring.numpy(), ring)
        row, lt = e.monitor_info()["last"], e.loss_terms()
        for k in ("loss", "loss_e", "loss_b"):
            assert abs(row[k] - float(lt[k])) <= 4 * 2.0 ** -24 * abs(row[k]), k
    names = [c[0] for c in monitor_fakes.CALLS if c[0].startswith("monitor")]
    assert names == (["monitor_vis_stats", "monitor_observe"] if flavour == "ev" else ["monitor_observe"]) * 5
    hist = e.monitor_history()
    assert list(hist[:, 0]) == [1.0, 2.0, 3.0, 4.0, 5.0] and e.monitor_info()["updates"] == 5
    if flavour == "ev":
        assert hist[-1, 10] == 1.0 / (1.0 / RE + hist[-1, 9]) and 0.0 < hist[-1, 10] <= RE
        assert 0.0 <= e.monitor_info()["cap_fraction"] <= 1.0
    e.reset_convergence_monitor()
    assert not e._mon.state.numpy().any() and not e._mon.ring.numpy().any() and e.monitor_info()["last"] is None


def test_off_adds_no_launch_and_lbfgs_does_not_observe(monkeypatch):
    import monitor_fakes
    case = _case()
    e = _engine(monkeypatch, case, "ev")
    del monitor_fakes.CALLS[:]
    e.step(LR)
    off = list(monitor_fakes.CALLS)
    assert not [c for c in off if c[0].startswith("monitor")] and e.monitor_info() is None and e.should_stop() is False
    with pytest.raises(RuntimeError, match="monitor is off"):
        e.monitor_history()
    e.set_convergence_monitor(window=2)
    e.set_convergence_monitor(every=0)
    del monitor_fakes.CALLS[:]
    e.step(LR)
    assert [c[0] for c in monitor_fakes.CALLS] == [c[0] for c in off]
    e.set_convergence_monitor(window=2)
    e.step(LR)
    e.lbfgs_step(max_iter=2)
    assert e.monitor_info()["updates"] == 1


def test_refusals_name_what_is_missing(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    with pytest.raises(ValueError, match="re_eff_tol needs the ev flavour"):
        e.set_convergence_monitor(re_eff_tol=1e-3)
    for kw in (dict(window=0), dict(patience=0), dict(history=0), dict(min_updates=-1), dict(every=-1),
               dict(min_rel_improvement=-1.0), dict(min_rel_improvement=float("nan")), dict(quantity="loss_s"),
               dict(mode="some")):
        with pytest.raises(ValueError, match="convergence monitor"):
            e.set_convergence_monitor(**kw)
    assert e.monitor_info() is None
    e.set_convergence_monitor(window=2)
    with pytest.raises(ValueError, match="convergence monitor needs the MSE loss"):
        e.loss_and_grad(mode="L2")
    with pytest.raises(ValueError, match="convergence monitor needs a resident store"):
        e.set_collocation(case["x"], case["y"], chunk_points=32)
    e.set_convergence_monitor(every=0)
    e.set_collocation(case["x"], case["y"], chunk_points=32)
    with pytest.raises(ValueError, match="convergence monitor needs a resident store"):
        e.set_convergence_monitor(window=2)


def test_mode_combines_the_criteria_on_the_host(monkeypatch):
    e = _engine(monkeypatch, _case(), "ev")
    for mode, code, want in (("any", 1, True), ("any", 2, True), ("all", 1, False), ("all", 3, True), ("all", 4, True),
                             ("any", 0, False)):
        e.set_convergence_monitor(window=2, re_eff_tol=0.1, mode=mode)
        e._mon.state[11] = float(code)
        assert e.should_stop() is want, (mode, code)
        assert e.monitor_info()["should_stop"] is want
    e.set_convergence_monitor(window=2, re_eff_tol=None, mode="all")
    e._mon.state[11] = 1.0
    assert e.should_stop() and e.monitor_info()["reasons"] == ["plateau"]


def test_graph_key_carries_the_launch_constants(monkeypatch):
    e = _engine(monkeypatch, _case())
    off = e._graph_key(LR, False)
    e.set_convergence_monitor(window=7, patience=2)
    on = e._graph_key(LR, False)
    assert on != off and on[:len(off)] == off
    e.set_convergence_monitor(window=8, patience=2)
    assert e._graph_key(LR, False) != on
    e.set_convergence_monitor(every=0)
    assert e._graph_key(LR, False) == off


@pytest.mark.parametrize("kind", ["plain", "ev"])
def test_a_stage_ends_at_the_first_log_point_after_the_bit(monkeypatch, kind):
    case = _case()
    P = _plain(monkeypatch, case) if kind == "plain" else _ev(monkeypatch, case)
    P.set_early_stopping(window=2, patience=1, min_rel_improvement=1e-3)
    if kind == "plain":
        P.log_every = 5          # log points: epochs 0, 5, 10, ...
    else:
        P.log_interval = 6       # log points: epochs 0, 5, 11, ...
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=40, lr=0.0)                       # lr = 0: the loss is constant, update 4 sets the bit
    info = P.engine.monitor_info()
    assert info["t_plateau"] == 4 and info["reasons"] == ["plateau"] and info["updates"] == 6
    text = out.getvalue()
    assert "early stop after epoch 6: plateau (set by update 4)" in text and "early stop (t=6): loss window mean=" in text
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=3, lr=0.0)                        # a stage start resets the monitor
    assert P.engine.monitor_info()["updates"] == 3 and not P.engine.should_stop()
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=5, lr=0.0, start_epoch=3)         # a resumed stage does not
    assert P.engine.monitor_info()["updates"] == 5
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=1)
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=2, lr=1.0, optimizer=opt)         # solve_LBFGS neither observes nor asks
    assert P.engine.monitor_info()["updates"] == 5
    P.set_early_stopping(every=0)
    assert not P._early_stop and P.engine.monitor_info() is None


# ------------------------------------------------------------------ YAML and the script
def _config_module():
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_mon", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_yaml_key_parses_and_is_validated(tmp_path):
    cfg = _config_module()
    prod = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                    "production.yaml"))
    assert prod.config.training.early_stop is None                  # absent: off
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  early_stop: {window: 500, min_rel_improvement: 0.01, patience: 4, re_eff_tol: 0.002, "
                 "min_updates: 20000, quantity: loss_e, mode: all, every: 2}\n")
    es = cfg.ConfigManager.from_file(str(p)).config.training.early_stop
    assert (es.window, es.min_rel_improvement, es.patience, es.re_eff_tol, es.min_updates, es.quantity, es.mode,
            es.every) == (500, 0.01, 4, 0.002, 20000, "loss_e", "all", 2)
    p.write_text("training:\n  early_stop: {window: 500}\n")
    es = cfg.ConfigManager.from_file(str(p)).config.training.early_stop
    assert (es.window, es.min_rel_improvement, es.patience, es.re_eff_tol, es.mode) == (500, 1e-3, 3, None, "any")
    for bad in ("window: 0", "patience: 0", "every: 0", "min_updates: -1", "min_rel_improvement: -0.1", "re_eff_tol: .inf",
                "quantity: loss_s", "mode: some", "min_rel_improvement: null"):
        p.write_text("training:\n  early_stop: {%s}\n" % bad)
        with pytest.raises(ValueError, match="training.early_stop"):
            cfg.ConfigManager.from_file(str(p))
    p.write_text("training:\n  early_stop: null\n")
    assert cfg.ConfigManager.from_file(str(p)).config.training.early_stop is None
    out = io.StringIO()
    p.write_text("training:\n  early_stop: {window: 250, re_eff_tol: 0.01}\n")
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "early stop : window=250 min_rel_improvement=0.001 patience=3 re_eff_tol=0.01" in out.getvalue()


def test_converge_ev_wires_its_arguments(monkeypatch, tmp_path):
    """The script on the fakes, a 2 x 8 net and 40 points: 5 updates of stage 1 with windows of 2 give five rows of
    monitor.jsonl and the monitor's summary in the stage record."""
    import json
    import monitor_fakes
    monitor_fakes.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    spec = importlib.util.spec_from_file_location("converge_ev_mon", os.path.join(ROOT, "scripts", "converge_ev.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    dns = os.path.join(ROOT, "tests", "golden", "dns", "cavity_Re3000_256_Uniform.mat")
    out = tmp_path / "run"
    monkeypatch.setattr(sys, "argv", ["converge_ev.py", "--dns", dns, "--out", str(out), "--first", "1", "--last", "1",
                                      "--epochs-scale", "1e-5", "--nf", "40", "--layers", "2", "--hidden", "8",
                                      "--early-stop", "2", "1e-3", "--re-eff-tol", "1e-2"])
    cwd = os.getcwd()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mod.main()
    finally:
        os.chdir(cwd)
    rows = [json.loads(l) for l in open(out / "monitor.jsonl")]
    assert [r["t"] for r in rows] == [1.0, 2.0, 3.0, 4.0, 5.0] and all(r["stage"] == 1 for r in rows)
    assert all(0.0 < r["Re_eff"] <= 3000.0 and r["loss"] > 0 for r in rows)
    rec = json.loads(open(out / "stages.jsonl").readline())
    assert rec["early_stop"]["updates"] == 5 and isinstance(rec["early_stop"]["reasons"], list)


# ------------------------------------------------------------------ training-state files
FINGERPRINT_KEYS = ["attention", "balancing", "batch_points", "colloc_weights", "confgrad", "first_layer", "flavour",
                    "hard_bc", "lbfgs_history", "net", "net_e", "points_boundary", "points_colloc", "points_colloc_passes",
                    "points_pool", "points_supervised", "points_val", "pseudo_time", "rank", "rwf", "schedule_or_clipping",
                    "validation", "world_size"]
INFO_KEYS = ["Re", "alpha_b", "alpha_e", "alpha_evm", "alpha_s", "attention", "balancing", "batch_seed", "eq4_weight",
             "kernels", "max_norm", "precision", "pseudo_time", "scale", "schedule", "validation_every", "vis_t0"]


def test_a_state_file_with_the_monitor_off_has_the_bytes_of_before(monkeypatch, tmp_path):
    import state_model as sm
    case = _case()
    never = _engine(monkeypatch, case, "ev")
    toggled = _engine(monkeypatch, case, "ev")
    toggled.set_convergence_monitor(window=2, re_eff_tol=0.1)
    toggled.set_convergence_monitor(every=0)
    for e in (never, toggled):
        for _ in range(3):
            e.step(LR)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    never.save_training_state(a)
    toggled.save_training_state(b)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    header, _ = sm.parse(raw)
    # the header's keys are those of the format before the monitor existed, and no segment is the monitor's
    assert sorted(header["fingerprint"]) == FINGERPRINT_KEYS and sorted(header["info"]) == INFO_KEYS
    assert not [s for s in header["segments"] if s["name"].startswith("monitor")]
    on = _engine(monkeypatch, case, "ev", setup=lambda e: e.set_convergence_monitor(window=2, re_eff_tol=0.1, history=16))
    on.step(LR)
    c = str(tmp_path / "c.bin")
    on.save_training_state(c)
    header, _ = sm.parse(open(c, "rb").read())
    assert header["fingerprint"]["monitor"] == dict(capacity=16)
    assert header["info"]["monitor"] == [1, 2, 1e-3, 3, 0.1, 0, "loss", "any"]
    assert [s["name"] for s in header["segments"] if s["name"].startswith("monitor")] == ["monitor.state", "monitor.ring"]
    with pytest.raises(ValueError, match="fingerprint key 'monitor'"):
        never.load_training_state(c)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_k_save_load_k_equals_2k(monkeypatch, tmp_path, flavour):
    case, K = _case(), 5
    setup = lambda e: e.set_convergence_monitor(window=2, patience=1, re_eff_tol=0.3 if flavour == "ev" else None,
                                                history=6)
    whole = _engine(monkeypatch, case, flavour, setup=setup)
    for _ in range(2 * K):
        whole.step(LR)
    first = _engine(monkeypatch, case, flavour, setup=setup)
    for _ in range(K):
        first.step(LR)
    path = str(tmp_path / "s.bin")
    first.save_training_state(path)
    second = _engine(monkeypatch, case, flavour, seed=77, setup=setup)
    assert second.load_training_state(path)["changed"] == []
    assert fm.same_bits(second._mon.state.numpy(), first._mon.state.numpy())
    for _ in range(K):
        second.step(LR)
    assert whole.monitor_info()["updates"] == 2 * K
    assert fm.same_bits(second._mon.state.numpy(), whole._mon.state.numpy())
    assert fm.same_bits(second._mon.ring.numpy(), whole._mon.ring.numpy())
    assert fm.same_bits(second.monitor_history(), whole.monitor_history()) and whole.monitor_history().shape[0] == 6
    np.testing.assert_array_equal(second.net.params.numpy(), whole.net.params.numpy())


# ------------------------------------------------------------------ two gloo ranks
def _run_rank(rank, world, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        import monitor_fakes
        monitor_fakes.install(None)
        from nsfnet_amd import ev_pinn_solver as es
        torch.manual_seed(3)
        case = _case(N=71)                                  # 35 + 36 points: unequal vis_t shares
        P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=71,
                                           alpha_evm=0.05, bc_weight=10, eq_weight=1)
        P.set_boundary_data(X=(case["xb"].reshape(-1, 1), case["yb"].reshape(-1, 1), case["ub"].reshape(-1, 1),
                               case["vb"].reshape(-1, 1)))
        P.set_eq_training_data(X=(case["x"].reshape(-1, 1), case["y"].reshape(-1, 1)))
        assert P.is_distributed and P.engine.world_size == world
        P.log_interval = 4
        P.save = lambda *a, **k: None
        P.set_early_stopping(window=2, patience=1, min_rel_improvement=None, re_eff_tol=0.5)
        with contextlib.redirect_stdout(io.StringIO()):
            P.train(num_epoch=30, lr=1e-3)
        e = P.engine
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), state=e._mon.state.numpy(), ring=e._mon.ring.numpy(),
                 info=e._mon.info.numpy(), stop=np.array(e.should_stop()), n=np.array(e.plan_f.n),
                 params=e.net.params.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_hold_the_same_bits_and_take_the_same_decision(tmp_path):
    world = 2
    mp.spawn(_run_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    assert sorted((int(r0["n"]), int(r1["n"]))) == [35, 36]
    assert fm.same_bits(r0["state"], r1["state"]) and fm.same_bits(r0["ring"], r1["ring"])
    assert bool(r0["stop"]) and bool(r1["stop"])
    assert r0["state"][mm.S_UPDATES] < 30 and int(r0["state"][mm.S_STOP]) & mm.STOP_RE_EFF      # both left the stage early
    assert (r0["info"][3], r1["info"][3]) == (float(r0["n"]), float(r1["n"]))            # the info words are per rank
    k = int(r0["state"][mm.S_OBS]) - 1
    np.testing.assert_allclose(r0["ring"][k, 9], (r0["info"][2] + r1["info"][2]) / 71.0, rtol=1e-6)  # the global mean
    np.testing.assert_array_equal(r0["params"], r1["params"])
