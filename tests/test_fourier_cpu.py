"""The frozen Fourier-feature first layer without a GPU: the two fp64 statements of
tests/fourier_model.py against each other, the engine's initialisation, the C ABI on the device-less library (plans are
sized for 256 compute units there), and the solvers' sidecar and the training-state fingerprint on the CPU stand-ins."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import fourier_model as fm
from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr


# ---- 1. the two statements of the model agree ----
def test_fwdmode_statement_matches_autograd_fp64():
    """Fields, residual sums and the gradient to 1e-11 relative in fp64 (the bar of test_fwdmode_matches_autograd_fp64),
    3x16 net, 41 points, frequencies of sigma = 2."""
    L, H, N, Re, ab = 3, 16, 41, 100.0, 10.0
    rng = np.random.RandomState(3)
    flat = ar.flat_params(ar.seeded_net(3, L, H, seed=11)).numpy().astype(np.float64)
    flat = fm.with_first_layer(flat, H, 2.0 * rng.randn(H // 2, 2)).astype(np.float64)
    x, y = rng.rand(N), rng.rand(N)
    xb, yb, ub, vb = (a.reshape(-1)[::32].astype(np.float64) for a in ar.cavity_boundary())
    a = fm.step(fm.sine_net(flat, L, H), H, x, y, Re, xb, yb, ub, vb, alpha_b=ab, alpha_e=1.0)
    P = fr.unflatten(flat, 2, 3, L, H)
    r = fm.pde_loss_and_grad(P, x, y, Re, alpha_e=1.0, chunk=16)      # (in three passes)
    b = fm.bc_loss_and_grad(P, xb, yb, ub, vb, alpha_b=ab)
    rel = lambda got, ref: np.max(np.abs(np.asarray(got) - np.asarray(ref))) / np.max(np.abs(ref))
    out = r["out"]
    for name, got in (("u", out[:, 0, 0]), ("v", out[:, 1, 0]), ("p", out[:, 2, 0]), ("u_x", out[:, 0, 1]),
                      ("u_y", out[:, 0, 2]), ("v_x", out[:, 1, 1]), ("v_y", out[:, 1, 2]), ("p_x", out[:, 2, 1]),
                      ("p_y", out[:, 2, 2]), ("u_d", out[:, 0, 3]), ("v_d", out[:, 1, 3])):
        assert rel(got, a["fields"][name]) < 1e-11, name
    for k in range(3):
        assert rel(r["eqs"][k], a["eqs"][k]) < 1e-11
        assert abs(r["sums"][k] - a["sums_eq"][k]) < 1e-11 * abs(a["sums_eq"][k])
    assert rel(b["pred"], a["pred_b"]) < 1e-11
    assert abs(sum(b["sums"]) / len(xb) - a["loss_b"]) < 1e-11 * a["loss_b"]
    g = r["grad"] + b["grad"]
    assert np.linalg.norm(g - a["grad"]) < 1e-11 * np.linalg.norm(a["grad"])
    assert not g[:3 * H].any() and not a["grad"][:3 * H].any() and g[3 * H:].any()      # layer 0 is frozen in both


# ---- 2. initialisation ----
def _fake_engine(monkeypatch, L=3, H=16, **kw):
    import fourier_fakes
    fourier_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    e = eng.PinnEngine("cpu", L, H, 100.0, alpha_b=10.0, **kw)
    e.net.set_flat(torch.tensor(np.random.RandomState(1).randn(e.P) * 0.3, dtype=torch.float32))
    return e


def test_initialisation_writes_the_embedding_and_nothing_else(monkeypatch):
    H = 16
    e = _fake_engine(monkeypatch, H=H)
    before = e.net.params.clone()
    assert e.fourier_info() is None and e.net.first_layer == 0
    ts, ns = torch.get_rng_state().clone(), np.random.get_state()
    e.set_fourier_features(sigma=2.0, seed=7)
    assert torch.equal(torch.get_rng_state(), ts)                                # the global generators are untouched
    ns2 = np.random.get_state()
    assert ns[0] == ns2[0] and np.array_equal(ns[1], ns2[1]) and ns[2:] == ns2[2:]
    info = e.fourier_info()
    assert info["kind"] == "sine" and info["sigma"] == 2.0 and info["seed"] == 7 and e.net.first_layer == 1
    B = info["frequencies"]
    assert tuple(B.shape) == (H // 2, 2) and B.dtype == torch.float64
    gen = torch.Generator(device="cpu")
    gen.manual_seed(7)
    assert torch.equal(B, 2.0 * torch.randn(H // 2, 2, generator=gen, dtype=torch.float64))
    p = e.net.params
    W0, b0 = p[:2 * H].reshape(H, 2), p[2 * H:3 * H]
    want = (2.0 * math.pi * B).to(torch.float32)
    assert torch.equal(W0[0::2], want) and torch.equal(W0[1::2], want)           # rows 2k and 2k + 1: 2 pi B_k
    assert torch.equal(b0[0::2], torch.full((H // 2,), float(np.float32(math.pi / 2)))) and not b0[1::2].any()
    assert torch.equal(p[3 * H:], before[3 * H:])                                 # layers >= 1 bit for bit
    sd = e.net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in e.net.keys_and_shapes()]
    # two seeds differ, one seed repeats, every rank draws alike
    e2 = _fake_engine(monkeypatch, H=H)
    e2.set_fourier_features(sigma=2.0, seed=8)
    assert not torch.equal(e2.fourier_info()["frequencies"], B)
    e3 = _fake_engine(monkeypatch, H=H)
    e3.set_fourier_features(sigma=2.0, seed=7)
    assert torch.equal(e3.net.params, e.net.params)
    # frequencies= is honoured
    mine = np.arange(H, dtype=np.float64).reshape(H // 2, 2) / 7.0
    e4 = _fake_engine(monkeypatch, H=H)
    e4.set_fourier_features(frequencies=mine)
    w0, b0 = fm.first_layer(mine)
    assert np.array_equal(e4.net.params[:2 * H].numpy().reshape(H, 2), w0) and np.array_equal(e4.net.params[2 * H:3 * H].numpy(), b0)
    assert e4.fourier_info()["sigma"] is None and np.array_equal(e4.fourier_info()["frequencies"].numpy(), mine)
    # off again: the kind goes back, the weights stay
    e4.set_fourier_features(sigma=None)
    assert e4.fourier_info() is None and e4.net.first_layer == 0


def test_engine_checks_its_arguments_and_the_order_of_calls(monkeypatch):
    e = _fake_engine(monkeypatch, H=16)
    for kw, text in ((dict(sigma=0.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                     (dict(frequencies=np.zeros((3, 2))), "shape"), (dict(frequencies=np.full((8, 2), np.inf)), "finite")):
        with pytest.raises(ValueError, match=text):
            e.set_fourier_features(**kw)
        assert e.fourier_info() is None and e.net.first_layer == 0
    with pytest.raises(ValueError, match="even"):
        _fake_engine(monkeypatch, H=15).set_fourier_features()
    with pytest.raises(ValueError, match="2 hidden layers"):
        _fake_engine(monkeypatch, L=1).set_fourier_features()
    xb, yb, ub, vb = (a.reshape(-1)[::64] for a in ar.cavity_boundary())
    e.set_boundary(xb, yb, ub, vb)
    with pytest.raises(ValueError, match="before any point set"):
        e.set_fourier_features()
    # the entropy net of the ev flavour keeps tanh
    ev = _fake_engine(monkeypatch, flavour="ev", n_hidden_e=2, hidden_e=8, alpha_evm=0.05)
    ev.set_fourier_features()
    assert ev.net.first_layer == 1 and ev.net_e.first_layer == 0


# ---- 3. the C ABI, on the device-less library ----
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def _net(lib, n_out, L, H, prec=(0, 0, 0), kind=None):
    from nsfnet_amd import _lib
    h = ctypes.c_void_p()
    _lib.check(lib.pinn_net_create(n_out, L, H, ctypes.byref(h)), "pinn_net_create")
    _lib.check(lib.pinn_net_set_precision(h, *prec), "pinn_net_set_precision")
    if kind is not None:
        _lib.check(lib.pinn_net_set_first_layer(h, kind), "pinn_net_set_first_layer")
    return h


def _plan(lib, net, n, streams):
    h = ctypes.c_void_p()
    rc = lib.pinn_plan_create(net, n, streams, ctypes.byref(h))
    return rc, h, lib.pinn_last_error().decode()


def _names(lib, plan):
    return tuple((lib.pinn_plan_kernel(plan, k) or b"").decode() for k in range(3))


def test_abi_round_trips_the_kind_and_keeps_its_version(lib):
    assert lib.pinn_abi_version() == 3
    net = _net(lib, 3, 3, 16)
    assert lib.pinn_net_first_layer(net) == 0                         # tanh is the default
    assert lib.pinn_net_set_first_layer(net, 1) == 0 and lib.pinn_net_first_layer(net) == 1
    assert lib.pinn_net_set_first_layer(net, 0) == 0 and lib.pinn_net_first_layer(net) == 0
    for bad in (-1, 2):
        assert lib.pinn_net_set_first_layer(net, bad) != 0 and "kind" in lib.pinn_last_error().decode()
        assert lib.pinn_net_first_layer(net) == 0
    assert lib.pinn_net_first_layer(None) == -1
    lib.pinn_net_destroy(net)


def test_abi_refusals_name_their_reason(lib):
    from nsfnet_amd import _lib
    odd = _net(lib, 3, 3, 15)
    assert lib.pinn_net_set_first_layer(odd, 1) != 0 and "even" in lib.pinn_last_error().decode()
    assert lib.pinn_net_first_layer(odd) == 0
    shallow = _net(lib, 3, 1, 16)
    assert lib.pinn_net_set_first_layer(shallow, 1) != 0 and "2 hidden layers" in lib.pinn_last_error().decode()
    net = _net(lib, 3, 3, 16, kind=1)
    bc = _lib.HardBcStruct(1, 2, 0.0, 0.0, 1.0, 10.0)
    h = ctypes.c_void_p()
    for streams in (1, 4):
        assert lib.pinn_plan_create_constrained(net, 100, streams, ctypes.byref(bc), ctypes.byref(h)) != 0
        err = lib.pinn_last_error().decode()
        assert "frozen sine" in err and "hard-wall" in err, err
    assert lib.pinn_plan_create_pseudo_time(net, 100, None, ctypes.byref(h)) != 0
    err = lib.pinn_last_error().decode()
    assert "frozen sine" in err and "pseudo-time" in err, err
    # a plan created before a change of kind is refused at launch and in the gradient assembly, by name
    one = ctypes.c_void_p(256)     # never dereferenced: the refusal comes before any launch
    coef = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 0.0)
    rc, res, err = _plan(lib, net, 64, 4)
    assert rc == 0, err
    rc, val, err = _plan(lib, net, 64, 1)
    assert rc == 0, err
    assert lib.pinn_net_set_first_layer(net, 0) == 0
    calls = (lambda: lib.pinn_residual_forward(res, one, one, one, one, None, None, None, None, one, 100.0, 0.0, 0.0, 1.0, 0, None, None),
             lambda: lib.pinn_residual_backward(res, one, one, one, one, None, None, None, one, coef, 100.0, 1.0, None, None),
             lambda: lib.pinn_residual_forward_backward(res, one, one, one, one, None, None, None, None, one, coef, 100.0, 0.0,
                                                        0.0, 1.0, None, None, None),
             lambda: lib.pinn_value_forward(val, one, one, one, one, None, None, None, 0, None, None),
             lambda: lib.pinn_value_backward(val, one, one, one, one, None, None),
             lambda: lib.pinn_grad_reduce(net, 1, (ctypes.c_void_p * 1)(res), (ctypes.c_void_p * 1)(one), one, 0, None))
    for call in calls:
        assert call() != 0
        assert "first-layer kind changed" in lib.pinn_last_error().decode()
    # the net may be destroyed before its plans
    for h in (odd, shallow, net):
        lib.pinn_net_destroy(h)
    lib.pinn_plan_destroy(res); lib.pinn_plan_destroy(val)


@pytest.mark.parametrize("prec", [(0, 0, 0), (1, 1, 1)], ids=["fp32", "bf16x3"])
def test_plan_of_a_sine_net_runs_the_8_wave_families_and_stores_layer_0(lib, monkeypatch, capfd, prec):
    """6x256 under default switches: the names are the 8-wave kernels', and the layout stores layer 0 - the plan is, byte
    for byte, the one a tanh net gets under PINN_SCHED=0 PINN_WSPLIT=0 PINN_FUSE=0 PINN_S0_SKIP32=0, whose layout
    is SPILL_CLASSIC in every precision, while the tanh net's default plan is another one."""
    for k in ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_FUSE", "PINN_TILE_COLS", "PINN_S0_SKIP32",
              "PINN_VERBOSE"):
        monkeypatch.delenv(k, raising=False)
    n = 360000
    tanh, sine = _net(lib, 3, 6, 256, prec), _net(lib, 3, 6, 256, prec, kind=1)
    rc, plain, err = _plan(lib, tanh, n, 4)
    assert rc == 0, err
    rc, ff, err = _plan(lib, sine, n, 4)
    assert rc == 0, err
    want = ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel") if prec[0] else ("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel")
    assert _names(lib, ff) == want
    if prec[0]:     # (the default role-split pair has no slot for layer 0; fp32's SPILL_SKIP0 keeps the slot and leaves it unused)
        assert lib.pinn_plan_workspace_bytes(ff, 1) > lib.pinn_plan_workspace_bytes(plain, 1)
    monkeypatch.setenv("PINN_VERBOSE", "1")
    capfd.readouterr()
    rc, loud, err = _plan(lib, sine, n, 4)
    assert rc == 0, err
    said = capfd.readouterr().err
    assert "frozen sine first layer: 8-wave kernels, layer 0 stored" in said, said
    lib.pinn_plan_destroy(loud)
    monkeypatch.delenv("PINN_VERBOSE")
    for k in ("PINN_SCHED", "PINN_WSPLIT", "PINN_FUSE", "PINN_S0_SKIP32"):
        monkeypatch.setenv(k, "0")
    rc, classic, err = _plan(lib, tanh, n, 4)
    assert rc == 0, err
    assert _names(lib, classic) == want
    tile = 16 if not prec[0] else 32
    ntiles = (n + tile - 1) // tile
    for a, b in ((ff, classic),):
        assert lib.pinn_plan_workspace_bytes(a, 1) == lib.pinn_plan_workspace_bytes(b, 1)
        assert lib.pinn_plan_padded_points(a) == lib.pinn_plan_padded_points(b) == ntiles * tile
    # S and Z-bar of a layout that stores layer 0: L blocks of 256 x (4 x tile) floats per tile, twice, (+1 scratch tile)
    spill = 2 * (ntiles + 1) * 6 * 256 * 4 * tile * 4
    assert lib.pinn_plan_workspace_bytes(ff, 1) - lib.pinn_plan_workspace_bytes(ff, 0) >= spill
    # the switches do not move a sine net's plan
    for k, v in (("PINN_SCHED", "2"), ("PINN_WSPLIT", "1"), ("PINN_FUSE", "1"), ("PINN_S0_SKIP32", "1")):
        monkeypatch.setenv(k, v)
    rc, again, err = _plan(lib, sine, n, 4)
    assert rc == 0, err
    assert _names(lib, again) == want and lib.pinn_plan_workspace_bytes(again, 1) == lib.pinn_plan_workspace_bytes(ff, 1)
    for p in (plain, ff, classic, again):
        lib.pinn_plan_destroy(p)
    lib.pinn_net_destroy(tanh); lib.pinn_net_destroy(sine)


def test_wide_sine_net_steps_back_to_the_8_wave_wide_kernels(lib, monkeypatch):
    for k in ("PINN_SCHED", "PINN_WSPLIT", "PINN_FUSE", "PINN_TILE_COLS", "PINN_S0_SKIP32"):
        monkeypatch.delenv(k, raising=False)
    sine = _net(lib, 3, 3, 400, (1, 1, 1), kind=1)
    rc, ff, err = _plan(lib, sine, 5000, 4)
    assert rc == 0, err
    assert _names(lib, ff) == ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel")
    ntiles = (5000 + 15) // 16
    assert lib.pinn_plan_workspace_bytes(ff, 1) - lib.pinn_plan_workspace_bytes(ff, 0) >= 2 * (ntiles + 1) * 3 * 416 * 64 * 4
    lib.pinn_plan_destroy(ff); lib.pinn_net_destroy(sine)


# ---- 4. sidecar and fingerprint, on the CPU stand-ins ----
def _case():
    rng = np.random.RandomState(0)
    xb, yb, ub, vb = (a.reshape(-1)[::64] for a in ar.cavity_boundary())
    return dict(x=rng.rand(70), y=rng.rand(70), xb=xb, yb=yb, ub=ub, vb=vb)


def test_solvers_keep_a_sidecar(monkeypatch, tmp_path):
    import fourier_fakes
    fourier_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es, pinn_solver as ps
    monkeypatch.chdir(tmp_path)
    c = _case()

    def solver(ff=None):
        torch.manual_seed(1)
        P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=8, N_f=70, bc_weight=10, device="cpu")
        if ff:
            P.set_fourier_features(**ff)
        P.set_boundary_data(X=(c["xb"], c["yb"], c["ub"], c["vb"]))
        P.set_eq_training_data(X=(c["x"], c["y"]))
        return P

    A = solver()
    with pytest.raises(ValueError, match="before any point set"):
        A.set_fourier_features()
    A.save("off.pth", N_HLayer=2, N_neu=8, N_f=70)
    assert [f for _, _, fs in os.walk(str(tmp_path)) for f in fs] == ["off.pth"]       # no sidecar with the option off
    B = solver(dict(sigma=1.5, seed=3))
    assert B.net.first_layer == "sine" and A.net.first_layer == "tanh"
    B.save("on.pth", N_HLayer=2, N_neu=8, N_f=70)
    ck = [os.path.join(d, "on.pth") for d, _, fs in os.walk(str(tmp_path)) if "on.pth" in fs][0]
    assert torch.load(ck + "_fourier", map_location="cpu", weights_only=True) == dict(kind="sine", sigma=1.5, seed=3)
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    assert list(sd) == [k for k, _ in B.net.dev_net.keys_and_shapes()]                 # the reference's format
    fresh = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=8, N_f=70, bc_weight=10, device="cpu")
    fresh.load(ck)                                                                     # takes the sidecar up
    info = fresh.engine.fourier_info()
    assert (info["kind"], info["sigma"], info["seed"]) == ("sine", 1.5, 3) and fresh.net.first_layer == "sine"
    assert torch.equal(fresh.net.dev_net.params, B.net.dev_net.params)                 # the weights hold B, bit for bit
    np.testing.assert_allclose(info["frequencies"].numpy(), B.engine.fourier_info()["frequencies"].numpy(), rtol=1e-6)
    solver(dict(sigma=1.5, seed=3)).load(ck)                                           # an engine of the same kind: fine
    with pytest.raises(ValueError, match="Fourier-feature first layer"):               # plans of the other kind
        solver().load(ck)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=8, hidden_size_1=8, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_fourier_features(sigma=2.0)
    assert P.engine.fourier_info()["sigma"] == 2.0 and P.engine.net_e.first_layer == 0


def test_training_state_of_the_other_kind_is_refused_by_name(monkeypatch, tmp_path):
    import fourier_fakes
    fourier_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    c = _case()

    def engine(ff):
        e = eng.PinnEngine("cpu", 3, 16, 100.0, alpha_b=10.0)
        e.net.set_flat(torch.tensor(np.random.RandomState(1).randn(e.P) * 0.3, dtype=torch.float32))
        if ff:
            e.set_fourier_features(sigma=1.0, seed=0)
        e.set_collocation(c["x"], c["y"])
        e.set_boundary(c["xb"], c["yb"], c["ub"], c["vb"])
        return e

    paths = {}
    for ff in (False, True):
        e = engine(ff)
        assert e._state_fingerprint()["first_layer"] == ("sine" if ff else None)
        e.step(1e-3)
        paths[ff] = str(tmp_path / ("s%d.bin" % ff))
        e.save_training_state(paths[ff])
    for ff in (False, True):
        with pytest.raises(ValueError, match="fingerprint key 'first_layer'"):
            engine(ff).load_training_state(paths[not ff])
        assert engine(ff).load_training_state(paths[ff])["changed"] == []


# ---- the ev YAML and the convergence script ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yaml_key_is_absent_by_default_and_parses(tmp_path):
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_fourier", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    cfg = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = cfg
    spec.loader.exec_module(cfg)
    prod = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml")
    assert cfg.ConfigManager.from_file(prod).config.network.fourier_features is None
    p = tmp_path / "c.yaml"
    p.write_text("network:\n  fourier_features: {sigma: 2.0, seed: 5}\n")
    ff = cfg.ConfigManager.from_file(str(p)).config.network.fourier_features
    assert (ff.sigma, ff.seed) == (2.0, 5)
    p.write_text("network:\n  fourier_features: {sigma: 3}\n")
    ff = cfg.ConfigManager.from_file(str(p)).config.network.fourier_features
    assert (ff.sigma, ff.seed) == (3.0, 0)
    p.write_text("network:\n  fourier_features: {sigma: 0}\n")
    with pytest.raises(ValueError, match="fourier_features"):
        cfg.ConfigManager.from_file(str(p))


def test_scripts_carry_the_option():
    import subprocess
    import sys
    conv = open(os.path.join(ROOT, "scripts", "converge_ev.py")).read()
    assert '"--fourier"' in conv and conv.index("set_fourier_features") < conv.index("P.set_boundary_data")
    train = open(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "train.py")).read()
    assert train.index("set_fourier_features") < train.index("PINN.set_boundary_data")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "converge_ev.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--fourier" in r.stdout, r.stderr
