"""Hard wall conditions by an output transform, without a device: the fp64 model's two
statements of the transform agree, the ansatz reproduces the cavity's boundary data, the transposed map is the
transpose, the C ABI refuses bad descriptors and resolves a constrained plan onto the 8-wave kernel families, and the
engine / solver surfaces check their arguments."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hardbc_model as hm
from oracle import autograd_ref as ar

BCS = [hm.HardBc(), hm.HardBc(lift_power=1), hm.HardBc(lift_power=5, lid_sharpness=6.0),
       hm.HardBc(lift_power=3, origin=(-1.0, -1.0), inv_len=0.5)]


def _flat(L, H, seed):
    return ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().astype(np.float64)


def _points(bc, n, seed):
    rng = np.random.RandomState(seed)
    lo, hi = bc.x0, bc.x0 + 1.0 / bc.inv_len
    sx, sy = hm.special_points(lo, hi)
    return (np.concatenate([sx.astype(np.float64), lo + (hi - lo) * rng.rand(n)]),
            np.concatenate([sy.astype(np.float64), lo + (hi - lo) * rng.rand(n)]))


@pytest.mark.parametrize("bc", BCS, ids=lambda b: "m%d_r%g_x0%g" % (b.m, b.r, b.x0))
def test_closed_form_streams_agree_with_autograd_through_the_ansatz(bc):
    L, H = 3, 20
    model = hm.constrained_net(_flat(L, H, 7), L, H, bc)
    x, y = _points(bc, 40, 1)
    scale = 1.0 / bc.inv_len
    xt, yt = hm._col(x, True), hm._col(y, True)
    want = {k: v.detach().numpy().reshape(-1) for k, v in hm.physical_fields(model, xt, yt, scale).items()}
    net = {k: v.detach().numpy().reshape(-1) for k, v in hm.physical_fields(model.net, xt, yt, scale).items()}
    h = hm.point_factors(bc, x, y)
    for c, lift in (("u", True), ("v", False)):
        got = hm.transform_streams(h, net[c], net[c + "_x"], net[c + "_y"], net[c + "_d"], lift)
        for name, g in zip((c, c + "_x", c + "_y", c + "_d"), got):
            assert np.abs(g - want[name]).max() <= 1e-10 * max(np.abs(want[name]).max(), 1.0), name
    for name in ("p", "p_x", "p_y"):
        np.testing.assert_array_equal(net[name], want[name])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("m", [1, 2, 8])
def test_constrained_fields_equal_the_cavity_boundary_data(seed, m):
    L, H = 2, 16
    model = hm.constrained_net(3.0 * _flat(L, H, seed), L, H, hm.HardBc(lift_power=m))
    xb, yb, ub, vb = ar.cavity_boundary()
    with torch.no_grad():
        out = model(torch.cat((hm._col(xb), hm._col(yb)), dim=1)).numpy()
    assert np.abs(out[:, 0] - ub.reshape(-1)).max() <= 1e-12
    assert np.abs(out[:, 1] - vb.reshape(-1)).max() <= 1e-12
    # ... and in the [-1, 1] coordinates of the ev flavour's map
    model = hm.constrained_net(3.0 * _flat(L, H, seed), L, H, hm.HardBc(lift_power=m, origin=(-1.0, -1.0), inv_len=0.5))
    with torch.no_grad():
        out = model(torch.cat((hm._col(2.0 * xb - 1.0), hm._col(2.0 * yb - 1.0)), dim=1)).numpy()
    assert np.abs(out[:, 0] - ub.reshape(-1)).max() <= 1e-12
    assert np.abs(out[:, 1] - vb.reshape(-1)).max() <= 1e-12


@pytest.mark.parametrize("bc", BCS, ids=lambda b: "m%d_r%g_x0%g" % (b.m, b.r, b.x0))
def test_transposed_map_passes_the_dot_product_test(bc):
    x, y = _points(bc, 50, 3)
    h = hm.point_factors(bc, x, y)
    rng = np.random.RandomState(4)
    n = [rng.randn(x.size) for _ in range(4)]
    a = [rng.randn(x.size) for _ in range(4)]
    zero = {k: (np.zeros_like(v) if k.startswith("g") else v) for k, v in h.items()}     # the linear part
    An = hm.transform_streams(zero, *n, lift=True)
    Ata = hm.transpose_streams(h, *a)
    lhs, rhs = sum(np.dot(p, q) for p, q in zip(An, a)), sum(np.dot(p, q) for p, q in zip(n, Ata))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)


def test_gradient_of_the_model_vanishes_for_the_boundary_term_alone():
    L, H = 2, 12
    model = hm.constrained_net(_flat(L, H, 5), L, H, hm.HardBc())
    xb, yb, ub, vb = (a.reshape(-1)[::64] for a in ar.cavity_boundary())
    r = hm.constrained_step(model, [0.3], [0.6], 100.0, xb, yb, ub, vb, alpha_b=1.0, alpha_e=0.0)
    assert r["loss_b"] <= 1e-24 and not r["grad"].any()


# ---- the C ABI: plan creation works without a device ----
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def _net(lib, n_out, L, H, prec=(0, 0, 0)):
    from nsfnet_amd import _lib
    h = ctypes.c_void_p()
    _lib.check(lib.pinn_net_create(n_out, L, H, ctypes.byref(h)), "pinn_net_create")
    _lib.check(lib.pinn_net_set_precision(h, *prec), "pinn_net_set_precision")
    return h


def _create(lib, net, n, streams, bc):
    h = ctypes.c_void_p()
    rc = lib.pinn_plan_create_constrained(net, n, streams, None if bc is None else ctypes.byref(bc), ctypes.byref(h))
    return rc, h, lib.pinn_last_error().decode()


def _names(lib, plan):
    return tuple((lib.pinn_plan_kernel(plan, k) or b"").decode() for k in range(3))


def test_abi_keeps_its_version_and_exports_the_new_symbols(lib):
    assert lib.pinn_abi_version() == 3
    assert hasattr(lib, "pinn_plan_create_constrained") and hasattr(lib, "pinn_plan_hard_bc")


def test_abi_refuses_invalid_descriptors(lib):
    from nsfnet_amd import _lib
    net = _net(lib, 3, 2, 16)
    ok = lambda **kw: _lib.HardBcStruct(**dict(dict(kind=1, lift_power=2, x0=0.0, y0=0.0, inv_len=1.0, lid_sharpness=10.0), **kw))
    for bad, text in ((ok(lift_power=0), "lift_power"), (ok(lift_power=9), "lift_power"), (ok(kind=2), "kind"),
                      (ok(inv_len=0.0), "inv_len"), (ok(inv_len=-1.0), "inv_len"), (ok(x0=float("nan")), "finite"),
                      (ok(y0=float("inf")), "finite"), (ok(lid_sharpness=float("nan")), "finite"),
                      (ok(inv_len=float("inf")), "finite"), (ok(lid_sharpness=151.0), "lid_sharpness")):
        for streams in (1, 4):
            rc, _, err = _create(lib, net, 100, streams, bad)
            assert rc != 0 and text in err, (rc, err)
    net_e = _net(lib, 1, 2, 16)
    rc, _, err = _create(lib, net_e, 100, 1, ok())
    assert rc != 0 and "n_out" in err
    lib.pinn_net_destroy(net); lib.pinn_net_destroy(net_e)


def test_abi_round_trips_the_descriptor_and_null_or_kind_0_is_the_plain_plan(lib):
    from nsfnet_amd import _lib
    net = _net(lib, 3, 4, 50)
    bc = _lib.HardBcStruct(1, 3, -1.0, -1.0, 0.5, 7.5)
    rc, plan, err = _create(lib, net, 777, 4, bc)
    assert rc == 0, err
    got = _lib.HardBcStruct()
    assert lib.pinn_plan_hard_bc(plan, ctypes.byref(got)) == 0
    assert [getattr(got, f) for f, _ in got._fields_] == [1, 3, -1.0, -1.0, 0.5, 7.5]
    lib.pinn_plan_destroy(plan)
    plain = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 777, 4, ctypes.byref(plain)) == 0
    for none in (None, _lib.HardBcStruct(0, 0, 0.0, 0.0, 0.0, 0.0)):
        rc, plan, err = _create(lib, net, 777, 4, none)
        assert rc == 0, err
        assert lib.pinn_plan_hard_bc(plan, ctypes.byref(got)) == 0 and got.kind == 0
        assert _names(lib, plan) == _names(lib, plain)
        assert lib.pinn_plan_workspace_bytes(plan, 1) == lib.pinn_plan_workspace_bytes(plain, 1)
        lib.pinn_plan_destroy(plan)
    lib.pinn_plan_destroy(plain)
    lib.pinn_net_destroy(net)


def test_constrained_plan_runs_the_8_wave_families(lib, monkeypatch):
    from nsfnet_amd import _lib
    for k in ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_FUSE", "PINN_TILE_COLS"):
        monkeypatch.delenv(k, raising=False)
    bc = _lib.HardBcStruct(1, 2, 0.0, 0.0, 1.0, 10.0)
    net = _net(lib, 3, 6, 256, (1, 1, 1))
    rc, plan, err = _create(lib, net, 360000, 4, bc)
    assert rc == 0, err
    assert _names(lib, plan) == ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")
    plain = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 360000, 4, ctypes.byref(plain)) == 0
    assert _names(lib, plain) == ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
    # the same plan as the switches give an unconstrained one
    for k in ("PINN_SCHED", "PINN_WSPLIT", "PINN_FUSE"):
        monkeypatch.setenv(k, "0")
    off = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 360000, 4, ctypes.byref(off)) == 0
    assert _names(lib, off) == _names(lib, plan)
    assert lib.pinn_plan_workspace_bytes(off, 1) == lib.pinn_plan_workspace_bytes(plan, 1)
    assert lib.pinn_plan_padded_points(off) == lib.pinn_plan_padded_points(plan)
    for p in (plan, plain, off):
        lib.pinn_plan_destroy(p)
    lib.pinn_net_destroy(net)
    for k in ("PINN_SCHED", "PINN_WSPLIT", "PINN_FUSE"):
        monkeypatch.delenv(k, raising=False)
    # the wide role-split sweeps step back to the 8-wave wide kernels, too
    net = _net(lib, 3, 3, 400, (1, 1, 1))
    rc, plan, err = _create(lib, net, 5000, 4, bc)
    assert rc == 0, err
    assert _names(lib, plan) == ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel")
    plain = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 5000, 4, ctypes.byref(plain)) == 0
    assert _names(lib, plain)[:2] == ("fwd_wsplit_kernel", "bwd_wsplit_kernel")
    lib.pinn_plan_destroy(plan); lib.pinn_plan_destroy(plain); lib.pinn_net_destroy(net)


def test_residual_call_refuses_a_scale_that_does_not_undo_inv_len(lib):
    from nsfnet_amd import _lib
    net = _net(lib, 3, 2, 16)
    rc, plan, err = _create(lib, net, 64, 4, _lib.HardBcStruct(1, 2, -1.0, -1.0, 0.5, 10.0))
    assert rc == 0, err
    one = ctypes.c_void_p(256)     # never dereferenced: the refusal comes before any launch
    coef = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 0.0)
    rc = lib.pinn_residual_forward(plan, one, one, one, one, None, None, None, None, one, 100.0, 0.0, 0.0, 1.0, 0, None, None)
    assert rc != 0 and "coord_scale" in lib.pinn_last_error().decode()
    rc = lib.pinn_residual_backward(plan, one, one, one, one, None, None, None, one, coef, 100.0, 1.0, None, None)
    assert rc != 0 and "coord_scale" in lib.pinn_last_error().decode()
    rc = lib.pinn_residual_forward_backward(plan, one, one, one, one, None, None, None, None, one, coef, 100.0, 0.0, 0.0,
                                            2.000003, None, None, None)
    assert rc != 0 and "coord_scale" in lib.pinn_last_error().decode()
    lib.pinn_plan_destroy(plan); lib.pinn_net_destroy(net)


# ---- engine and solvers against the CPU stand-ins ----
def _case():
    rng = np.random.RandomState(0)
    xb, yb, ub, vb = (a.reshape(-1)[::64] for a in ar.cavity_boundary())
    return dict(x=rng.rand(70), y=rng.rand(70), xb=xb, yb=yb, ub=ub, vb=vb)


def test_engine_checks_its_arguments_and_the_order_of_calls(monkeypatch):
    import fakes
    fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    c = _case()
    E = eng.PinnEngine("cpu", 2, 8, 100.0)
    assert E.hard_boundary_info() is None and E.net.hard_bc is None
    for kw in (dict(lift_power=0), dict(lift_power=9), dict(lift_power=2.5), dict(inv_len=0.0), dict(inv_len=-1.0),
               dict(lid_sharpness=float("nan")), dict(lid_sharpness=200.0), dict(origin=(float("inf"), 0.0)),
               dict(inv_len=0.5)):
        with pytest.raises(ValueError, match="hard boundary"):
            E.set_hard_boundary(True, **kw)
        assert E.hard_boundary_info() is None
    E.set_hard_boundary(True, lift_power=3, lid_sharpness=8.0)
    assert E.hard_boundary_info() == dict(lift_power=3, lid_sharpness=8.0, origin=(0.0, 0.0), inv_len=1.0)
    bc = E.net.hard_bc
    assert (bc.kind, bc.lift_power, bc.x0, bc.y0, bc.inv_len, bc.lid_sharpness) == (1, 3, 0.0, 0.0, 1.0, 8.0)
    E.set_hard_boundary(False)
    assert E.hard_boundary_info() is None
    E.set_hard_boundary()
    assert E.hard_boundary_info()["lift_power"] == 2 and E.hard_boundary_info()["lid_sharpness"] == 10.0
    E.set_boundary(c["xb"], c["yb"], c["ub"], c["vb"])
    for enabled in (True, False):
        with pytest.raises(ValueError, match="before any point set"):
            E.set_hard_boundary(enabled)
    E2 = eng.PinnEngine("cpu", 2, 8, 100.0)
    E2.set_collocation(c["x"], c["y"])
    with pytest.raises(ValueError, match="before any point set"):
        E2.set_hard_boundary()
    # the ev flavour: the coordinate map's descriptor, and the entropy net is never constrained
    Ev = eng.PinnEngine("cpu", 2, 8, 100.0, flavour="ev", n_hidden_e=2, hidden_e=8, alpha_evm=0.05, coord_scale=2.0)
    with pytest.raises(ValueError, match="coord_scale"):
        Ev.set_hard_boundary()
    Ev.set_hard_boundary(origin=(-1.0, -1.0), inv_len=0.5)
    assert Ev.net.hard_bc is not None and Ev.net_e.hard_bc is None


def test_plans_of_a_constrained_net_are_created_constrained(lib):
    """PointPlan takes the descriptor from its net: the C plan carries it (no device is needed to create a plan)."""
    from nsfnet_amd import engine as eng

    class Net:      # what PointPlan reads of a DeviceNet
        def __init__(self, lib, handle, bc):
            self.lib, self.handle, self.hard_bc, self.device = lib, handle, bc, torch.device("cpu")

    h = _net(lib, 3, 2, 16)
    bc = hm.HardBc(lift_power=4, lid_sharpness=9.0).struct()
    plan = eng.PointPlan(Net(lib, h, bc), [0.1, 0.2], [0.3, 0.4], 4, with_backward=False)
    assert plan.hard_bc() == dict(kind=1, lift_power=4, x0=0.0, y0=0.0, inv_len=1.0, lid_sharpness=9.0)
    plan = eng.PointPlan(Net(lib, h, None), [0.1, 0.2], [0.3, 0.4], 1, with_backward=False)
    assert plan.hard_bc() is None
    del plan
    lib.pinn_net_destroy(h)


def test_solvers_pass_the_coordinate_map_and_keep_a_sidecar(monkeypatch, tmp_path):
    import fakes
    fakes.install(monkeypatch)
    from nsfnet_amd import cavity_data, ev_pinn_solver as es, pinn_solver as ps
    monkeypatch.chdir(tmp_path)
    c = _case()

    def solver(constrain=None):
        torch.manual_seed(1)
        P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=8, N_f=70, bc_weight=10, device="cpu")
        if constrain:
            P.set_hard_boundary_constraints(**constrain)
        P.set_boundary_data(X=(c["xb"], c["yb"], c["ub"], c["vb"]))
        P.set_eq_training_data(X=(c["x"], c["y"]))
        return P

    A = solver()
    with pytest.raises(ValueError, match="before any point set"):
        A.set_hard_boundary_constraints()
    A.save("off.pth", N_HLayer=2, N_neu=8, N_f=70)
    assert [f for _, _, fs in os.walk(str(tmp_path)) for f in fs] == ["off.pth"]       # no sidecar with the feature off
    B = solver(dict(lift_power=3))
    info = dict(lift_power=3, lid_sharpness=10.0, origin=(0.0, 0.0), inv_len=1.0)
    assert B.engine.hard_boundary_info() == info
    B.save("on.pth", N_HLayer=2, N_neu=8, N_f=70)
    ck = [os.path.join(d, "on.pth") for d, _, fs in os.walk(str(tmp_path)) if "on.pth" in fs][0]
    assert torch.load(ck + "_hardbc", map_location="cpu", weights_only=True) == info
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    assert list(sd) == [k for k, _ in B.net.dev_net.keys_and_shapes()]                 # the reference's format
    fresh = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=8, N_f=70, bc_weight=10, device="cpu")
    fresh.load(ck)                                                                     # takes the descriptor up
    assert fresh.engine.hard_boundary_info() == info
    solver(dict(lift_power=3)).load(ck)                                                # the same descriptor: fine
    for other in (solver(), solver(dict(lift_power=2))):                               # plans that contradict it
        with pytest.raises(ValueError, match="hard wall conditions"):
            other.load(ck)
    # the ev class takes origin and inv_len from the loader's coordinate map
    loader = cavity_data.DataLoader(N_f=70, N_b=10, coord_transform=True)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=8, hidden_size_1=8, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_coordinate_transform(loader.get_coord_scale())
    P.set_hard_boundary_constraints(dataloader=loader)
    assert P.engine.hard_boundary_info() == dict(lift_power=2, lid_sharpness=10.0, origin=(-1.0, -1.0), inv_len=0.5)
    Q = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=8, hidden_size_1=8, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    Q.set_coordinate_transform(2.0)
    Q.set_hard_boundary_constraints(lift_power=1)                                      # no loader: from the scale
    assert Q.engine.hard_boundary_info()["origin"] == (-1.0, -1.0)
    with pytest.raises(ValueError, match="coord_scale"):                               # a loader that contradicts the scale
        Q.set_hard_boundary_constraints(dataloader=cavity_data.DataLoader(N_f=70, N_b=10))


# ---- the ev YAML and the convergence script ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config_module():
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_hardbc", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_yaml_key_is_off_by_default_and_parses(tmp_path):
    import contextlib
    import io
    cfg = _config_module()
    prod = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml")
    hb = cfg.ConfigManager.from_file(prod).config.training.hard_boundary
    assert (hb.enabled, hb.lift_power) == (False, 2)
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  hard_boundary: {enabled: true, lift_power: 3}\n")
    hb = cfg.ConfigManager.from_file(str(p)).config.training.hard_boundary
    assert (hb.enabled, hb.lift_power) == (True, 3)
    p.write_text("training:\n  hard_boundary: {lift_power: 3}\n")
    assert not cfg.ConfigManager.from_file(str(p)).config.training.hard_boundary.enabled
    for bad in (0, 9):
        p.write_text("training:\n  hard_boundary: {enabled: true, lift_power: %d}\n" % bad)
        with pytest.raises(ValueError, match="hard_boundary"):
            cfg.ConfigManager.from_file(str(p))
    out = io.StringIO()
    p.write_text("training:\n  hard_boundary: {enabled: true}\n")
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "hard walls : lift_power=2" in out.getvalue()


def test_scripts_carry_the_option():
    import subprocess
    import sys
    conv = open(os.path.join(ROOT, "scripts", "converge_ev.py")).read()
    assert '"--hard-bc"' in conv and "set_hard_boundary_constraints(lift_power=a.hard_bc" in conv
    assert conv.index("set_hard_boundary_constraints") < conv.index("P.set_boundary_data")
    train = open(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "train.py")).read()
    assert train.index("set_hard_boundary_constraints") < train.index("PINN.set_boundary_data")
    for script, option in (("converge_ev.py", "--hard-bc"), ("profile_hardbc.py", "--lift-power")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True)
        assert r.returncode == 0 and option in r.stdout, r.stderr
