"""Viscosity identification without a GPU: the formula d loss / d nu = -(2 alpha_e / N) S against a central difference
of the fp64 oracle's loss, the conditions on the inputs of the GPU rows (tests/test_viscosity_gpu.py), the numpy
statement of the update, the golden Kovasznay trajectory, and the engine's host logic on the model-backed fakes
(tests/visc_fakes.py): where the two launches sit in a step, the refusals, the graph key and the training-state file."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fold_model as fm  # noqa: E402
import visc_model as vm  # noqa: E402

# the bars of S in the GPU test: 3 x the `sums` bars of tests/test_tile_loops.py (3: the cancellation cap kappa <= 3)
S_BAR = {"fp32": 3e-5, "bf16x3": 6e-4}
L, H, RE, LR = 2, 10, 400.0, 1e-3
SHAPE_E = (1, 2, 6)


# ------------------------------------------------------------------ the formula and the rows' inputs
def _one_per_reference(names):
    """The first row of every fp64 reference (vm.ref_key): rows that differ by precision or switch share it."""
    seen, out = set(), []
    for name in names:
        if vm.ref_key(name) not in seen:
            seen.add(vm.ref_key(name))
            out.append(name)
    return out


# (the first three: the rows this test was written on; then one row of every other reference of the second set)
@pytest.mark.parametrize("name", _one_per_reference(["2x8-fp32", "4x50-fp32-ev", "4x50-bf16x3-hardbc"] + list(vm.ROWS)))
def test_the_formula_is_the_central_difference_of_the_oracle_loss(name):
    c = vm.row_case(name)
    nu = float(np.float32(1.0) / np.float32(c["Re"]))
    ev = {}
    if c.get("ev"):     # the lagged viscosity and e are inputs of the evaluation: held while nu moves
        ev = dict(vis_t=np.minimum(20.0 / c["Re"], vm.ALPHA_EVM * np.abs(_e(c))), e=_e(c))
    r = vm.row_reference(c, **ev)
    h = 1e-4 * nu
    kw = dict(w=c["w"], scale=c["scale"], **ev)
    if c.get("ff"):
        kw["ff"] = True
    if c.get("hard_bc"):
        import hardbc_model as hm
        kw["bc"] = hm.HardBc()
    lp = vm.evaluate(c["flat"], c["L"], c["H"], c["x"], c["y"], nu + h, **kw)["loss_e"]
    lm = vm.evaluate(c["flat"], c["L"], c["H"], c["x"], c["y"], nu - h, **kw)["loss_e"]
    fd = (lp - lm) / (2.0 * h)
    # the loss is quadratic in nu: the central difference is exact up to rounding, ~ eps loss / h
    assert abs(r["dnu"] - fd) <= 1e-6 * abs(fd) + 1e-9 * abs(r["loss_e"]) / h, (r["dnu"], fd)


def _e(c):
    from oracle import fwdmode_ref as fr
    Pe = fr.unflatten(c["flat_e"].astype(np.float64), 2, 1, *vm.EV_NET)
    return fr.forward1(Pe, c["x"].astype(np.float64), c["y"].astype(np.float64))[0][:, 0]


_REF = {}


def _ref(name, shifted=False):
    key = vm.ref_key(name) + (shifted,)
    if key not in _REF:
        c = vm.row_case(name)
        _REF[key] = vm.row_reference(c, re0=vm.row_re0(c, shifted))
    return _REF[key]


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", sorted(vm.ROWS))
def test_rows_are_not_dominated_by_cancellation(name, shifted):
    r = _ref(name, shifted)
    assert r["kappa"] <= 3.0, r["kappa"]
    assert np.isfinite(r["S"]) and r["S"] != 0.0
    if shifted:     # the shifted run tells the two viscosities apart: far beyond the bars of the planes and of S
        r0 = _ref(name)
        prec = vm.ROWS[name]["prec"]
        assert abs(r["S"] - r0["S"]) > 10.0 * S_BAR[prec] * abs(r["S"])
        assert np.abs(r["eqs"][0] - r0["eqs"][0]).max() > 10.0 * {"fp32": 2e-5, "bf16x3": 5e-4}[prec] * np.abs(r["eqs"][0]).max()
        g, g0 = r["grad"], r0["grad"]
        assert np.linalg.norm(g - g0) > 10.0 * 1e-4 * np.linalg.norm(g)


def test_the_ev_row_sees_eq4_and_the_weighted_row_its_weights_and_scale():
    name = "4x50-fp32-ev"
    c, r = vm.row_case(name), _ref(name)
    bar = S_BAR[c["prec"]] * abs(r["S"])
    no4 = float(np.sum(vm.terms(r["eqs"], r["u"], r["v"], r["lap"], c["w"], 0.0)))
    assert abs(r["S"] - no4) > 10.0 * bar, (r["S"], no4)
    no_w = float(np.sum(vm.terms(r["eqs"], r["u"], r["v"], r["lap"], None, 0.1)))
    assert abs(r["S"] - no_w) > 10.0 * bar, (r["S"], no_w)
    s2 = c["scale"] * c["scale"]
    no_sc2 = float(np.sum(vm.terms(r["eqs"], r["u"], r["v"], (r["lap"][0] / s2, r["lap"][1] / s2), c["w"], 0.1)))
    assert abs(r["S"] - no_sc2) > 10.0 * bar, (r["S"], no_sc2)


def test_the_bf16x3_ev_row_sees_eq4_its_weights_and_scale():
    name = "4x50-bf16x3-ev"
    c, r = vm.row_case(name), _ref(name)
    bar = S_BAR[c["prec"]] * abs(r["S"])
    s2 = c["scale"] * c["scale"]
    for what, lap, w, w4 in (("eq4", r["lap"], c["w"], 0.0), ("weights", r["lap"], None, 0.1),
                             ("scale", (r["lap"][0] / s2, r["lap"][1] / s2), c["w"], 0.1)):
        other = float(np.sum(vm.terms(r["eqs"], r["u"], r["v"], lap, w, w4)))
        assert abs(r["S"] - other) > 10.0 * bar, (what, r["S"], other)


# the bars of tests/test_viscosity_gpu.py per quantity: planes (lap, eq), S, sums, loss, gradient per block
ROW_BARS = {"fp32": dict(plane=2e-5, S=3e-5, sums=1e-5, loss=1e-5, grad=1e-4),
            "bf16x3": dict(plane=5e-4, S=6e-4, sums=2e-4, loss=1e-4, grad=1e-4)}


class _Cast(torch.nn.Module):
    """A model that rounds its input to `dtype`, computes in it and returns fp64 (tests/test_fourier_gpu.py model_step)."""

    def __init__(self, m, dtype):
        super().__init__()
        self.m, self.dtype = m, dtype

    def parameters(self, recurse=True):
        return self.m.parameters(recurse)

    def forward(self, X):
        return self.m(X.to(self.dtype)).double()


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", _one_per_reference([n for n in vm.ROWS if vm.ROWS[n].get("ff")]))
def test_sine_rows_keep_the_fp32_error_of_the_reference_within_a_quarter_of_each_bar(name, shifted):
    """The check of tests/test_fourier_gpu.py's docstring on the rows with the sine first layer: a straight fp32 torch
    evaluation of the row's model against the fp64 one - the fp32 rounding of the sine's argument, the reference's own
    error - stays within a quarter of every bar the GPU test applies to the row, at both estimates."""
    import fourier_model as fo
    import hardbc_model as hm
    from oracle import autograd_ref as ar
    from oracle import fwdmode_ref as fr
    c = vm.row_case(name)
    nu = float(np.float32(1.0) / np.float32(vm.row_re0(c, shifted)))
    xb, yb, ub, vb = (a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())
    run = {}
    for dtype in (torch.float64, torch.float32):
        model = fo.sine_net(c["flat"], c["L"], c["H"], dtype=dtype)
        r = hm.constrained_step(_Cast(model, dtype), c["x"], c["y"], 1.0 / nu, xb, yb, ub, vb, alpha_b=10.0, alpha_e=1.0)
        f = r["fields"]
        r["S"] = float(np.sum(vm.terms(r["eqs"], f["u"], f["v"], (f["u_d"], f["v_d"]))))
        r["grad"] = fo.freeze(r["grad"], c["H"])
        run[dtype] = r
    a, b = run[torch.float32], run[torch.float64]
    rel_max = lambda p, q: float(np.abs(p - q).max() / np.abs(q).max())
    blocks = lambda g: [q for wb in fr.unflatten(np.asarray(g, np.float64), 2, 3, c["L"], c["H"]) for q in wb]
    errs = dict(plane=max([rel_max(a["fields"][k], b["fields"][k]) for k in ("u_d", "v_d")] +
                          [rel_max(p, q) for p, q in zip(a["eqs"], b["eqs"])]),
                S=abs(a["S"] - b["S"]) / abs(b["S"]),
                sums=rel_max(np.asarray(a["sums_eq"]), np.asarray(b["sums_eq"])),
                loss=abs(a["loss"] - b["loss"]) / b["loss"],
                grad=max(float(np.linalg.norm(p - q) / max(np.linalg.norm(q), 1e-300))
                         for p, q in zip(blocks(a["grad"]), blocks(b["grad"]))))
    print("[viscosity] %s nu=%g fp32 torch against fp64: %s" % (name, nu, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k, bar in ROW_BARS[c["prec"]].items():
        assert errs[k] <= 0.25 * bar, (k, errs[k], bar)
    # (the autograd statement and the forward-mode one the GPU test uses are the same model)
    ref = _ref(name, shifted)
    assert rel_max(b["fields"]["u_d"], ref["lap"][0]) < 1e-9 and abs(b["S"] - ref["S"]) < 1e-9 * abs(ref["S"])


def test_the_two_estimates_of_the_lap_check_are_exact_and_a_factor_two_apart():
    a, b = (np.float32(1.0) / np.float32(r) for r in vm.TWO_RE0)
    assert a == 2.0 * b and float(a) * vm.TWO_RE0[0] == 1.0 and float(b) * vm.TWO_RE0[1] == 1.0
    assert np.frexp(a)[0] == 0.5 and np.frexp(b)[0] == 0.5                  # powers of two: nu Lap u is exact in fp32
    assert all(1e-2 <= r <= 1e6 for r in vm.TWO_RE0)                         # inside the default re_bounds
    assert all(n in vm.BIT_ROWS or not vm.ROWS[n].get("ev") for n in vm.LAP_ROWS)
    kinds = [dict(vm.BIT_ROWS, **vm.ROWS)[n] for n in vm.LAP_ROWS]
    assert any(k.get("hard_bc") for k in kinds) and any(k.get("ff") for k in kinds)


def test_the_pool_test_s_control_tells_the_two_viscosities_apart():
    """tests/test_viscosity_gpu.py judges the pool plan's eq1 plane against the model at 1 / re0: at 1 / Re the model is
    more than ten bars away, so a pool forward that kept the launch constant would miss."""
    c = vm.row_case("2x8-fp32", n=vm.N_OPT)
    xp, yp = vm.pool_points()
    at = lambda re: vm.evaluate(c["flat"], c["L"], c["H"], xp, yp, float(np.float32(1.0) / np.float32(re)))["eqs"][0]
    e0, e1 = at(c["Re"]), at(c["re0"])
    assert np.abs(e1 - e0).max() > 10.0 * ROW_BARS["fp32"]["plane"] * np.abs(e1).max()
    assert vm.B_OPT % 16 != 0 and vm.B_OPT < vm.N_OPT
    r = vm.evaluate(c["flat"], c["L"], c["H"], c["x"], c["y"], float(np.float32(1.0) / np.float32(c["re0"])))
    assert r["kappa"] <= 3.0, r["kappa"]


# ------------------------------------------------------------------ the rows' plans, from the ABI without a device
@pytest.mark.parametrize("name", list(vm.ROWS) + list(vm.BIT_ROWS))
def test_every_row_s_plan_names_its_kernels_and_says_its_path(monkeypatch, capfd, name):
    """resolve_plan is host arithmetic: the kernels a row's switches, width, precision and variant lead to, and the
    $PINN_VERBOSE line of its path, need no GPU (the GPU test asserts both again on the plan it runs)."""
    import ctypes
    from nsfnet_amd import _lib, engine as eng
    import hardbc_model as hm
    r = dict(vm.BIT_ROWS, **vm.ROWS)[name]
    for k in list(os.environ):
        if k.startswith("PINN_") or k.startswith("NSFNET_"):
            monkeypatch.delenv(k, raising=False)
    for k, v in r.get("env", ()):
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PINN_VERBOSE", "1")
    lib = _lib.load()
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pinn_net_create(3, r["L"], r["H"], ctypes.byref(net)) == 0
    try:
        assert lib.pinn_net_set_precision(net, *[eng.PRECISIONS[r["prec"]]] * 3) == 0
        if r.get("ff"):
            assert lib.pinn_net_set_first_layer(net, 1) == 0
        capfd.readouterr()
        if r.get("hard_bc"):
            bc = hm.HardBc().struct()
            assert lib.pinn_plan_create_constrained(net, vm.N_ROW, 4, ctypes.byref(bc), ctypes.byref(plan)) == 0
        else:
            assert lib.pinn_plan_create(net, vm.N_ROW, 4, ctypes.byref(plan)) == 0
        err = capfd.readouterr().err
        names = tuple((lib.pinn_plan_kernel(plan, k) or b"").decode() for k in (0, 1, 2))
        lib.pinn_plan_destroy(plan)
    finally:
        lib.pinn_net_destroy(net)
    assert names == r["names"], names
    for s in r.get("say", ()):
        assert any(s in line for line in err.splitlines() if line.startswith("[pinn] plan:")), (s, err)


# ------------------------------------------------------------------ the update
def test_update_model_is_adam_on_theta_and_a_bad_sum_only_counts():
    st, nu = vm.new_state(100.0)
    assert nu == np.float32(0.01) and np.float32(np.exp(st[0])) == nu
    p = torch.nn.Parameter(torch.tensor(st[0], dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1e-2)
    rng = np.random.RandomState(0)
    for _ in range(30):
        s = np.float32(rng.randn() * 3.0)
        nu_before = nu
        st, nu = vm.update(st, nu, s, -2.0 / 69, 1e-2)
        p.grad = torch.tensor(float(nu_before) * (-2.0 / 69) * float(s), dtype=torch.float64)
        opt.step()
        assert abs(st[0] - float(p.detach())) <= 1e-13 * abs(st[0])
    before = st.copy()
    for bad in (np.float32("nan"), np.float32("inf")):
        st, nu2 = vm.update(st, nu, bad, -2.0 / 69, 1e-2)
        assert nu2 == nu
    assert fm.same_bits(st[:7], before[:7]) and st[7] == 2.0 and st[5] == 30.0
    lo, hi = math.log(1.0 / 200.0), math.log(1.0 / 50.0)
    st, nu = vm.update(st, nu, np.float32(1e6), -1.0, 10.0, theta_min=lo, theta_max=hi)
    assert st[0] == hi
    st, nu = vm.update(st, nu, np.float32(-1e6), -1.0, 50.0, theta_min=lo, theta_max=hi)
    assert st[0] == lo and nu == np.float32(np.exp(lo))


def test_the_golden_trajectory_is_the_model_and_meets_its_condition():
    g = np.load(vm.GOLDEN)
    re, seed = g["re"], int(g["seed"])
    assert re.shape == (vm.KOV["updates"] // vm.KOV["every"],) and int(g["every"]) == vm.KOV["every"]
    assert abs(re[-1] - vm.KOV["Re"]) / vm.KOV["Re"] <= 0.025, re[-1]
    # the file is what the model gives (its first 100 updates, run again here)
    again = vm.kovasznay_model(vm.kovasznay_case(seed), updates=100)
    assert abs(again[0] - re[0]) <= 1e-9 * re[0], (again[0], re[0])
    u, v, p = vm.kovasznay(np.array([0.0, 0.3]), np.array([0.25, -0.1]))
    assert abs(u[0] - 1.0) < 1e-15 and abs(p[0]) < 1e-15      # cos(pi / 2) = 0, x = 0


# ------------------------------------------------------------------ the ABI without a device
def test_abi_refuses_bad_arguments_by_name():
    import ctypes
    from nsfnet_amd import _lib
    lib = _lib.load()
    assert lib.pinn_abi_version() == 3
    assert lib.pinn_visc_scratch_bytes(69) > 0 and lib.pinn_visc_scratch_bytes(0) == -1
    buf = (ctypes.c_double * 66)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)      # 16-byte aligned host memory: nothing is launched
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.pinn_visc_grad(0, p, 4, p, None, 0.0, p, p, None) == -22 and b"n must be" in lib.pinn_last_error()
    assert lib.pinn_visc_grad(5, p, 6, p, None, 0.0, p, p, None) == -22 and b"multiple of 4" in lib.pinn_last_error()
    assert lib.pinn_visc_grad(4, p, 4, odd, None, 0.0, p, p, None) == -22 and b"16-byte" in lib.pinn_last_error()
    assert lib.pinn_visc_grad(4, p, 4, p, None, -1.0, p, p, None) == -22 and b"w4" in lib.pinn_last_error()
    assert lib.pinn_visc_update(None, -1.0, 1e-2, 0.9, 0.999, 1e-8, -1.0, 1.0, p, p, None) == -22
    assert lib.pinn_visc_update(p, -1.0, 1e-2, 1.0, 0.999, 1e-8, -1.0, 1.0, p, p, None) == -22 and b"betas" in lib.pinn_last_error()
    assert lib.pinn_visc_update(p, -1.0, 1e-2, 0.9, 0.999, 1e-8, 1.0, -1.0, p, p, None) == -22 and b"theta_min" in lib.pinn_last_error()
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pinn_net_create(3, 2, 8, ctypes.byref(net)) == 0
    try:
        assert lib.pinn_plan_create(net, 69, 1, ctypes.byref(plan)) == 0
        assert lib.pinn_plan_set_viscosity(plan, p, None) == -22 and b"not a residual" in lib.pinn_last_error()
        lib.pinn_plan_destroy(plan)
        assert lib.pinn_plan_create(net, 69, 4, ctypes.byref(plan)) == 0
        assert lib.pinn_plan_set_viscosity(plan, ctypes.c_void_p(p.value + 2), None) == -22
        assert b"4-byte" in lib.pinn_last_error()
        assert lib.pinn_plan_set_viscosity(plan, p, odd) == -22 and b"16-byte" in lib.pinn_last_error()
        assert lib.pinn_plan_set_viscosity(plan, None, p) == -22 and b"lap comes with nu_dev" in lib.pinn_last_error()
        assert lib.pinn_plan_set_viscosity(plan, p, p) == 0
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        assert lib.pinn_plan_viscosity(plan, ctypes.byref(a), ctypes.byref(b)) == 0 and a.value == p.value == b.value
        assert lib.pinn_plan_set_viscosity(plan, None, None) == 0
        assert lib.pinn_plan_viscosity(plan, ctypes.byref(a), ctypes.byref(b)) == 0 and not a.value and not b.value
        lib.pinn_plan_destroy(plan)
    finally:
        lib.pinn_net_destroy(net)


# ------------------------------------------------------------------ the engine on the fakes
def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", seed=5, setup=None, attach=True):
    import visc_fakes
    visc_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=SHAPE_E[1], hidden_e=SHAPE_E[2], alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev)
    rng = np.random.RandomState(seed)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    if attach:
        e.set_collocation(case["x"], case["y"])
        e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    if setup is not None:
        setup(e)
    return e


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_engine_state_is_the_model_on_the_slot_and_the_slot_is_the_model_sum(monkeypatch, flavour):
    import visc_fakes
    e = _engine(monkeypatch, _case(), flavour)
    assert e.viscosity_info() is None
    e.set_viscosity_identification(re0=100.0, lr=1e-2)
    info = e.viscosity_info()
    assert info["updates"] == 0 and info["nu"] == float(np.float32(0.01)) and abs(info["Re"] - 100.0) < 1e-4
    st, nu = vm.new_state(100.0)
    del visc_fakes.CALLS[:]
    for i in range(5):
        e.step(LR)
        s = e.sums.numpy().copy()
        f = e.plan_f
        d = lambda t: t.numpy().astype(np.float64)
        eqs = [d(f.field("eq%d" % k)) for k in (1, 2, 3, 4)]
        t = vm.terms(eqs, d(f.field("u")), d(f.field("v")), (d(f.lap[0, :f.n]), d(f.lap[1, :f.n])), None,
                     0.1 if flavour == "ev" else 0.0)
        assert s[vm.SLOT] == np.float32(np.sum(t)) and s[vm.SLOT] != 0.0
        st, nu = vm.update(st, nu, s[vm.SLOT], -2.0 / 70, 1e-2, theta_min=math.log(1e-6), theta_max=math.log(1e2))
        assert fm.same_bits(e._visc.state.numpy(), st) and e._visc.nu.numpy()[0] == nu
    names = [c[0] for c in visc_fakes.CALLS if c[0].startswith("visc")]
    assert names == ["visc_grad", "visc_update"] * 5
    info = e.viscosity_info()
    assert info["updates"] == 5 and info["skipped"] == 0 and info["grad"] == st[6] and info["Re"] != 100.0
    # the plans evaluate at the estimate: the residual planes are those of the oracle at 1 / nu
    e.loss_and_grad()
    r = vm.evaluate(e.net.params.numpy(), L, H, _case()["x"], _case()["y"], float(nu)) if flavour == "nsfnet" else None
    if r is not None:
        np.testing.assert_allclose(e.plan_f.field("eq1").numpy(), r["eqs"][0], rtol=1e-5, atol=1e-6)


def test_held_by_lbfgs_and_full_batch_and_off_adds_no_launch(monkeypatch):
    import visc_fakes
    e = _engine(monkeypatch, _case())
    del visc_fakes.CALLS[:]
    e.step(LR)
    off = [c[0] for c in visc_fakes.CALLS]
    assert not [c for c in off if c.startswith("visc")]
    e.set_viscosity_identification(lr=1e-2)
    e.set_viscosity_identification(enabled=False)
    assert e.viscosity_info() is None and e.plan_f.nu is None and e.plan_f.lap is None
    del visc_fakes.CALLS[:]
    e.step(LR)
    assert [c[0] for c in visc_fakes.CALLS] == off
    e.set_viscosity_identification(lr=1e-2)
    e.step(LR)
    before = e._visc.state.numpy().copy()
    e.lbfgs_step(max_iter=2)
    e.loss_and_grad(full_batch=True)
    assert e.sums.numpy()[vm.SLOT] == 0.0
    e.adam_step(LR)
    assert fm.same_bits(e._visc.state.numpy(), before)


def test_every_residual_plan_gets_nu_and_the_evaluated_ones_lap(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, attach=False)
    e.set_viscosity_identification(re0=50.0)
    e.set_collocation(case["x"], case["y"])
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    e.set_batching(batch_points=35)
    e.set_resample_pool(case["x"][::-1].copy(), case["y"][::-1].copy())
    nu = e._visc.nu
    assert e.plan_f.nu is nu and e._batch.f.nu is nu and e._pool.nu is nu
    assert e.plan_f.lap is not None and e._batch.f.lap is not None and e._pool.lap is None
    e.step(LR)
    assert e.viscosity_info()["updates"] == 1
    e.set_collocation(case["x"], case["y"])
    assert e.plan_f.nu is nu and e._batch.f.nu is nu


def test_refusals_name_the_other_option(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    for kw in (dict(lr=-1.0), dict(eps=0.0), dict(betas=(1.0, 0.9)), dict(re_bounds=(0.0, 1.0)), dict(re0=1e9),
               dict(re0=float("nan"))):
        with pytest.raises(ValueError, match="viscosity identification"):
            e.set_viscosity_identification(**kw)
    assert e.viscosity_info() is None
    e.set_viscosity_identification()
    with pytest.raises(ValueError, match="convergence monitor is not available with viscosity identification"):
        e.set_convergence_monitor(window=2)
    with pytest.raises(ValueError, match="conflict-free gradients are not available with viscosity identification"):
        e.set_conflict_free_gradients()
    with pytest.raises(ValueError, match="viscosity identification needs the MSE loss"):
        e.loss_and_grad(mode="L2")
    with pytest.raises(ValueError, match="viscosity identification needs a resident store"):
        e.set_collocation(case["x"], case["y"], chunk_points=32)
    e.set_viscosity_identification(enabled=False)
    e.set_convergence_monitor(window=2)
    with pytest.raises(ValueError, match="not available with the convergence monitor"):
        e.set_viscosity_identification()
    e.set_convergence_monitor(every=0)
    e.set_conflict_free_gradients()
    with pytest.raises(ValueError, match="not available with conflict-free gradients"):
        e.set_viscosity_identification()
    e.set_conflict_free_gradients(False)
    e.set_collocation(case["x"], case["y"], chunk_points=32)
    with pytest.raises(ValueError, match="viscosity identification needs a resident store"):
        e.set_viscosity_identification()
    # pseudo-time stepping is set before the collocation points: both orders
    e2 = _engine(monkeypatch, case, attach=False)
    e2.set_pseudo_time(dtau=0.1, every=2)
    with pytest.raises(ValueError, match="not available with pseudo-time stepping"):
        e2.set_viscosity_identification()
    e3 = _engine(monkeypatch, case, attach=False)
    e3.set_viscosity_identification()
    with pytest.raises(ValueError, match="pseudo-time stepping is not available with viscosity identification"):
        e3.set_pseudo_time(dtau=0.1, every=2)


def test_graph_key_carries_the_launch_constants(monkeypatch):
    e = _engine(monkeypatch, _case())
    off = e._graph_key(LR, False)
    e.set_viscosity_identification(lr=1e-2)
    on = e._graph_key(LR, False)
    assert on != off and on[:len(off)] == off
    e.set_viscosity_identification(lr=2e-2)
    assert e._graph_key(LR, False) != on
    e.set_viscosity_identification(enabled=False)
    assert e._graph_key(LR, False) == off


def test_state_file_carries_fingerprints_and_omits_the_segment(monkeypatch, tmp_path):
    import state_model as sm
    case = _case()
    never = _engine(monkeypatch, case)
    toggled = _engine(monkeypatch, case)
    toggled.set_viscosity_identification(lr=1e-2)
    toggled.set_viscosity_identification(enabled=False)
    for e in (never, toggled):
        for _ in range(3):
            e.step(LR)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    never.save_training_state(a)
    toggled.save_training_state(b)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    header, _ = sm.parse(raw)
    assert "viscosity" not in header["fingerprint"] and "viscosity" not in header["info"]
    assert not [s for s in header["segments"] if s["name"].startswith("visc")]
    setup = lambda e: e.set_viscosity_identification(re0=100.0, lr=1e-2)
    K = 4
    whole = _engine(monkeypatch, case, setup=setup)
    for _ in range(2 * K):
        whole.step(LR)
    first = _engine(monkeypatch, case, setup=setup)
    for _ in range(K):
        first.step(LR)
    c = str(tmp_path / "c.bin")
    first.save_training_state(c)
    header, _ = sm.parse(open(c, "rb").read())
    assert header["fingerprint"]["viscosity"] is True
    assert header["info"]["viscosity"] == [100.0, 1e-2, [0.9, 0.999], 1e-8, [1e-2, 1e6]]
    assert [s["name"] for s in header["segments"] if s["name"].startswith("visc")] == ["visc.state", "visc.nu"]
    with pytest.raises(ValueError, match="fingerprint key 'viscosity'"):
        never.load_training_state(c)
    second = _engine(monkeypatch, case, seed=77, setup=setup)
    assert second.load_training_state(c)["changed"] == []
    assert fm.same_bits(second._visc.state.numpy(), first._visc.state.numpy())
    for _ in range(K):
        second.step(LR)
    assert fm.same_bits(second._visc.state.numpy(), whole._visc.state.numpy())
    assert second._visc.nu.numpy()[0] == whole._visc.nu.numpy()[0]
    np.testing.assert_array_equal(second.net.params.numpy(), whole.net.params.numpy())


# ------------------------------------------------------------------ the solvers, the YAML key
def _plain(monkeypatch, case):
    import visc_fakes
    visc_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=L, hidden_size=H, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_every, P.save_every = 2, 0
    return P


def _ev(monkeypatch, case):
    import visc_fakes
    visc_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(0)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=L, layers_1=SHAPE_E[1], hidden_size=H, hidden_size_1=SHAPE_E[2],
                                       N_f=70, alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_interval = 2
    return P


@pytest.mark.parametrize("kind", ["plain", "ev"])
def test_solvers_log_re_est_and_the_sidecar_round_trips(monkeypatch, tmp_path, kind):
    import contextlib
    import io
    case = _case()
    make = _plain if kind == "plain" else _ev
    P = make(monkeypatch, case)
    assert not P._identify
    P.set_viscosity_identification(re0=100.0, lr=1e-2)
    assert P._identify and P.Re != 100.0
    saved = P.save
    P.save = lambda *a, **k: None
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=4, lr=1e-3)
    assert "Re_est=" in out.getvalue() and "updates=" in out.getvalue() and P.engine.viscosity_info()["updates"] == 4
    if kind == "plain":        # the residuals a user inspects are those training minimises: at the identified viscosity
        nu = float(P.engine._visc.nu.numpy()[0])
        r = vm.evaluate(P.engine.net.params.numpy(), L, H, case["x"], case["y"], nu)
        eq1 = P.neural_net_equations(case["x"], case["y"])[0].numpy().reshape(-1)
        np.testing.assert_allclose(eq1, r["eqs"][0], rtol=1e-5, atol=1e-6)
        far = vm.evaluate(P.engine.net.params.numpy(), L, H, case["x"], case["y"], 1.0 / P.Re)
        assert np.abs(eq1 - far["eqs"][0]).max() > 1e-4
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=1)
    before = P.engine._visc.state.numpy().copy()
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=1, lr=1.0, optimizer=opt)            # held during an L-BFGS stage
    assert fm.same_bits(P.engine._visc.state.numpy(), before)
    P.save = saved
    P.save("net.pth", directory=str(tmp_path), N_HLayer=L, N_neu=H, N_f=70000, **(dict(lr=1e-3) if kind == "plain" else {}))
    side = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "net.pth_visc"]
    assert len(side) == 1
    Q = make(monkeypatch, case)
    Q.load(side[0][:-len("_visc")])
    assert Q._identify and fm.same_bits(Q.engine._visc.state.numpy(), before)
    assert Q.engine._visc.nu.numpy()[0] == P.engine._visc.nu.numpy()[0]
    i, j = P.engine.viscosity_info(), Q.engine.viscosity_info()
    assert (i["re0"], i["lr"], i["re_bounds"]) == (j["re0"], j["lr"], j["re_bounds"])
    P.set_viscosity_identification(enabled=False)
    assert not P._identify and P.engine.viscosity_info() is None


def test_yaml_key_parses_and_is_validated(tmp_path):
    import contextlib
    import importlib.util
    import io
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_visc", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    cfg = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = cfg
    spec.loader.exec_module(cfg)
    prod = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml"))
    assert prod.config.training.identify_viscosity is None         # absent: off
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  identify_viscosity: {re0: 10, lr: 0.02, re_min: 1, re_max: 5000}\n")
    iv = cfg.ConfigManager.from_file(str(p)).config.training.identify_viscosity
    assert (iv.re0, iv.lr, iv.re_min, iv.re_max) == (10.0, 0.02, 1.0, 5000.0)
    p.write_text("training:\n  identify_viscosity: {lr: 0.005}\n")
    iv = cfg.ConfigManager.from_file(str(p)).config.training.identify_viscosity
    assert (iv.re0, iv.lr, iv.re_min, iv.re_max) == (None, 0.005, 1e-2, 1e6)
    for bad in ("re_min: 0", "re0: 1.0e+9", "lr: -1", "re_min: 10, re_max: 1"):
        p.write_text("training:\n  identify_viscosity: {%s}\n" % bad)
        with pytest.raises(ValueError, match="training.identify_viscosity"):
            cfg.ConfigManager.from_file(str(p))
    p.write_text("training:\n  identify_viscosity: {re0: 10}\n  early_stop: {window: 500}\n")
    with pytest.raises(ValueError, match="does not go together with training.early_stop"):
        cfg.ConfigManager.from_file(str(p))
    p.write_text("training:\n  identify_viscosity: null\n")
    assert cfg.ConfigManager.from_file(str(p)).config.training.identify_viscosity is None
    out = io.StringIO()
    p.write_text("training:\n  identify_viscosity: {re0: 10}\n")
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "identify Re: re0=10.0 lr=0.01" in out.getvalue()


def test_with_attention_the_sum_takes_the_weights_the_sweep_read(monkeypatch):
    e = _engine(monkeypatch, _case())
    e.set_residual_attention(eta=0.5, gamma=0.9)
    e.set_viscosity_identification(lr=1e-2)
    e.step(LR)
    f = e.plan_f
    w_read = f.w.numpy().astype(np.float64).copy()
    e.loss_and_grad()
    assert not np.array_equal(f.w.numpy().astype(np.float64), w_read)      # rewritten for the next evaluation
    d = lambda t: t.numpy().astype(np.float64)
    eqs = [d(f.field("eq%d" % k)) for k in (1, 2, 3, 4)]
    t = vm.terms(eqs, d(f.field("u")), d(f.field("v")), (d(f.lap[0, :f.n]), d(f.lap[1, :f.n])), w_read, 0.0)
    assert e.sums.numpy()[vm.SLOT] == np.float32(np.sum(t))


# ------------------------------------------------------------------ two gloo ranks
def _run_rank(rank, world, out_dir):
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        import visc_fakes
        visc_fakes.install(None)
        from nsfnet_amd import ev_pinn_solver as es
        torch.manual_seed(3)
        case = _case(N=71)                                  # 35 + 36 points: unequal shares of S
        P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=71,
                                           alpha_evm=0.05, bc_weight=10, eq_weight=1)
        P.set_boundary_data(X=(case["xb"].reshape(-1, 1), case["yb"].reshape(-1, 1), case["ub"].reshape(-1, 1),
                               case["vb"].reshape(-1, 1)))
        P.set_eq_training_data(X=(case["x"].reshape(-1, 1), case["y"].reshape(-1, 1)))
        assert P.is_distributed and P.engine.world_size == world
        P.set_viscosity_identification(re0=100.0, lr=1e-2)
        e = P.engine
        slots, local = [], []
        for _ in range(4):
            e.step(1e-3)
            f = e.plan_f
            d = lambda t: t.numpy().astype(np.float64)
            eqs = [d(f.field("eq%d" % k)) for k in (1, 2, 3, 4)]
            t = vm.terms(eqs, d(f.field("u")), d(f.field("v")), (d(f.lap[0, :f.n]), d(f.lap[1, :f.n])), None, 0.1)
            local.append(float(np.float32(np.sum(t))))
            slots.append(float(e.sums.numpy()[vm.SLOT]))
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), state=e._visc.state.numpy(), nu=e._visc.nu.numpy(),
                 slots=np.array(slots), local=np.array(local), n=np.array(e.plan_f.n), params=e.net.params.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_update_from_the_same_global_sum(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_run_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    assert sorted((int(r0["n"]), int(r1["n"]))) == [35, 36]
    assert fm.same_bits(r0["state"], r1["state"]) and r0["nu"][0] == r1["nu"][0] and r0["state"][5] == 4.0
    assert fm.same_bits(r0["slots"], r1["slots"])                                  # what both ranks read after the exchange
    np.testing.assert_array_equal(np.float32(r0["local"]) + np.float32(r1["local"]), np.float32(r0["slots"]))
    assert (r0["local"] != r1["local"]).all()
    np.testing.assert_array_equal(r0["params"], r1["params"])
    # the state is the model's on the global sum with the global count
    st, nu = vm.new_state(100.0)
    for s in r0["slots"]:
        st, nu = vm.update(st, nu, np.float32(s), -2.0 / 71, 1e-2, theta_min=math.log(1e-6), theta_max=math.log(1e2))
    assert fm.same_bits(r0["state"], st)
