"""Viscosity identification on the GPU (csrc/visc.hip, the nu_dev / lap members of the residual plans,
PinnEngine.set_viscosity_identification) against the fp64 model of tests/visc_model.py:

  1. one evaluation per kernel family at N = 69 (a ragged last tile) with nu read from device memory, once with the
     estimate at the configured Re and once away from it (a sweep that keeps the launch constant fails): the Laplacian
     planes, S, the residual planes, the loss sums, the loss and the net gradient; and one row where a workgroup of the
     fused sweep takes a second pair of tiles
  2. pinn_visc_update alone on 20 synthetic sums, bit for bit against the numpy statement
  3. 20 eager engine updates with the nets held: state = model(slot) bit for bit, every S at its bar
  4. hipGraph replay = eager, bit for bit; identification with lr = 0 = training without it, bit for bit
  5. Kovasznay flow at Re = 40 from Re0 = 10: the estimate after 2000 updates
  6. every row without the entropy net, and plain bf16: the engine that reads nu = fp32(1 / re0) from the device against
     an engine configured at Re = re0 without the option - planes, sums, gradient and loss bit for bit
  7. the lap plane without a precision bar: two estimates with nu_a = 2 nu_b, both powers of two - (eq_b - eq_a) /
     (nu_a - nu_b) is the stored Laplacian up to the two roundings of eq, and lap is the same bits in both runs
  8. pinn_visc_grad alone on synthetic planes, bit for bit against fold_model.grid_fold: one block to the grid-stride
     repeat, every ragged tail of w, NaN behind n, one scratch for every launch
  9. the options that run with the scalar on: mini-batching (and its replay), residual attention, the resampling
     pool, loss balancing

Bars: the planes take the `eq` bars of tests/test_tile_loops.py relative to the plane's maximum; S takes 3 x its `sums`
bars (3: the cap on the cancellation ratio kappa of the rows, tests/test_viscosity_cpu.py); sums, loss and gradient keep
that file's bars."""
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
from oracle import autograd_ref as ar  # noqa: E402
from oracle import fwdmode_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

BARS = {"fp32": dict(eq=2e-5, sums=1e-5, loss=1e-5, grad=1e-4),          # tests/test_tile_loops.py
        "bf16x3": dict(eq=5e-4, sums=2e-4, loss=1e-4, grad=1e-4)}
S_BAR = {k: 3.0 * v["sums"] for k, v in BARS.items()}                     # 3e-5, 6e-4
SWITCHES = ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_TILE_COLS", "PINN_STAGGER", "PINN_FUSE",
            "PINN_S0_SKIP32", "NSFNET_CHUNK_POINTS", "NSFNET_GRAPH", "PINN_PTIME_SPLIT", "PINN_HBC_SPLIT", "PINN_FF_SPLIT",
            "PINN_VERBOSE")
DEV = "cuda:0"


def _rel_max(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def _block_rel_l2(a, b, n_out, L, H):
    blocks = lambda g: [q for wb in fr.unflatten(np.asarray(g, np.float64), 2, n_out, L, H) for q in wb]
    return max(_rel_l2(p, q) for p, q in zip(blocks(a), blocks(b)))


def _bc():
    return tuple(a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())


def _clean_env(monkeypatch, env=()):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PINN_VERBOSE", "1")     # every plan says its path on stderr (_attach reads it)
    for k, v in env:
        monkeypatch.setenv(k, v)


def _engine(c, Re=None, **kw):
    """The engine of a row's case, configured at the row's Re (or at Re), before any point set is attached."""
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=vm.EV_NET[0], hidden_e=vm.EV_NET[1], alpha_evm=vm.ALPHA_EVM) if c.get("ev") else {}
    E = eng.PinnEngine(torch.device(DEV), c["L"], c["H"], c["Re"] if Re is None else Re, alpha_b=10.0, alpha_e=1.0,
                       precision=c["prec"], coord_scale=c["scale"], **ev, **kw)
    E.net.set_flat(torch.tensor(c["flat"]))
    if c.get("ff"):
        E.set_fourier_features(frequencies=c["B"])
        assert torch.equal(E.net.params.cpu(), torch.tensor(c["flat"]))      # the same layer 0, bit for bit
    if c.get("ev"):
        E.net_e.set_flat(torch.tensor(c["flat_e"]))
        E.e_trainable = True
    if c.get("hard_bc"):
        E.set_hard_boundary()
    return E


def _attach(E, c, capfd=None):
    """The row's collocation and boundary points; the collocation plan names the row's kernels and, with capfd, its
    $PINN_VERBOSE lines say the row's path (the only proof where kernel_names() cannot tell two rows apart)."""
    if capfd is not None:
        capfd.readouterr()
    E.set_collocation(c["x"], c["y"], weights=c["w"])
    if capfd is not None:
        err = capfd.readouterr().err
        for s in c.get("say", ()):
            assert any(s in line for line in err.splitlines() if line.startswith("[pinn] plan:")), (s, err)
    E.set_boundary(*_bc())
    assert E.plan_f.kernel_names() == c["names"], E.plan_f.kernel_names()


# ------------------------------------------------------------------ 1. one evaluation per family
_REF = {}


@pytest.mark.parametrize("shifted", [False, True], ids=["re0=Re", "re0-away"])
@pytest.mark.parametrize("name", list(vm.ROWS))
def test_evaluation_matches_the_model(monkeypatch, capfd, name, shifted):
    """shifted: the estimate starts away from the configured Re, so a sweep that keeps the launch constant 1 / Re, in all
    or in some of its tiles, misses the model (tests/test_viscosity_cpu.py: by more than ten bars in S, eq1, the gradient)."""
    c = vm.row_case(name)
    re0 = vm.row_re0(c, shifted)
    _clean_env(monkeypatch, c.get("env", ()))
    E = _engine(c)
    E.set_viscosity_identification(re0=re0)
    _attach(E, c, capfd)
    xb, yb, ub, vb = _bc()
    f = E.plan_f
    nu32 = np.float32(1.0) / np.float32(re0)
    assert E._visc.nu.cpu().numpy()[0] == nu32 and E.viscosity_info()["nu"] == float(nu32)
    vtm0 = f.vis_t_minus.cpu().numpy().astype(np.float64) if c.get("ev") else None
    f.lap.fill_(float("nan"))
    E.loss_and_grad()
    torch.cuda.synchronize()
    assert E._visc.nu.cpu().numpy()[0] == nu32
    n, prec, bar = f.n, c["prec"], BARS[c["prec"]]
    lap = f.lap.cpu().numpy().astype(np.float64)
    assert np.isfinite(lap).all(), "a padded or real entry of lap was not written"
    # the reference: one per (net, points, Re, re0) - rows that differ by precision or switch share theirs (an ev row
    # keeps its own: it takes the lagged viscosity its device run read)
    key = vm.ref_key(name) + (shifted, name if c.get("ev") else "")
    if key not in _REF:
        vis_t = None if vtm0 is None else np.minimum(np.float32(20.0 / c["Re"]), vtm0)
        r = vm.row_reference(c, vis_t=vis_t, re0=re0)
        P = fr.unflatten(c["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
        if c.get("hard_bc"):
            import hardbc_model as hm
            b = hm.constrained_value(P, hm.HardBc(), xb, yb, targets=[ub, vb, None], coef=[20.0 / xb.size] * 2 + [0.0])
        elif c.get("ff"):
            import fourier_model as fo
            b = fo.bc_loss_and_grad(P, xb.astype(np.float64), yb.astype(np.float64), ub, vb, alpha_b=10.0)
            b["grad"] = fo.freeze(b["grad"], c["H"])
        else:
            b = fr.bc_loss_and_grad(P, xb.astype(np.float64), yb.astype(np.float64), ub, vb, alpha_b=10.0)
        _REF[key] = (r, b)
    r, b = _REF[key]
    nq = len(r["eqs"])
    sums = E.sums.cpu().numpy().astype(np.float64)
    errs = dict(lap_u=_rel_max(lap[0, :n], r["lap"][0]), lap_v=_rel_max(lap[1, :n], r["lap"][1]))
    for k in range(nq):
        errs["eq%d" % (k + 1)] = _rel_max(f.field("eq%d" % (k + 1)).cpu().numpy(), r["eqs"][k])
    errs["S"] = abs(sums[vm.SLOT] - r["S"]) / abs(r["S"])
    errs["sums"] = _rel_max(sums[:nq], np.asarray(r["sums"]))
    ref_loss = 10.0 * (b["sums"][0] + b["sums"][1]) / xb.size + r["loss_e"]
    errs["loss"] = abs(float(E.loss_terms()["loss"]) - ref_loss) / ref_loss
    errs["grad"] = _block_rel_l2(E.grads.cpu().numpy(), r["grad"] + b["grad"], 3, c["L"], c["H"])
    print("[viscosity] %s re0=%g N=%d kappa %.2f: %s" % (name, re0, n, r["kappa"], " ".join("%s %.2e" % kv for kv in errs.items())))
    for k in errs:
        limit = S_BAR[prec] if k == "S" else bar["eq"] if k.startswith(("lap", "eq")) else bar[k]
        assert errs[k] <= limit, (k, errs[k], limit)


def test_a_workgroup_s_second_tiles_index_lap_off_its_first(monkeypatch):
    """The fused hidden-256 sweep at 2 x CUs + 1 tiles of 32 points: one workgroup takes a second pair."""
    _clean_env(monkeypatch)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = vm.row_case("6x256-bf16x3-fused", n=2 * cus * 32 + 5)
    E = _engine(c)
    re0 = vm.row_re0(c, True)
    E.set_viscosity_identification(re0=re0)
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(*_bc())
    f = E.plan_f
    assert f.kernel_names() == c["names"] and f.npad == (2 * cus + 1) * 32
    f.lap.fill_(float("nan"))
    E.loss_and_grad()
    torch.cuda.synchronize()
    lap = f.lap.cpu().numpy().astype(np.float64)
    assert np.isfinite(lap).all()
    r = vm.row_reference(c, want_grad=False, re0=re0)
    bar = BARS["bf16x3"]["eq"]
    assert r["kappa"] <= 3.0, r["kappa"]
    errs = dict(lap_u=_rel_max(lap[0, :f.n], r["lap"][0]), lap_v=_rel_max(lap[1, :f.n], r["lap"][1]),
                S=abs(float(E.sums[vm.SLOT]) - r["S"]) / abs(r["S"]))
    # per tile, too: a tile written at another tile's place moves that tile's error to order one
    tiles = np.abs(lap[0, :f.n] - r["lap"][0])[:f.n // 32 * 32].reshape(-1, 32).max(axis=1) / np.abs(r["lap"][0]).max()
    print("[viscosity] second tiles N=%d kappa %.2f: %s worst tile %d" % (f.n, r["kappa"],
          " ".join("%s %.2e" % kv for kv in errs.items()), int(tiles.argmax())))
    assert errs["lap_u"] <= bar and errs["lap_v"] <= bar and tiles.max() <= bar
    assert errs["S"] <= S_BAR["bf16x3"], errs["S"]


# ------------------------------------------------------------------ 2. the update alone
def test_update_kernel_is_the_numpy_statement_bit_for_bit():
    from nsfnet_amd import engine as eng
    lo, hi = math.log(1.0 / 200.0), math.log(1.0 / 50.0)
    coef = -2.0 / 69
    # (sum, lr): both signs, zero, a run against each bound, one NaN and one inf
    seq = [(0.37, 1e-2), (-1.2, 1e-2), (0.0, 1e-2), (3.5e-3, 1e-2), (-4.0e2, 1e-2), (7.0, 1e-2), (float("nan"), 1e-2),
           (-2.5e4, 5.0), (-2.5e4, 5.0), (1.0e-7, 1e-2), (float("inf"), 1e-2), (3.0e4, 5.0), (3.0e4, 5.0), (3.0e4, 5.0),
           (-0.75, 1e-2), (0.11, 1e-3), (-9.0, 1e-3), (2.0e-2, 1e-2), (1.0, 0.0), (-1.0, 1e-2)]
    assert len(seq) == 20
    st, nu = vm.new_state(100.0)
    state = torch.tensor(st, dtype=torch.float64, device=DEV)
    nu_d = torch.tensor([float(nu)], dtype=torch.float32, device=DEV)
    s_d = torch.zeros(1, dtype=torch.float32, device=DEV)
    hits = set()
    for s, lr in seq:
        s_d.fill_(s)
        eng.visc_update(s_d, coef, lr, (0.9, 0.999), 1e-8, (lo, hi), state, nu_d)
        got_nu = np.float32(nu_d.cpu().numpy()[0])
        st, model_nu = vm.update(st, nu, np.float32(s), coef, lr, theta_min=lo, theta_max=hi)
        assert fm.same_bits(state.cpu().numpy(), st), (s, lr, state.cpu().numpy(), st)
        # the device's exp may differ from numpy's in the last bit of the double: at most one fp32 ulp after rounding
        assert abs(float(got_nu) - float(model_nu)) <= float(np.spacing(model_nu)), (got_nu, model_nu)
        nu = got_nu                      # the next chain rule reads what the device wrote
        hits |= {"lo"} if st[0] == lo else {"hi"} if st[0] == hi else set()
    assert hits == {"lo", "hi"} and st[7] == 2.0 and st[5] == 18.0


# ------------------------------------------------------------------ 3. the engine, nets held
def test_engine_updates_are_the_model_on_the_slot(monkeypatch):
    _clean_env(monkeypatch)
    c = vm.row_case("2x8-fp32")
    E = _engine(c)
    E.set_viscosity_identification(re0=c["Re"], lr=5e-2)
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(*_bc())
    p0 = E.net.params.clone()
    st, nu = vm.new_state(c["Re"])
    vs = E._visc
    for i in range(20):
        E.loss_and_grad()
        E.adam_step(0.0)
        slot = np.float32(E.sums[vm.SLOT].item())
        ref = vm.evaluate(c["flat"], c["L"], c["H"], c["x"], c["y"], float(nu))
        assert abs(float(slot) - ref["S"]) <= S_BAR["fp32"] * abs(ref["S"]), (i, slot, ref["S"])
        st, model_nu = vm.update(st, nu, slot, -2.0 / vm.N_ROW, 5e-2, theta_min=vs.theta_bounds[0],
                                 theta_max=vs.theta_bounds[1])
        assert fm.same_bits(vs.state.cpu().numpy(), st), i
        nu = np.float32(vs.nu.cpu().numpy()[0])
        assert abs(float(nu) - float(model_nu)) <= float(np.spacing(model_nu))
    assert torch.equal(E.net.params, p0)
    info = E.viscosity_info()
    assert info["updates"] == 20 and info["skipped"] == 0 and info["nu"] == float(nu) and info["nu"] != 1.0 / c["Re"]


# ------------------------------------------------------------------ 4. replay = eager; lr 0 = off
def _train(monkeypatch, graph, steps, visc):
    _clean_env(monkeypatch, (("NSFNET_GRAPH", "1"),) if graph else ())
    c = vm.row_case("4x50-fp32-ev")
    E = _engine(c)
    if visc is not None:
        E.set_viscosity_identification(**visc)
    E.set_collocation(c["x"], c["y"], weights=c["w"])
    E.set_boundary(*_bc())
    for _ in range(steps):
        E.step(1e-3)
    torch.cuda.synchronize()
    out = dict(p=E.net.params.cpu().numpy().copy(), pe=E.net_e.params.cpu().numpy().copy())
    if visc is not None:
        out.update(state=E._visc.state.cpu().numpy().copy(), nu=E._visc.nu.cpu().numpy().copy())
    return out


def test_replayed_steps_equal_eager_ones_and_lr_zero_equals_off(monkeypatch):
    on = dict(lr=1e-2)
    eager = _train(monkeypatch, False, 21, on)
    replay = _train(monkeypatch, True, 21, on)          # 1 eager step + the capture, then 20 replays
    for k in ("p", "pe", "state", "nu"):
        assert fm.same_bits(eager[k], replay[k]), k
    assert eager["state"][5] == 21.0 and eager["nu"][0] != np.float32(1.0) / np.float32(400.0)
    held = _train(monkeypatch, False, 20, dict(lr=0.0))
    off = _train(monkeypatch, False, 20, None)
    assert fm.same_bits(held["p"], off["p"]) and fm.same_bits(held["pe"], off["pe"])
    assert held["nu"][0] == np.float32(1.0) / np.float32(400.0) and held["state"][5] == 20.0


# ------------------------------------------------------------------ 5. Kovasznay
def test_kovasznay_reynolds_number_is_identified(monkeypatch):
    """fp32, 4x50, 1000 collocation + 300 supervised (u, v, p) + 260 boundary points, Adam 1e-3 on the net and 1e-2 on
    ln nu from Re0 = 10: after 2000 updates the estimate is within 5 % of 40 and of the fp64 model's end value."""
    from nsfnet_amd import engine as eng
    _clean_env(monkeypatch)
    k = vm.KOV
    g = np.load(vm.GOLDEN)
    case = vm.kovasznay_case(int(g["seed"]))
    E = eng.PinnEngine(torch.device(DEV), k["L"], k["H"], k["re0"], alpha_b=k["alpha_b"], alpha_e=k["alpha_e"],
                       alpha_s=k["alpha_s"], precision="fp32")
    E.net.set_flat(torch.tensor(case["flat"]))
    E.set_viscosity_identification(re0=k["re0"], lr=k["lr_nu"])
    E.set_collocation(case["xf"], case["yf"])
    E.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    E.set_supervised(case["xs"], case["ys"], case["us"], case["vs"], case["ps"])
    traj = []
    for t in range(1, k["updates"] + 1):
        E.step(k["lr"])
        if t % k["every"] == 0:
            traj.append(1.0 / float(E._visc.nu.item()))
    info = E.viscosity_info()
    print("[viscosity] Kovasznay Re_est %.3f (model %.3f) after %d updates; every 500: %s" % (
        info["Re"], g["re"][-1], info["updates"], " ".join("%.2f" % v for v in traj[4::5])))
    assert info["updates"] == k["updates"] and info["skipped"] == 0
    assert abs(info["Re"] - k["Re"]) / k["Re"] <= 0.05, info["Re"]
    assert abs(info["Re"] - g["re"][-1]) / g["re"][-1] <= 0.05, (info["Re"], g["re"][-1])


# ------------------------------------------------------------------ 6. device nu = the launch constant
def _evaluated(monkeypatch, c, Re, re0):
    """The row's engine configured at Re after one loss_and_grad, identifying from re0 (None: the option off)."""
    _clean_env(monkeypatch, c.get("env", ()))
    E = _engine(c, Re=Re)
    if re0 is not None:
        E.set_viscosity_identification(re0=re0)
    _attach(E, c)
    if re0 is not None:
        E.plan_f.lap.fill_(float("nan"))
    E.loss_and_grad()
    torch.cuda.synchronize()
    f = E.plan_f
    out = dict(fields=f.fields[:, :f.n].cpu().numpy().copy(), sums=E.sums.cpu().numpy().copy(),
               grads=E.grads.cpu().numpy().copy(), loss=float(E.loss_terms()["loss"]), n=f.n)
    if re0 is not None:
        out["lap"] = f.lap.cpu().numpy().copy()
        assert E._visc.nu.cpu().numpy()[0] == np.float32(1.0) / np.float32(re0)
    return out


@pytest.mark.parametrize("name", [n for n in vm.ROWS if not vm.ROWS[n].get("ev")] + list(vm.BIT_ROWS))
def test_device_nu_gives_the_bits_of_the_launch_constant(monkeypatch, name):
    """nu starts as the fp32 quotient 1 / re0 the launches would have taken as a constant: the identifying engine,
    configured at another Re, and an engine configured at Re = re0 without the option hold the same bits.  A kernel
    that keeps the launch constant in some tile, a prologue or one of the fused kernel's two argument blocks fails, at
    any precision (the ev rows are left out: their vis_t0 follows the configured Re)."""
    c = vm.row_case(name)
    assert c["Re"] != c["re0"]
    a = _evaluated(monkeypatch, c, c["Re"], c["re0"])
    b = _evaluated(monkeypatch, c, c["re0"], None)
    assert np.isfinite(a["lap"]).all() and np.isfinite(a["sums"][vm.SLOT]) and a["sums"][vm.SLOT] != 0.0
    assert b["sums"][vm.SLOT] == 0.0
    keep = np.arange(a["sums"].size) != vm.SLOT
    for k, plane in enumerate(("u", "v", "u_x", "u_y", "v_x", "v_y", "eq1", "eq2", "eq3", "eq4", "p")):
        assert fm.same_bits(a["fields"][k], b["fields"][k]), plane
    assert np.abs(a["fields"][6]).max() > 0.0
    assert fm.same_bits(a["sums"][keep], b["sums"][keep]), (a["sums"], b["sums"])
    assert fm.same_bits(a["grads"], b["grads"]), int((a["grads"] != b["grads"]).sum())
    assert a["loss"] == b["loss"]


# ------------------------------------------------------------------ 7. the lap plane from two viscosities
@pytest.mark.parametrize("name", vm.LAP_ROWS)
def test_lap_is_the_laplacian_the_residual_used(monkeypatch, name):
    """eq1 = A - nu Lap u with A the same bits in both runs and nu a power of two (nu Lap u is exact, contracted into an
    fma or not), so eq_b - eq_a = (nu_a - nu_b) Lap u up to the two roundings of eq: per real point
    |(eq_b - eq_a) / (nu_a - nu_b) - lap| <= 2^-23 (|nu_a lap| + |nu_b lap| + |eq_a| + |eq_b|) / |nu_a - nu_b|.  On a
    hard-wall and on a sine row: the stored Laplacian is the one the residual used, after the transform."""
    c = vm.row_case(name)
    runs = [_evaluated(monkeypatch, c, c["Re"], re0) for re0 in vm.TWO_RE0]
    nu_a, nu_b = (float(np.float32(1.0) / np.float32(r)) for r in vm.TWO_RE0)
    a, b = runs
    n = a["n"]
    assert np.isfinite(a["lap"]).all() and fm.same_bits(a["lap"], b["lap"])
    for k, plane in ((0, 6), (1, 7)):
        L = a["lap"][k, :n].astype(np.float64)
        ea, eb = a["fields"][plane].astype(np.float64), b["fields"][plane].astype(np.float64)
        got = (eb - ea) / (nu_a - nu_b)                               # (the difference of two fp32 is exact in fp64)
        bound = 2.0 ** -23 * (np.abs(nu_a * L) + np.abs(nu_b * L) + np.abs(ea) + np.abs(eb)) / abs(nu_a - nu_b)
        worst = int(np.argmax(np.abs(got - L) - bound))
        print("[viscosity] %s lap[%d]: max |quotient - lap| / bound = %.3f, max |lap| %.3e" % (
            name, k, float((np.abs(got - L) / np.maximum(bound, 1e-300)).max()), np.abs(L).max()))
        assert np.abs(L).max() > 0.0 and (np.abs(got - L) <= bound).all(), (k, worst, got[worst], L[worst], bound[worst])
    for k in (0, 1, 2, 3, 4, 5, 8, 10):                               # everything ahead of - nu Lap: the same bits
        assert fm.same_bits(a["fields"][k], b["fields"][k]), k


# ------------------------------------------------------------------ 8. pinn_visc_grad alone
def _visc_grad_model(fields, lap, w, n, w4):
    """S as visc_grad_kernel forms it: the per-point term in fp64 from the fp32 planes, one rounding per operation in
    the kernel's order, fold_model.grid_fold over min(ceil(n / 1024), 512) blocks, one rounding to fp32."""
    d = lambda a: a[:n].astype(np.float64)
    a1, a2 = d(fields[6]), d(fields[7])
    if w4 != 0.0:
        c4 = np.float64(w4) * d(fields[9])
        du, dv = d(fields[0]) - 0.5, d(fields[1]) - 0.5
        q1, q2 = c4 * du, c4 * dv
        a1, a2 = a1 + q1, a2 + q2
    m1, m2 = a1 * d(lap[0]), a2 * d(lap[1])
    t = (1.0 if w is None else d(w)) * (m1 + m2)
    nblk = min(-(-n // 1024), 512)
    return np.float32(fm.grid_fold(t, nblk, threads=256, per=4))


VG_N = (1, 2, 3, 4, 5, 69, 1023, 1024, 1025, 512 * 1024, 512 * 1024 + 5, 2 * 512 * 1024 + 1027)


def test_visc_grad_is_the_numpy_statement_bit_for_bit():
    """Every launch on ONE scratch that is never cleared (the ticket must be left at 0), each twice in a row, the sizes
    in an order that puts small launches behind large ones; every entry of every plane behind n is NaN."""
    import types
    from nsfnet_amd import engine as eng
    gen = torch.Generator(device=DEV).manual_seed(11)
    scratch = eng.visc_scratch(max(VG_N), DEV)
    out = torch.zeros(1, dtype=torch.float32, device=DEV)
    order = (69, 2 * 512 * 1024 + 1027, 3, 512 * 1024 + 5, 1, 1025, 2, 512 * 1024, 5, 1024, 4, 1023)
    assert sorted(order) == sorted(VG_N)
    bad, ran = [], 0
    for n in order:
        npads = [-(-n // 4) * 4] + ([4096] if n == 69 else [])
        for npad in npads:
            fields = torch.randn(11, npad, generator=gen, dtype=torch.float32, device=DEV)
            lap = torch.randn(2, npad, generator=gen, dtype=torch.float32, device=DEV)
            w = torch.randn(n, generator=gen, dtype=torch.float32, device=DEV)
            fields[:, n:] = float("nan")
            lap[:, n:] = float("nan")
            fh, lh, wh = fields.cpu().numpy(), lap.cpu().numpy(), w.cpu().numpy()
            assert (fh[[0, 1, 6, 7, 9], :n] < 0).any() or n < 4
            for with_w in (False, True):
                for w4 in (0.0, 0.1):
                    plan = types.SimpleNamespace(n=n, npad=npad, fields=fields, lap=lap, w=w if with_w else None)
                    want = _visc_grad_model(fh, lh, wh if with_w else None, n, w4)
                    got = []
                    for _ in range(2):          # the second launch finds the scratch as the first left it
                        out.fill_(float("nan"))
                        eng.visc_grad(plan, w4, out, scratch)
                        got.append(out.cpu().numpy()[0])
                    ran += 2
                    assert np.isfinite(want)
                    if not all(g.view(np.uint32) == want.view(np.uint32) for g in got):
                        bad.append((n, npad, with_w, w4, got, want))
    assert int(scratch.view(torch.int64)[0].item()) == 0, "the ticket was not left at 0"
    assert not bad, bad[:8]
    assert ran == 2 * 4 * (len(VG_N) + 1)


# ------------------------------------------------------------------ 9. the options that run with the scalar on
def _option_engine(monkeypatch, graph=False):
    """The 2x8 fp32 engine at N_OPT collocation points, configured at the row's Re (the tests start nu at its re0)."""
    _clean_env(monkeypatch, (("NSFNET_GRAPH", "1"),) if graph else ())
    c = vm.row_case("2x8-fp32", n=vm.N_OPT)
    E = _engine(c)
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(*_bc())
    return E, c


def _nu32(re0):
    return np.float32(1.0) / np.float32(re0)


def test_a_batch_s_sum_and_lap_are_those_of_the_drawn_points(monkeypatch):
    E, c = _option_engine(monkeypatch)
    E.set_viscosity_identification(re0=c["re0"], lr=5e-2)
    E.set_batching(vm.B_OPT, seed=3)
    bf, vs, B = E._batch.f, E._visc, vm.B_OPT
    assert bf.nu is vs.nu and bf.n == B and bf.lap is not None
    bf.lap.fill_(float("nan"))
    E.plan_f.lap.fill_(float("nan"))
    E.loss_and_grad()
    E.adam_step(0.0)
    torch.cuda.synchronize()
    assert E.evaluated_batch
    idx = E.batch_indices().cpu().numpy()
    assert idx.shape == (B,) and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < vm.N_OPT
    lap = bf.lap.cpu().numpy().astype(np.float64)
    assert np.isfinite(lap).all() and torch.isnan(E.plan_f.lap).all()          # the batch plan ran, the store's did not
    r = vm.evaluate(c["flat"], c["L"], c["H"], c["x"][idx], c["y"][idx], float(_nu32(c["re0"])))
    assert r["kappa"] <= 3.0, r["kappa"]
    slot = np.float32(E.sums[vm.SLOT].item())
    errs = dict(lap_u=_rel_max(lap[0, :B], r["lap"][0]), lap_v=_rel_max(lap[1, :B], r["lap"][1]),
                eq1=_rel_max(bf.field("eq1").cpu().numpy(), r["eqs"][0]), S=abs(float(slot) - r["S"]) / abs(r["S"]))
    print("[viscosity] batch of %d of %d, kappa %.2f: %s" % (B, vm.N_OPT, r["kappa"], " ".join("%s %.2e" % kv for kv in errs.items())))
    assert errs["S"] <= S_BAR["fp32"], errs
    assert max(errs["lap_u"], errs["lap_v"], errs["eq1"]) <= BARS["fp32"]["eq"], errs
    st, nu = vm.new_state(c["re0"])
    st, _ = vm.update(st, nu, slot, -2.0 / B, 5e-2, theta_min=vs.theta_bounds[0], theta_max=vs.theta_bounds[1])
    assert fm.same_bits(vs.state.cpu().numpy(), st), (vs.state.cpu().numpy(), st)


def _train_batches(monkeypatch, graph, steps):
    E, c = _option_engine(monkeypatch, graph=graph)
    E.set_viscosity_identification(re0=c["re0"], lr=1e-2)
    E.set_batching(vm.B_OPT, seed=3)
    for _ in range(steps):
        E.step(1e-3)
    torch.cuda.synchronize()
    return dict(p=E.net.params.cpu().numpy().copy(), state=E._visc.state.cpu().numpy().copy(),
                nu=E._visc.nu.cpu().numpy().copy(), draws=E.batch_info()["draws"])


def test_replayed_batch_steps_equal_eager_ones_with_the_scalar_on(monkeypatch):
    eager = _train_batches(monkeypatch, False, 21)
    replay = _train_batches(monkeypatch, True, 21)          # 1 eager step + the capture, then 20 replays
    for k in ("p", "state", "nu"):
        assert fm.same_bits(eager[k], replay[k]), k
    assert eager["draws"] == replay["draws"] == 21 and eager["state"][5] == 21.0 and eager["nu"][0] != _nu32(100.0)


def test_with_attention_the_sum_takes_the_weights_the_sweep_read(monkeypatch):
    E, c = _option_engine(monkeypatch)
    E.set_residual_attention(eta=0.5, gamma=0.9)
    E.set_viscosity_identification(re0=c["re0"], lr=1e-2)
    E.step(1e-3)                        # the weights leave their start, the net and nu move
    f = E.plan_f
    w_read = f.w.cpu().numpy().astype(np.float64).copy()
    flat, nu = E.net.params.cpu().numpy().copy(), float(E._visc.nu.item())
    E.loss_and_grad()
    torch.cuda.synchronize()
    w_next = f.w.cpu().numpy().astype(np.float64)
    assert not np.array_equal(w_next, w_read)              # rewritten for the next evaluation
    r = vm.evaluate(flat, c["L"], c["H"], c["x"], c["y"], nu, w=w_read)
    other = float(np.sum(vm.terms(r["eqs"], r["u"], r["v"], r["lap"], w_next)))
    slot = float(E.sums[vm.SLOT].item())
    print("[viscosity] attention: S %.6e model %.6e (with the rewritten weights %.6e), kappa %.2f" % (slot, r["S"], other, r["kappa"]))
    assert r["kappa"] <= 3.0 and abs(other - r["S"]) > 10.0 * S_BAR["fp32"] * abs(r["S"])     # the control: the two differ
    assert abs(slot - r["S"]) <= S_BAR["fp32"] * abs(r["S"]), (slot, r["S"])


def test_the_pool_s_forward_reads_the_device_nu(monkeypatch):
    E, c = _option_engine(monkeypatch)
    E.set_viscosity_identification(re0=c["re0"])
    xp, yp = vm.pool_points()
    E.set_resample_pool(xp, yp)
    assert E._pool.nu is E._visc.nu and E._pool.lap is None
    at = lambda re: vm.evaluate(c["flat"], c["L"], c["H"], xp, yp, float(_nu32(re)))["eqs"][0]
    E.resample(seed=1)
    torch.cuda.synchronize()
    err = _rel_max(E._pool.field("eq1").cpu().numpy(), at(c["re0"]))
    E.set_viscosity_identification(enabled=False)
    assert E._pool.nu is None and E.plan_f.nu is None
    E.resample(seed=1)
    torch.cuda.synchronize()
    err_off = _rel_max(E._pool.field("eq1").cpu().numpy(), at(c["Re"]))
    print("[viscosity] pool eq1: on, against the model at 1 / re0 %.2e; detached, at 1 / Re %.2e" % (err, err_off))
    assert err <= BARS["fp32"]["eq"] and err_off <= BARS["fp32"]["eq"], (err, err_off)


def test_with_loss_balancing_the_state_is_the_model_on_the_slot(monkeypatch):
    E, c = _option_engine(monkeypatch)
    E.set_loss_balancing(every=2)
    E.set_viscosity_identification(re0=c["re0"], lr=5e-2)
    vs = E._visc
    st, nu = vm.new_state(c["re0"])
    for i in range(10):
        E.step(1e-3)
        slot = np.float32(E.sums[vm.SLOT].item())
        st, model_nu = vm.update(st, nu, slot, -2.0 / vm.N_OPT, 5e-2, theta_min=vs.theta_bounds[0], theta_max=vs.theta_bounds[1])
        assert fm.same_bits(vs.state.cpu().numpy(), st), i
        nu = np.float32(vs.nu.cpu().numpy()[0])
        assert abs(float(nu) - float(model_nu)) <= float(np.spacing(model_nu))
    info, bal = E.viscosity_info(), E.balance_info()
    assert info["updates"] == 10 and info["skipped"] == 0 and info["nu"] != float(_nu32(c["re0"]))
    assert bal["updates"] >= 4 and bal["adam_updates"] == 10 and bal["skipped"] == 0, bal
