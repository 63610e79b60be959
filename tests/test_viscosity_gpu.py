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
            "PINN_S0_SKIP32", "NSFNET_CHUNK_POINTS", "NSFNET_GRAPH", "PINN_PTIME_SPLIT")
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
    for k, v in env:
        monkeypatch.setenv(k, v)


def _engine(c, **kw):
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=vm.EV_NET[0], hidden_e=vm.EV_NET[1], alpha_evm=vm.ALPHA_EVM) if c.get("ev") else {}
    E = eng.PinnEngine(torch.device(DEV), c["L"], c["H"], c["Re"], alpha_b=10.0, alpha_e=1.0, precision=c["prec"],
                       coord_scale=c["scale"], **ev, **kw)
    E.net.set_flat(torch.tensor(c["flat"]))
    if c.get("ev"):
        E.net_e.set_flat(torch.tensor(c["flat_e"]))
        E.e_trainable = True
    if c.get("hard_bc"):
        E.set_hard_boundary()
    return E


# ------------------------------------------------------------------ 1. one evaluation per family
_REF = {}


@pytest.mark.parametrize("shifted", [False, True], ids=["re0=Re", "re0-away"])
@pytest.mark.parametrize("name", list(vm.ROWS))
def test_evaluation_matches_the_model(monkeypatch, name, shifted):
    """shifted: the estimate starts away from the configured Re, so a sweep that keeps the launch constant 1 / Re, in all
    or in some of its tiles, misses the model (tests/test_viscosity_cpu.py: by more than ten bars in S, eq1, the gradient)."""
    c = vm.row_case(name)
    re0 = vm.row_re0(c, shifted)
    _clean_env(monkeypatch, c.get("env", ()))
    E = _engine(c)
    E.set_viscosity_identification(re0=re0)
    E.set_collocation(c["x"], c["y"], weights=c["w"])
    xb, yb, ub, vb = _bc()
    E.set_boundary(xb, yb, ub, vb)
    f = E.plan_f
    assert f.kernel_names() == c["names"]
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
    # the reference: one per (net, points) - the 6x256 rows share theirs
    key = (name if c["L"] != 6 else "6x256", shifted)
    if key not in _REF:
        vis_t = None if vtm0 is None else np.minimum(np.float32(20.0 / c["Re"]), vtm0)
        r = vm.row_reference(c, vis_t=vis_t, re0=re0)
        P = fr.unflatten(c["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
        if c.get("hard_bc"):
            import hardbc_model as hm
            b = hm.constrained_value(P, hm.HardBc(), xb, yb, targets=[ub, vb, None], coef=[20.0 / xb.size] * 2 + [0.0])
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
