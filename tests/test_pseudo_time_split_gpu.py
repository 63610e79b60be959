"""The pseudo-time variants of the role-split, wide role-split and fused sweeps ($PINN_PTIME_SPLIT=1, DESIGN.md section
7.11, "Role-split and fused sweeps"): the PT instantiations of fwd_split / bwd_split / fwdbwd_split (hidden 256) and
fwd_wsplit / bwd_wsplit (hidden 288 .. 448), with and without hard walls.

They run the point-stage expressions of point_stage.h that the 8-wave pseudo-time kernels run, so the method and the
bars are those of tests/test_pseudo_time_gpu.py, imported from it (_problem, _engine, BARS) - no bar here is new:
bf16x3 steady planes 5e-4 unscaled, loss (and each sum w q_k^2 alone) 1e-4 and gradient 1e-4 each times max(1, A),
with A <= 8 and "the pseudo-time terms carry weight" asserted on the fp64 model alone.  Anchors: the fields of an independently seeded net; rates: 1x
and 10x ptime_model.balanced_rates.  One row departs: 2x400 with walls runs at 1x and 2x, because at 10x the MODEL has
A = 15.4 (3x: 10.4, 2x: 7.2; the same at every point count tried from 37 to 200, and 11.0 at 3x400, 9.3 at 3x330):
with the lid's lift max|u| is 1 while q1 stays small, so the cancellation measure grows with the rate.  The bound
A <= 8 stays; 2x is the largest whole multiple that meets it.

Shapes: pairs of 32-point tiles (16 for the wide nets); N = 69 is 3 tiles at hidden 256 (a dummy partner and a partial
last tile), 5 at the wide widths; the tile-loop rows take N = (2 CUs + 2) x tile + 5, 2 CUs + 3 tiles in CUs + 2 pairs,
so that two workgroups take a second pair and the last pair has a dummy partner.  The fp64 model of 3x256 at that count
(16 453 points on 256 compute units) takes 2.5 s per evaluation on the CPU, so the row keeps L = 3.

Then: the fused kernel against the two launches bit for bit, zero rates against the plain plan of the same kernels,
the anchors untouched by an evaluation, pinn_ptime_advance after a fused step against its numpy model, graph replay
against eager steps, the switch inert without pseudo-time stepping, and plain bf16 finite.  Each row asserts the plan's
kernel names, and what its PINN_VERBOSE line says of the sweeps, before it compares."""
import functools
import os

import numpy as np
import pytest
import torch

import ptime_model as pm
from test_pseudo_time_gpu import ALPHA_E, BARS, RE, _engine, _problem, _rel_l2, _rel_max

pytestmark = pytest.mark.gpu

SWITCH = "PINN_PTIME_SPLIT"
SPLIT = ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
WSPLIT = ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")
FUSED, TWO, WIDE = "fused role-split kernel", "role-split kernels, two launches", "wide role-split kernels"
X3 = "bf16x3"


def _env(monkeypatch, fuse=None, switch="1", **more):
    """Every switch unset, then PINN_PTIME_SPLIT (and PINN_FUSE) as the row has them; PINN_VERBOSE=1 for _built."""
    for k in list(os.environ):
        if k.startswith("PINN_") or k in ("NSFNET_GRAPH", "NSFNET_CHUNK_POINTS"):
            monkeypatch.delenv(k, raising=False)
    if switch is not None:
        monkeypatch.setenv(SWITCH, switch)
    if fuse is not None:
        monkeypatch.setenv("PINN_FUSE", fuse)
    monkeypatch.setenv("PINN_VERBOSE", "1")
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def _built(capfd, make, names, path):
    """The engine make() builds, after its collocation plan named `names` and said `path` of its pseudo-time sweeps."""
    capfd.readouterr()
    E = make()
    err = capfd.readouterr().err
    said = [line.split("pseudo-time sweeps: ")[1] for line in err.splitlines() if "pseudo-time sweeps: " in line]
    assert E.plan_f.kernel_names() == names, E.plan_f.kernel_names()
    assert said and all(s == "%s (%s=%s)" % (path, SWITCH, os.environ.get(SWITCH, "0")) for s in said), err
    assert E.pseudo_time_info()["kernels"][:3] == names
    return E


def _loop_points(tile):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (2 * cus + 2) * tile + 5


def _n(N, H):
    return _loop_points(32 if H == 256 else 16) if N == "loop" else N


@functools.lru_cache(maxsize=None)
def _model_at_one(L, H, N, extra, vis_key):
    """The fp64 model of the case at rates (1, 1), which the balanced rates come from; computed once per case."""
    c = _problem(L, H, N, extra)
    return pm.residual_term(c.P, c.x, c.y, RE, c.anchor, 1.0, 1.0, alpha_e=ALPHA_E, vis_t=_VIS.get(vis_key), w=c.w,
                            scale=c.scale, bc=c.bc, params_e=c.P_e)


_VIS = {}

# (L, H, N, what else the case carries, PINN_FUSE, names, what the plan says, rate multiples)
ROWS = [
    (3, 256, 69, "plain", None, SPLIT, FUSED, (1.0, 10.0)),
    (3, 256, 69, "plain", "0", SPLIT, TWO, (1.0, 10.0)),
    (6, 256, 320, "plain", None, SPLIT, FUSED, (1.0, 10.0)),
    (3, 256, 69, "walls", None, SPLIT, FUSED, (1.0, 10.0)),
    (3, 256, 69, "ev", None, SPLIT, FUSED, (1.0, 10.0)),         # 3x256 + 4x40, weights, the coordinate map: vtm_old
    (3, 330, 69, "plain", None, WSPLIT, WIDE, (1.0, 10.0)),
    (2, 400, 150, "plain", None, WSPLIT, WIDE, (1.0, 10.0)),
    (2, 400, 150, "walls", None, WSPLIT, WIDE, (1.0, 2.0)),      # (10x: A = 15.4 on the model, see above)
    (3, 256, "loop", "plain", None, SPLIT, FUSED, (1.0, 10.0)),
    (2, 400, "loop", "plain", None, WSPLIT, WIDE, (1.0, 10.0)),
]
CASES = [r[:7] + (m,) for r in ROWS for m in r[7]]
IDS = ["%dx%d_%s_%s%s_%gx" % (c[0], c[1], c[2], c[3], "" if c[4] is None else "_fuse0", c[7]) for c in CASES]


@pytest.mark.parametrize("L,H,N,extra,fuse,names,path,mult", CASES, ids=IDS)
def test_loss_and_gradient_match_the_fp64_model(monkeypatch, capfd, L, H, N, extra, fuse, names, path, mult):
    N = _n(N, H)
    c, bar = _problem(L, H, N, extra), BARS[X3]
    _env(monkeypatch, fuse, PINN_HBC_SPLIT="0")         # (a pseudo-time plan with walls never looks at that one)
    E = _built(capfd, lambda: _engine(c, L, H, X3, True), names, path)
    f = E.plan_f
    tile = 32 if H == 256 else 16
    assert f.npad == -(-N // tile) * tile and (f.hard_bc() is not None) == (extra == "walls")
    f.anchor[:, :N].copy_(torch.tensor(c.anchor))
    vis_t, vis_key = None, None
    if c.ev:        # the artificial viscosity of the evaluation, which the steady residuals and so the rates depend on
        E.loss_and_grad()
        torch.cuda.synchronize()
        vis_t = f.vis_t.cpu().numpy().astype(np.float64)
        E.init_vis_t()                              # ... and the same lagged state again for the evaluation judged
        vis_key = (L, H, N, extra)
        _VIS.setdefault(vis_key, vis_t)
        np.testing.assert_array_equal(_VIS[vis_key], vis_t)
    model = lambda s, sp: pm.residual_term(c.P, c.x, c.y, RE, c.anchor, s, sp, alpha_e=ALPHA_E, vis_t=vis_t, w=c.w,
                                           scale=c.scale, bc=c.bc, params_e=c.P_e)
    sb, spb = pm.balanced_rates(_model_at_one(L, H, N, extra, vis_key))
    f.set_pseudo_time(mult * sb, mult * spb)
    sigma, sigma_p = f.pseudo_time()                # the fp32 launch constants
    assert abs(sigma - mult * sb) <= 1e-6 * mult * sb and abs(sigma_p - mult * spb) <= 1e-6 * mult * spb
    before = f.anchor.clone()
    E.loss_and_grad()
    torch.cuda.synchronize()
    assert torch.equal(f.anchor, before)            # an evaluation never writes the anchors
    if c.ev:
        np.testing.assert_array_equal(f.vis_t.cpu().numpy().astype(np.float64), vis_t)
        assert float(np.abs(vis_t).max()) > 0.0
    r = model(sigma, sigma_p)
    A = pm.amplification(r, c.anchor, sigma, sigma_p)
    grow = max(1.0, A)
    print("rates %.4e / %.4e (%gx balanced), A = %.3f" % (sigma, sigma_p, mult, A))
    assert A <= 8.0
    ratio = [r["sums"][k] / r["steady_sums"][k] for k in range(3)]
    print("sum w q_k^2 / sum w eq_k^2 = %.3f %.3f %.3f" % tuple(ratio))
    assert all(abs(q - 1.0) > 0.05 for q in ratio)          # the pseudo-time terms carry weight
    for name in ("u", "v", "p", "u_x", "u_y", "v_x", "v_y"):
        err = _rel_max(f.field(name).cpu().numpy(), r["fields"][name])
        print("%s: max-abs / max|ref| = %.3e" % (name, err))
        assert err < bar["field"], name
    for k, ref in enumerate(r["eqs"]):
        err = _rel_max(f.field("eq%d" % (k + 1)).cpu().numpy(), ref)
        print("eq%d (steady): max-abs / max|ref| = %.3e" % (k + 1, err))
        assert err < bar["field"], k
    sums = E.sums.cpu().numpy().astype(np.float64)
    for k in range(3):
        print("sum w q%d^2: relative error %.3e" % (k + 1, abs(sums[k] - r["sums"][k]) / r["sums"][k]))
        assert abs(sums[k] - r["sums"][k]) < bar["loss"] * grow * r["sums"][k], k
    lt = E.loss_terms()
    loss, want = float(lt["loss"]), c.loss_v + r["loss_e"]
    print("loss %.9e (model %.9e): relative error %.3e, bar %.3e" % (loss, want, abs(loss - want) / want, bar["loss"] * grow))
    assert abs(float(lt["loss_e"]) - r["loss_e"]) < bar["loss"] * grow * r["loss_e"]
    assert abs(loss - want) < bar["loss"] * grow * want
    g, gw = E.grads.cpu().numpy(), c.grad_v + r["grad"]
    print("gradient rel-L2 = %.3e, bar %.3e" % (_rel_l2(g, gw), bar["grad"] * grow))
    assert _rel_l2(g, gw) < bar["grad"] * grow
    if c.ev:
        print("entropy-net gradient rel-L2 = %.3e" % _rel_l2(E.grads_e.cpu().numpy(), r["grad_e"]))
        assert _rel_l2(E.grads_e.cpu().numpy(), r["grad_e"]) < bar["grad"] * grow


# ---- the fused kernel equals the two launches on the same pseudo-time plan, bit for bit ----
def _rates(extra):
    """Balanced rates of the N = 69 case (its lagged viscosity at zero): both terms carry weight at every count."""
    return pm.balanced_rates(_model_at_one(3, 256, 69, extra, None))


def _evaluated(monkeypatch, capfd, c, prec, fuse, path, rates):
    _env(monkeypatch, fuse)
    E = _built(capfd, lambda: _engine(c, 3, 256, prec, True), SPLIT, path)
    f = E.plan_f
    f.anchor[:, :c.N].copy_(torch.tensor(c.anchor))
    f.set_pseudo_time(*rates)
    E.loss_and_grad()
    torch.cuda.synchronize()
    out = dict(fields=f.fields, vis_t=f.vis_t, sums=E.sums, grads=E.grads)
    if c.ev:
        out.update(vis_t_minus=f.vis_t_minus, grads_e=E.grads_e, ebar=f.ebar)
    return E, {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("prec", [X3, "bf16"])
@pytest.mark.parametrize("N", [69, "loop"])
@pytest.mark.parametrize("extra", ["plain", "ev", "walls"])
def test_fused_equals_the_two_launches_bit_for_bit(monkeypatch, capfd, extra, N, prec):
    c, rates = _problem(3, 256, _n(N, 256), extra), _rates(extra)
    _, one = _evaluated(monkeypatch, capfd, c, prec, None, FUSED, rates)
    _, two = _evaluated(monkeypatch, capfd, c, prec, "0", TWO, rates)
    assert sorted(one) == sorted(two) and ("ebar" in one) == (extra == "ev")
    assert torch.isfinite(one["grads"]).all() and float(one["grads"].abs().max()) > 0 and float(one["sums"][:3].min()) > 0
    if extra == "ev":
        assert float(one["vis_t"].abs().max()) > 0 and float(one["ebar"].abs().max()) > 0
    for k in sorted(one):
        np.testing.assert_array_equal(one[k].cpu().numpy(), two[k].cpu().numpy(), err_msg=k)


# ---- zero rates: the plain plan of the same role-split kernels ----
@pytest.mark.parametrize("L,H,N,extra,names,path", [(6, 256, 320, "plain", SPLIT, FUSED), (2, 400, 150, "plain", WSPLIT, WIDE),
                                                    (3, 256, 69, "walls", SPLIT, FUSED)],
                         ids=["6x256", "2x400", "3x256_walls"])
def test_zero_rates_equal_the_plain_plan_of_the_same_kernels(monkeypatch, capfd, L, H, N, extra, names, path):
    c, bar = _problem(L, H, N, extra), BARS[X3]
    _env(monkeypatch, PINN_HBC_SPLIT="1")               # (the plain plan with walls on the role-split kernels, too)
    plain = _engine(c, L, H, X3, False)
    E = _built(capfd, lambda: _engine(c, L, H, X3, True), names, path)
    assert plain.plan_f.kernel_names() == names
    E.plan_f.anchor[:, :c.N].copy_(torch.tensor(c.anchor))
    E.plan_f.set_pseudo_time(0.0, 0.0)
    for e in (plain, E):
        e.loss_and_grad()
    torch.cuda.synchronize()
    for name in ("u", "v", "p", "u_x", "u_y", "v_x", "v_y", "eq1", "eq2", "eq3"):
        err = _rel_max(E.plan_f.field(name).cpu().numpy(), plain.plan_f.field(name).cpu().numpy())
        print("%s: max-abs / max|plain| = %.3e" % (name, err))
        assert err < bar["field"], name
    la, lb = float(E.loss_terms()["loss"]), float(plain.loss_terms()["loss"])
    err = _rel_l2(E.grads.cpu().numpy(), plain.grads.cpu().numpy())
    print("loss: relative difference %.3e; gradient rel-L2 = %.3e" % (abs(la - lb) / lb, err))
    assert abs(la - lb) < bar["loss"] * lb and err < bar["grad"]


# ---- pinn_ptime_advance on the planes the fused kernel wrote ----
def test_advance_after_a_fused_step_equals_its_model_bit_for_bit(monkeypatch, capfd):
    from nsfnet_amd import engine as eng
    c = _problem(3, 256, 69, "plain")
    E, _ = _evaluated(monkeypatch, capfd, c, X3, None, FUSED, _rates("plain"))
    f, pt = E.plan_f, E._pt
    fld, anchor, rec = f.fields.cpu().numpy(), f.anchor.cpu().numpy(), pt.record.cpu().numpy()
    assert np.abs(fld[pm.FLD_U, :c.N] - anchor[0, :c.N]).max() > 0
    eng.ptime_advance(f, pt.every, True, pt.scratch, pt.record)
    torch.cuda.synchronize()
    want_anchor, want = pm.advance(fld, c.N, anchor, pt.every, True, None, rec)
    got = pt.record.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (got, want)
    assert want[pm.R_DRIFT_UV] > 0.0 and want[pm.R_REFRESHES] == rec[pm.R_REFRESHES] + 1.0
    np.testing.assert_array_equal(f.anchor.cpu().numpy(), want_anchor)
    np.testing.assert_array_equal(f.anchor[0, :c.N].cpu().numpy(), fld[pm.FLD_U, :c.N])


# ---- the engine: graph replay, the switch without the feature, plain bf16 ----
def _stepping(c, pt, prec=X3):
    from nsfnet_amd import engine as eng
    E = eng.PinnEngine(torch.device("cuda:0"), 3, 256, RE, alpha_b=10.0, alpha_e=ALPHA_E, precision=prec)
    if c.bc is not None:
        E.set_hard_boundary(True, lift_power=c.bc.m)
    if pt is not None:
        E.set_pseudo_time(**pt)
    E.net.set_flat(torch.tensor(c.flat))
    E.set_collocation(c.x, c.y)
    E.set_boundary(*c.bnd)
    return E


@pytest.mark.parametrize("extra", ["plain", "walls"])
def test_ten_replayed_steps_equal_ten_eager_ones(monkeypatch, capfd, extra):
    c = _problem(3, 256, 69, extra)

    def run(graph):
        _env(monkeypatch, NSFNET_GRAPH="1" if graph else "0")
        E = _built(capfd, lambda: _stepping(c, dict(dtau=0.5, every=3, pressure_dtau=2.0)), SPLIT, FUSED)
        for _ in range(10):         # graph: one eager step and the capture, then nine replays
            E.step(1e-3)
        torch.cuda.synchronize()
        assert len(E._graphs) == (1 if graph else 0)
        i = E.pseudo_time_info()
        assert (i["since_refresh"], i["refreshes"]) == (1, 4)           # the attach, then updates 3, 6, 9
        assert float(E.loss_terms()["drift"]) > 0.0
        return [t.cpu().numpy().copy() for t in (E.net.params, E.plan_f.anchor, E._pt.record, E.plan_f.fields)]

    for a, b in zip(run(False), run(True)):
        assert a.tobytes() == b.tobytes()


def test_switch_is_inert_without_pseudo_time_stepping(monkeypatch):
    c = _problem(3, 256, 69, "plain")

    def run(switch):
        _env(monkeypatch, switch=switch)
        E = _stepping(c, None)
        assert E.plan_f.kernel_names() == SPLIT and E.plan_f.anchor is None and E.pseudo_time_info() is None
        E.loss_and_grad()
        first = [t.cpu().numpy().copy() for t in (E.grads, E.sums, E.plan_f.fields)]
        for _ in range(5):
            E.step(1e-3)
        torch.cuda.synchronize()
        return first + [t.cpu().numpy().copy() for t in (E.grads, E.sums, E.plan_f.fields, E.net.params)]

    off, on = run(None), run("1")
    for a, b in zip(off, on):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("fuse,path", [(None, FUSED), ("0", TWO)], ids=["fused", "two_launches"])
def test_plain_bf16_runs_and_is_finite(monkeypatch, capfd, fuse, path):
    c = _problem(3, 256, 69, "plain")
    _env(monkeypatch, fuse)
    E = _built(capfd, lambda: _stepping(c, dict(dtau=0.5, every=2, pressure_dtau=1.0), "bf16"), SPLIT, path)
    for _ in range(3):
        E.step(1e-3)
    torch.cuda.synchronize()
    assert np.isfinite(E.grads.cpu().numpy()).all() and np.isfinite(E.net.params.cpu().numpy()).all()
    i = E.pseudo_time_info()
    assert np.isfinite(i["steady_sums"]).all() and i["refreshes"] == 2 and i["drift_uv"] >= 0.0
