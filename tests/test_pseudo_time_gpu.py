"""Pseudo-time stepping of the residual loss on the device: loss_and_grad of a pseudo-time plan
in every 8-wave kernel family against the fp64 model of tests/ptime_model.py, with anchors that are the fields of an
independently seeded net and rates at 1x and 10x the balanced ones (ptime_model.balanced_rates), so that both the
steady residuals and the pseudo-time terms carry weight.  Bars, those of tests/test_hardbc_gpu.py:
                                   fp32     bf16x3
  steady planes, max-abs / max|ref|  2e-5     5e-4       (fields, derivatives, eq1..eq4; unscaled)
  loss, relative                     1e-5     1e-4       x max(1, A)      (and each of the sums w q_k^2 alone)
  gradient, relative L2              1e-4     1e-4       x max(1, A)
A = max_k (max|eq_k| + sigma_k max|c_k|) / max|q_k| (ptime_model.amplification) is the first-order growth of q's error
from the cancellation in eq + sigma (c - c*); the test asserts A <= 8 on the model alone.  Then: zero rates equal the
plain plan of the same kernels, pinn_ptime_advance equals its numpy model bit for bit, a replayed graph equals the eager
steps with the refresh inside the replay, and with the feature off nothing changes."""
import functools
import types

import numpy as np
import pytest
import torch

import fold_model as fm
import hardbc_model as hm
import ptime_model as pm
from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr

pytestmark = pytest.mark.gpu

BARS = {"fp32": dict(field=2e-5, loss=1e-5, grad=1e-4), "bf16x3": dict(field=5e-4, loss=1e-4, grad=1e-4)}
RE, ALPHA_B, ALPHA_E = 400.0, 10.0, 1.0
# (L, H, N, precision, what else the case carries, (forward, reverse sweep) kernels it must reach or None).  N = "2cu":
# the ragged count just above twice the compute units times 32; "4cu": just above four times - the 4x50 sweeps run
# up to 8 / (64 / 32) = 4 workgroups per compute unit (resolve_plan), so only there does a workgroup of every
# residency take a second tile and index the anchors of a tile that is not its first.
CASES = [
    (1, 8, 37, "fp32", "plain", None),
    (4, 50, 1000, "fp32", "ev", None),
    (4, 50, 1000, "bf16x3", "supervised", None),
    (6, 256, 320, "fp32", "plain", ("fwd_wide_kernel", "bwd_wide_kernel")),
    (6, 256, 320, "bf16x3", "plain", ("fwd_bf16_kernel", "bwd_bf16_kernel")),
    (3, 400, 150, "bf16x3", "plain", ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel")),
    (4, 50, 1000, "bf16x3", "walls", None),
    (4, 50, "2cu", "bf16x3", "plain", None),
    (4, 50, "4cu", "bf16x3", "plain", None),
]
IDS = ["%dx%d_%s_%s_%s" % (c[0], c[1], c[2], c[3], c[4]) for c in CASES]


def _engine_mod():
    from nsfnet_amd import engine
    return engine


def _rel_max(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _flat(n_out, L, H, seed):
    return ar.flat_params(ar.seeded_net(n_out, L, H, seed=seed)).numpy().copy()


def _boundary(Nb=129):
    return tuple(a.reshape(-1)[:: max(1, 2052 // Nb)][:Nb].astype(np.float32) for a in ar.cavity_boundary())


def _points(N):
    if isinstance(N, str):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        return int(N[0]) * cus * 32 + 5
    return N


@functools.lru_cache(maxsize=None)
def _problem(L, H, N, extra):
    """Everything of a case that does not depend on the precision or the rates, computed once: the parameters, the
    points, the fp32 anchors (the fields of another net of the same shape) and the value terms of the fp64 model."""
    N = _points(N)
    ev, walls = extra == "ev", extra == "walls"
    c = types.SimpleNamespace(N=N, ev=ev, flat=_flat(3, L, H, 100 + H), flat_e=None, w=None, sup=None, alpha_s=0.0,
                              scale=1.0, bc=None, kw={})
    lo = 0.0
    if ev:      # the coordinate map (scale 2, origin -1), SDF-like weights and a trainable entropy net
        c.flat_e, c.scale, lo = _flat(1, 4, 40, 6), 2.0, -1.0
        c.kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05, coord_scale=2.0)
        c.w = (0.3 + np.random.RandomState(9).rand(N)).astype(np.float32)
    if walls:
        c.bc = hm.HardBc(lift_power=3)
    rng = np.random.RandomState(H + L)
    sx, sy = hm.special_points(lo, 1.0)
    c.x = np.concatenate([sx, (lo + (1.0 - lo) * rng.rand(N - sx.size)).astype(np.float32)])
    c.y = np.concatenate([sy, (lo + (1.0 - lo) * rng.rand(N - sy.size)).astype(np.float32)])
    xb, yb, ub, vb = _boundary()
    c.bnd = ((1.0 - lo) * xb + lo, (1.0 - lo) * yb + lo, ub, vb)
    if extra == "supervised":       # samples with NaN-masked pressure targets
        r = np.random.RandomState(11)
        c.sup = [r.rand(77).astype(np.float32), r.rand(77).astype(np.float32), r.randn(77).astype(np.float32),
                 r.randn(77).astype(np.float32), r.randn(77).astype(np.float32)]
        c.sup[4][::3] = np.nan
        c.alpha_s = 2.0
        c.kw = dict(alpha_s=2.0)
    c.P = fr.unflatten(c.flat.astype(np.float64), 2, 3, L, H)
    c.P_e = None if not ev else fr.unflatten(c.flat_e.astype(np.float64), 2, 1, 4, 40)
    other = fr.unflatten(_flat(3, L, H, 200 + H).astype(np.float64), 2, 3, L, H)
    f = pm.residual_term(other, c.x, c.y, RE, np.zeros((3, N)), 0.0, 0.0, bc=c.bc, scale=c.scale)["fields"]
    c.anchor = np.stack([f["u"], f["v"], f["p"]]).astype(np.float32)
    # the value terms: loss and gradient of the boundary and the supervised points
    value = (lambda x, y, t, coef: hm.constrained_value(c.P, c.bc, x, y, t, coef)) if walls else (
        lambda x, y, t, coef: fr.value_loss_and_grad_chunked(c.P, x, y, t, coef))
    nb = len(ub)
    b = value(c.bnd[0], c.bnd[1], [ub, vb, None], (2.0 * ALPHA_B / nb, 2.0 * ALPHA_B / nb, 0.0))
    c.loss_v, c.grad_v = ALPHA_B * (b["sums"][0] + b["sums"][1]) / nb, b["grad"]
    if c.sup is not None:
        ns, n_p = 77, int(np.isfinite(c.sup[4]).sum())
        s = value(c.sup[0], c.sup[1], c.sup[2:], (2.0 * c.alpha_s / ns, 2.0 * c.alpha_s / ns, 2.0 * c.alpha_s / n_p))
        c.loss_v += c.alpha_s * ((s["sums"][0] + s["sums"][1]) / ns + s["sums"][2] / n_p)
        c.grad_v = c.grad_v + s["grad"]
    return c


def _engine(c, L, H, prec, pseudo_time, dtau=1.0, pressure_dtau=1.0):
    eng = _engine_mod()
    E = eng.PinnEngine(torch.device("cuda:0"), L, H, RE, alpha_b=ALPHA_B, alpha_e=ALPHA_E, precision=prec, **c.kw)
    if c.bc is not None:
        E.set_hard_boundary(True, lift_power=c.bc.m)
    if pseudo_time:
        E.set_pseudo_time(dtau=dtau, every=1000, pressure_dtau=pressure_dtau)
    E.net.set_flat(torch.tensor(c.flat))
    if c.ev:
        E.net_e.set_flat(torch.tensor(c.flat_e))
        E.e_trainable = True
    E.set_collocation(c.x, c.y, weights=c.w)
    E.set_boundary(*c.bnd)
    if c.sup is not None:
        E.set_supervised(*c.sup)
    return E


@pytest.mark.parametrize("mult", [1.0, 10.0], ids=["1x", "10x"])
@pytest.mark.parametrize("L,H,N,prec,extra,kernels", CASES, ids=IDS)
def test_loss_and_gradient_match_the_fp64_model(L, H, N, prec, extra, kernels, mult):
    c, bar = _problem(L, H, N, extra), BARS[prec]
    N = c.N
    E = _engine(c, L, H, prec, True)        # (the engine's own rates are placeholders: the plan gets the balanced ones below)
    f = E.plan_f
    names = f.kernel_names()
    if kernels is not None:
        assert names[:2] == kernels
    assert "split" not in names[0] + names[1] and "pipe" not in names[0] + names[1]
    f.anchor[:, :N].copy_(torch.tensor(c.anchor))
    vis_t = None
    if c.ev:        # the artificial viscosity of the evaluation, which the steady residuals and so the rates depend on
        E.loss_and_grad()
        torch.cuda.synchronize()
        vis_t = f.vis_t.cpu().numpy().astype(np.float64)
        E.init_vis_t()                              # ... and the same lagged state again for the evaluation judged
    model = lambda s, sp: pm.residual_term(c.P, c.x, c.y, RE, c.anchor, s, sp, alpha_e=ALPHA_E, vis_t=vis_t, w=c.w,
                                           scale=c.scale, bc=c.bc, params_e=c.P_e)
    sb, spb = pm.balanced_rates(model(1.0, 1.0))
    f.set_pseudo_time(mult * sb, mult * spb)
    sigma, sigma_p = f.pseudo_time()                # the fp32 launch constants
    assert abs(sigma - mult * sb) <= 1e-6 * mult * sb and abs(sigma_p - mult * spb) <= 1e-6 * mult * spb
    E.loss_and_grad()
    torch.cuda.synchronize()
    if c.ev:
        np.testing.assert_array_equal(f.vis_t.cpu().numpy().astype(np.float64), vis_t)
    r = model(sigma, sigma_p)
    A = pm.amplification(r, c.anchor, sigma, sigma_p)
    grow = max(1.0, A)
    print("rates %.4e / %.4e (%gx balanced), A = %.3f" % (sigma, sigma_p, mult, A))
    assert A <= 8.0
    ratio = [r["sums"][k] / r["steady_sums"][k] for k in range(3)]
    print("sum w q_k^2 / sum w eq_k^2 = %.3f %.3f %.3f" % tuple(ratio))
    assert all(abs(q - 1.0) > 0.05 for q in ratio)          # the pseudo-time terms carry weight
    # the steady planes, unscaled bars
    for name in ("u", "v", "p", "u_x", "u_y", "v_x", "v_y"):
        err = _rel_max(f.field(name).cpu().numpy(), r["fields"][name])
        print("%s: max-abs / max|ref| = %.3e" % (name, err))
        assert err < bar["field"], name
    for k, ref in enumerate(r["eqs"]):
        err = _rel_max(f.field("eq%d" % (k + 1)).cpu().numpy(), ref)
        print("eq%d (steady): max-abs / max|ref| = %.3e" % (k + 1, err))
        assert err < bar["field"], k
    # loss sums 0..2 hold sum w q_k^2; the loss and the gradient
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


@pytest.mark.parametrize("L,H,N,prec,extra", [(4, 50, 1000, "fp32", "plain"), (6, 256, 320, "bf16x3", "plain"),
                                              (3, 400, 150, "bf16x3", "plain"), (4, 50, 1000, "bf16x3", "walls")],
                         ids=["4x50_fp32", "6x256_bf16x3", "3x400_bf16x3", "4x50_bf16x3_walls"])
def test_zero_rates_equal_the_plain_plan_of_the_same_kernels(L, H, N, prec, extra, monkeypatch):
    c, bar = _problem(L, H, N, extra), BARS[prec]
    for k in ("PINN_SCHED", "PINN_WSPLIT", "PINN_FUSE"):       # the plain plan on the 8-wave families, too
        monkeypatch.setenv(k, "0")
    monkeypatch.delenv("PINN_HBC_SPLIT", raising=False)
    plain = _engine(c, L, H, prec, False)
    E = _engine(c, L, H, prec, True)
    assert E.plan_f.kernel_names() == plain.plan_f.kernel_names()
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


# ---- pinn_ptime_advance against its numpy model ----
def _advance_state(n, seed, weights=True):
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(seed)
    npad = -(-n // 32) * 32
    s = types.SimpleNamespace(n=n, npad=npad)
    s.fld = rng.randn(pm.FLD_COUNT, npad).astype(np.float32)
    s.anc = rng.randn(3, npad).astype(np.float32)
    s.wv = (0.5 + rng.rand(n)).astype(np.float32) if weights else None
    s.fields, s.anchor = torch.tensor(s.fld, device=dev), torch.tensor(s.anc, device=dev)
    s.w = None if s.wv is None else torch.tensor(s.wv, device=dev)
    s.scratch = _engine_mod().ptime_scratch(n, dev)
    s.record = torch.zeros(pm.RECORD, dtype=torch.float64, device=dev)
    return s


# one thread's tail; several blocks with a ragged last quad; past the grid cap of 512 blocks x 1024 points
@pytest.mark.parametrize("n,weights", [(37, True), (5001, False), (5003, True), (512 * 1024 + 3001, True)],
                         ids=["37", "5001_no_w", "5003", "past_the_grid_cap"])
def test_advance_equals_its_model_bit_for_bit(n, weights):
    eng = _engine_mod()
    s = _advance_state(n, n % 97, weights)
    anchor, rec = s.anc, None
    for t, (every, force) in enumerate([(3, False), (3, False), (3, False), (0, False), (0, True)] if n < 10000 else [(1, False)]):
        s.fields.copy_(torch.tensor(np.roll(s.fld, t, axis=1)))         # the field moves
        eng.ptime_advance(s, every, force, s.scratch, s.record)
        torch.cuda.synchronize()
        anchor, rec = pm.advance(np.roll(s.fld, t, axis=1), n, anchor, every, force, s.wv, rec)
        got = s.record.cpu().numpy()
        assert fm.same_bits(got[:6], rec[:6]), (t, got, rec)
        assert got[6] == rec[6] and got[7] == rec[7], (t, got, rec)
        np.testing.assert_array_equal(s.anchor.cpu().numpy(), anchor)
        assert not s.scratch[0].item()                                 # the ticket word is 0 between launches
    assert rec[pm.R_REFRESHES] == (2.0 if n < 10000 else 1.0)


def test_advance_is_bit_reproducible_and_propagates_a_nan():
    eng = _engine_mod()
    n = 200003
    runs = []
    for _ in range(2):
        s = _advance_state(n, 5)
        eng.ptime_advance(s, 0, False, s.scratch, s.record)
        torch.cuda.synchronize()
        runs.append(s.record.cpu().numpy().copy())
    assert runs[0].tobytes() == runs[1].tobytes() and runs[0][pm.R_MAX] > 0.0
    s.fields[pm.FLD_U, 123457] = float("nan")
    eng.ptime_advance(s, 0, False, s.scratch, s.record)
    torch.cuda.synchronize()
    rec = s.record.cpu().numpy()
    assert np.isnan(rec[pm.R_MAX]) and np.isnan(rec[pm.R_DRIFT_UV]) and np.isfinite(rec[pm.R_DRIFT_P])
    assert np.isfinite(rec[:3]).all() and rec[pm.R_SINCE] == 2.0


# ---- the engine: graph replay, feature off, plain bf16 ----
def _small_engine(prec="fp32", pt=None, seed=3, walls=False):
    eng = _engine_mod()
    L, H = 3, 40
    E = eng.PinnEngine(torch.device("cuda:0"), L, H, RE, alpha_b=ALPHA_B, alpha_e=ALPHA_E, precision=prec)
    if walls:
        E.set_hard_boundary(True)
    if pt is not None:
        E.set_pseudo_time(**pt)
    E.net.set_flat(torch.tensor(_flat(3, L, H, seed)))
    rng = np.random.RandomState(7)
    E.set_collocation(rng.rand(300).astype(np.float32), rng.rand(300).astype(np.float32))
    E.set_boundary(*_boundary())
    return E


@pytest.mark.parametrize("walls", [False, True], ids=["plain", "walls"])
def test_ten_replayed_steps_equal_ten_eager_ones(monkeypatch, walls):
    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E = _small_engine(pt=dict(dtau=0.5, every=3, pressure_dtau=2.0), walls=walls)
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


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_feature_off_is_bitwise_the_engine_that_never_heard_of_it(prec):
    def run(pt):
        E = _small_engine(prec, pt)
        assert E.plan_f.anchor is None and E.pseudo_time_info() is None
        E.loss_and_grad()
        first = [t.cpu().numpy().copy() for t in (E.grads, E.sums, E.plan_f.fields)]
        for _ in range(5):
            E.step(1e-3)
        torch.cuda.synchronize()
        assert "drift" not in E.loss_terms()
        return first + [t.cpu().numpy().copy() for t in (E.grads, E.sums, E.plan_f.fields, E.net.params)]

    never, off = run(None), run(dict(dtau=None, every=0))
    for a, b in zip(never, off):
        assert a.tobytes() == b.tobytes()
    # ... and the term is not a no-op
    E = _small_engine(prec, dict(dtau=0.5, every=2))
    for _ in range(5):
        E.step(1e-3)
    torch.cuda.synchronize()
    assert not np.array_equal(E.net.params.cpu().numpy(), never[-1])


def test_plain_bf16_runs_and_is_finite():
    E = _small_engine("bf16", dict(dtau=0.5, every=2, pressure_dtau=1.0))
    for _ in range(3):
        E.step(1e-3)
    torch.cuda.synchronize()
    assert np.isfinite(E.grads.cpu().numpy()).all() and np.isfinite(E.net.params.cpu().numpy()).all()
    i = E.pseudo_time_info()
    assert np.isfinite(i["steady_sums"]).all() and i["refreshes"] == 2 and i["drift_uv"] >= 0.0
