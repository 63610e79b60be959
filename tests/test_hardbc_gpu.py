"""Hard wall conditions by an output transform on the device: the constrained
loss_and_grad of every 8-wave kernel family against the fp64 model of tests/hardbc_model.py (autograd through the
ansatz), at the bars tests/test_hip_kernels.py uses for the same precision:
                                   fp32     bf16x3
  fields, max-abs / max|ref|       2e-5     5e-4
  loss, relative                   1e-5     1e-4
  gradient, relative L2            1e-4     1e-4
and the properties of the constraint itself: the boundary plan reproduces its targets, the boundary term's gradient is
exactly zero, predict returns the wall values on the walls, a replayed graph step equals the eager one, and with the
feature off nothing changes."""
import numpy as np
import pytest
import torch

import hardbc_model as hm
from oracle import autograd_ref as ar

pytestmark = pytest.mark.gpu

BARS = {"fp32": dict(field=2e-5, loss=1e-5, grad=1e-4), "bf16x3": dict(field=5e-4, loss=1e-4, grad=1e-4)}
# (L, H, N, Nb, precision, what else the case carries, (forward, reverse sweep) kernels it must reach or None)
CASES = [
    (1, 8, 37, 5, "fp32", "plain", None),
    (4, 50, 1000, 129, "fp32", "ev", None),
    (4, 50, 1000, 129, "bf16x3", "supervised", None),
    (6, 256, 320, 100, "fp32", "plain", ("fwd_wide_kernel", "bwd_wide_kernel")),
    (6, 256, 320, 100, "bf16x3", "plain", ("fwd_bf16_kernel", "bwd_bf16_kernel")),
    (3, 400, 150, 70, "bf16x3", "plain", ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel")),
]


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


def _collocation(N, seed, lo=0.0, hi=1.0):
    """N points (not a tile multiple): the four corners, one point on each wall, the centre, then random ones."""
    rng = np.random.RandomState(seed)
    sx, sy = hm.special_points(lo, hi)
    x = np.concatenate([sx, (lo + (hi - lo) * rng.rand(N - sx.size)).astype(np.float32)])
    y = np.concatenate([sy, (lo + (hi - lo) * rng.rand(N - sy.size)).astype(np.float32)])
    return x, y


def _boundary(Nb):
    return tuple(a.reshape(-1)[:: max(1, 2052 // Nb)][:Nb].astype(np.float32) for a in ar.cavity_boundary())


def _bits_zero(t):
    return not t.cpu().numpy().view(np.uint32).any()


@pytest.mark.parametrize("L,H,N,Nb,prec,extra,kernels", CASES,
                         ids=["%dx%d_%s_%s" % (c[0], c[1], c[4], c[5]) for c in CASES])
def test_constrained_loss_and_gradient_match_the_fp64_model(L, H, N, Nb, prec, extra, kernels):
    eng = _engine_mod()
    dev = torch.device("cuda:0")
    bar = BARS[prec]
    Re, alpha_b, alpha_e, m = 400.0, 10.0, 1.0, 2 + (L % 2)
    ev = extra == "ev"
    flat = _flat(3, L, H, seed=100 + H)
    xb, yb, ub, vb = _boundary(Nb)
    kw, sup, w, flat_e, alpha_s = {}, None, None, None, 0.0
    bc = hm.HardBc(lift_power=m)
    if ev:      # the coordinate map (scale 2, origin -1), SDF-like weights and a trainable entropy net
        L1, H1 = 4, 40
        flat_e = _flat(1, L1, H1, seed=6)
        bc = hm.HardBc(lift_power=m, origin=(-1.0, -1.0), inv_len=0.5)
        kw = dict(flavour="ev", n_hidden_e=L1, hidden_e=H1, alpha_evm=0.05, coord_scale=2.0)
        xb, yb = 2.0 * xb - 1.0, 2.0 * yb - 1.0
        x, y = _collocation(N, H + L, -1.0, 1.0)
        w = (0.3 + np.random.RandomState(9).rand(N)).astype(np.float32)
    else:
        x, y = _collocation(N, H + L)
    if extra == "supervised":       # samples with NaN-masked pressure targets
        rng = np.random.RandomState(11)
        ns = 77
        sup = [rng.rand(ns).astype(np.float32), rng.rand(ns).astype(np.float32), rng.randn(ns).astype(np.float32),
               rng.randn(ns).astype(np.float32), rng.randn(ns).astype(np.float32)]
        sup[4][::3] = np.nan
        alpha_s = 2.0
        kw = dict(alpha_s=alpha_s)
    E = eng.PinnEngine(dev, L, H, Re, alpha_b=alpha_b, alpha_e=alpha_e, precision=prec, **kw)
    E.set_hard_boundary(True, lift_power=m, origin=(bc.x0, bc.y0), inv_len=bc.inv_len)
    E.net.set_flat(torch.tensor(flat))
    if ev:
        E.net_e.set_flat(torch.tensor(flat_e))
        E.e_trainable = True
    E.set_collocation(x, y, weights=w)
    E.set_boundary(xb, yb, ub, vb)
    if sup is not None:
        E.set_supervised(*sup)
    assert E.plan_f.hard_bc()["lift_power"] == m and E.plan_b.hard_bc() is not None
    assert (E.plan_e.hard_bc() is None) if ev else True
    names = E.plan_f.kernel_names()
    if kernels is not None:
        assert names[:2] == kernels
    assert "split" not in names[0] + names[1] and "pipe" not in names[0] + names[1]
    E.loss_and_grad()
    torch.cuda.synchronize()

    model = hm.constrained_net(flat, L, H, bc)
    net_e = vis_t = None
    if ev:
        net_e = ar.RefFCNet(2, 1, 4, 40).double()
        torch.nn.utils.vector_to_parameters(torch.tensor(flat_e, dtype=torch.float64), net_e.parameters())
        vis_t = E.plan_f.vis_t.cpu().numpy().astype(np.float64)
    r = hm.constrained_step(model, x, y, Re, xb, yb, ub, vb, alpha_b=alpha_b, alpha_e=alpha_e, scale=1.0 / bc.inv_len,
                            w=w, net_e=net_e, vis_t=vis_t, sup=sup, alpha_s=alpha_s)
    f = E.plan_f
    for name in ("u", "v", "p", "u_x", "u_y", "v_x", "v_y"):
        err = _rel_max(f.field(name).cpu().numpy(), r["fields"][name])
        print("%s: max-abs / max|ref| = %.3e" % (name, err))
        assert err < bar["field"], name
    for k, ref in enumerate(r["eqs"]):
        err = _rel_max(f.field("eq%d" % (k + 1)).cpu().numpy(), ref)
        print("eq%d: max-abs / max|ref| = %.3e" % (k + 1, err))
        assert err < bar["field"], k
    lt = E.loss_terms()
    loss = float(lt["loss"])
    print("loss %.9e (model %.9e), loss_b %.3e" % (loss, r["loss"], float(lt["loss_b"])))
    assert abs(loss - r["loss"]) < bar["loss"] * r["loss"]
    g = E.grads.cpu().numpy()
    print("gradient rel-L2 = %.3e" % _rel_l2(g, r["grad"]))
    assert _rel_l2(g, r["grad"]) < bar["grad"]
    if ev:
        print("entropy-net gradient rel-L2 = %.3e" % _rel_l2(E.grads_e.cpu().numpy(), r["grad_e"]))
        assert _rel_l2(E.grads_e.cpu().numpy(), r["grad_e"]) < bar["grad"]
    # the constraint itself: the boundary plan reproduces its targets and its term has no gradient at all
    pred = E.plan_b.pred.cpu().numpy()
    print("boundary misfit: %.3e" % max(np.abs(pred[0] - ub).max(), np.abs(pred[1] - vb).max()))
    np.testing.assert_allclose(pred[0], ub, rtol=0, atol=2e-6)
    np.testing.assert_allclose(pred[1], vb, rtol=0, atol=2e-6)
    gb = torch.full_like(E.grads, 7.0)
    eng.grad_reduce(E.net, [E.plan_b], gb)
    torch.cuda.synchronize()
    assert _bits_zero(gb)


def _small_engine(constrain, prec="fp32", seed=3, **kw):
    eng = _engine_mod()
    L, H = 3, 40
    E = eng.PinnEngine(torch.device("cuda:0"), L, H, 400.0, alpha_b=10.0, alpha_e=1.0, precision=prec, **kw)
    if constrain is not None:
        E.set_hard_boundary(**constrain)
    E.net.set_flat(torch.tensor(_flat(3, L, H, seed)))
    return E


def test_term_split_assembly_gives_a_zero_boundary_gradient():
    E = _small_engine(dict(enabled=True))
    x, y = _collocation(300, 1)
    E.set_collocation(x, y)
    E.set_boundary(*_boundary(129))
    E.set_conflict_free_gradients(True)
    E.loss_and_grad()
    torch.cuda.synchronize()
    assert np.isfinite(E.grads.cpu().numpy()).all() and E.grads.abs().max().item() > 0.0     # the zero-norm guard held
    eng = _engine_mod()
    outs = [torch.full_like(E.grads, 7.0) for _ in range(2)]
    eng.grad_reduce_terms(E.net, [[E.plan_f], [E.plan_b], []], outs + [None])
    torch.cuda.synchronize()
    assert _bits_zero(outs[1]) and outs[0].abs().max().item() > 0.0


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_predict_returns_the_wall_values_on_the_walls(prec):
    E = _small_engine(dict(enabled=True, lift_power=3), prec)
    xb, yb, ub, vb = (a.reshape(-1).astype(np.float32) for a in ar.cavity_boundary())
    u, v, p = (t.cpu().numpy() for t in E.predict(xb, yb))
    np.testing.assert_allclose(u, ub, rtol=0, atol=2e-6)
    np.testing.assert_allclose(v, vb, rtol=0, atol=2e-6)
    assert np.isfinite(p).all() and np.abs(p).max() > 0.0
    # inside, the prediction is the ansatz of the unconstrained net's outputs
    F = _small_engine(None, prec)
    x, y = _collocation(200, 2)
    un, vn, pn = (t.cpu().numpy().astype(np.float64) for t in F.predict(x, y))
    uc, vc, pc = (t.cpu().numpy() for t in E.predict(x, y))
    h = hm.point_factors(hm.HardBc(lift_power=3), x.astype(np.float64), y.astype(np.float64))
    np.testing.assert_allclose(uc, h["g"] + h["D"] * un, rtol=0, atol=2e-6 * max(1.0, np.abs(un).max()))
    np.testing.assert_allclose(vc, h["D"] * vn, rtol=0, atol=2e-6 * max(1.0, np.abs(vn).max()))
    np.testing.assert_allclose(pc, pn, rtol=0, atol=2e-6 * max(1.0, np.abs(pn).max()))      # p is the net's own


def test_graph_replay_of_a_constrained_step_equals_the_eager_step(monkeypatch):
    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E = _small_engine(dict(enabled=True))
        x, y = _collocation(300, 5)
        E.set_collocation(x, y)
        E.set_boundary(*_boundary(129))
        for _ in range(3):      # capture, then replays
            E.step(1e-3)
        torch.cuda.synchronize()
        assert len(E._graphs) == (1 if graph else 0)
        return E.net.params.cpu().numpy().copy(), E.plan_f.fields.cpu().numpy().copy()

    p_e, f_e = run(False)
    p_g, f_g = run(True)
    assert np.array_equal(p_e, p_g) and np.array_equal(f_e, f_g)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_feature_off_is_bitwise_the_engine_that_never_heard_of_it(prec):
    def run(constrain):
        E = _small_engine(constrain, prec)
        x, y = _collocation(300, 7)
        E.set_collocation(x, y)
        E.set_boundary(*_boundary(129))
        assert E.plan_f.hard_bc() is None and E.plan_b.hard_bc() is None
        E.loss_and_grad()
        E.adam_step(1e-3)
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (E.grads, E.sums, E.plan_f.fields, E.plan_b.pred, E.net.params)]

    never, off = run(None), run(dict(enabled=False))
    for a, b in zip(never, off):
        assert a.tobytes() == b.tobytes()
    # ... and the constraint is not a no-op
    E = _small_engine(dict(enabled=True), prec)
    x, y = _collocation(300, 7)
    E.set_collocation(x, y)
    E.set_boundary(*_boundary(129))
    E.loss_and_grad()
    torch.cuda.synchronize()
    assert not np.array_equal(E.plan_f.fields.cpu().numpy(), never[2])
