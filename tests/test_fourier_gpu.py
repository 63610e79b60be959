"""The frozen Fourier-feature first layer on the device: loss_and_grad of every 8-wave kernel
family's FF instantiation against the fp64 autograd model of tests/fourier_model.py, at the bars tests/test_hip_kernels.py
and tests/test_hardbc_gpu.py use for the same precision:
                                   fp32     bf16x3
  fields, max-abs / max|ref|       2e-5     5e-4
  loss, relative                   1e-5     1e-4
  gradient, relative L2            1e-4     1e-4
then a looping tile count, the frozen layer under every optimizer and term combiner, the value paths, graph replay and
mini-batching (bitwise), and that a tanh net does not notice a sine net beside it.

The frequencies are drawn with sigma = 2, so |z| reaches tens of radians and the bf16 modes' range reduction works.
Check made when the cases were settled (a straight fp32 torch evaluation of each case's model against the
fp64 one must stay within a quarter of each fp32 bar, so that the fp32 rounding of the sine's argument - the
reference's own error - does not eat the bar): every case stayed inside at sigma = 2 - fields and residuals 0.9e-6 to 1.2e-6 (5e-6 allowed), loss
at most 1.2e-7 (2.5e-6), gradient at most 5.8e-7 (2.5e-5) - so SIGMA below lowers none."""
import ctypes

import numpy as np
import pytest
import torch

import fourier_model as fm
import val_model as vm
from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr

pytestmark = pytest.mark.gpu

BARS = {"fp32": dict(field=2e-5, loss=1e-5, grad=1e-4), "bf16x3": dict(field=5e-4, loss=1e-4, grad=1e-4)}
# (L, H, N, Nb, precision, what else the case carries, (forward, reverse sweep) kernels it must reach or None)
CASES = [
    (2, 8, 37, 5, "fp32", "plain", None),
    (4, 50, 1000, 129, "fp32", "ev", None),
    (4, 50, 1000, 129, "bf16x3", "supervised", None),
    (3, 128, 200, 70, "bf16x3", "cols64", None),
    (3, 256, 320, 100, "fp32", "plain", ("fwd_wide_kernel", "bwd_wide_kernel")),
    (3, 256, 320, 100, "bf16x3", "plain", ("fwd_bf16_kernel", "bwd_bf16_kernel")),
    (3, 400, 150, 70, "bf16x3", "plain", ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel")),
]
IDS = ["%dx%d_%s_%s" % (c[0], c[1], c[4], c[5]) for c in CASES]
# sigma of each case's frequencies: 2 unless the fp32 check of the module docstring asked for less
SIGMA = {}
DEV = "cuda:0"


def _rel_max(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _flat(n_out, L, H, seed):
    return ar.flat_params(ar.seeded_net(n_out, L, H, seed=seed)).numpy().copy()


def _freqs(H, sigma, seed):
    return sigma * np.random.RandomState(seed).randn(H // 2, 2)


def _boundary(Nb):
    return tuple(a.reshape(-1)[:: max(1, 2052 // Nb)][:Nb].astype(np.float32) for a in ar.cavity_boundary())


def _bits_zero(t):
    return not t.detach().cpu().numpy().view(np.uint32).any()


def build_case(L, H, N, Nb, prec, extra):
    """Everything a case feeds the engine and the model (no device needed): the fp32 check runs on it, too."""
    sigma = SIGMA.get((L, H, prec, extra), 2.0)
    B = _freqs(H, sigma, seed=7 + H)
    c = dict(L=L, H=H, N=N, prec=prec, extra=extra, Re=400.0, alpha_b=10.0, alpha_e=1.0, alpha_s=0.0, scale=1.0, B=B, sigma=sigma,
             flat=fm.with_first_layer(_flat(3, L, H, seed=100 + H), H, B), kw={}, w=None, sup=None, flat_e=None)
    rng = np.random.RandomState(H + L)
    xb, yb, ub, vb = _boundary(Nb)
    lo = 0.0
    if extra == "ev":       # the coordinate map (scale 2 on [-1, 1]^2), SDF-like weights and a trainable 4x40 entropy net
        lo = -1.0
        c.update(flat_e=_flat(1, 4, 40, seed=6), scale=2.0, w=(0.3 + np.random.RandomState(9).rand(N)).astype(np.float32),
                 kw=dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05, coord_scale=2.0))
        xb, yb = 2.0 * xb - 1.0, 2.0 * yb - 1.0
    c["x"] = (lo + (1.0 - lo) * rng.rand(N)).astype(np.float32)
    c["y"] = (lo + (1.0 - lo) * rng.rand(N)).astype(np.float32)
    c["bc"] = (xb, yb, ub, vb)
    if extra == "supervised":       # samples with NaN-masked pressure targets
        r2 = np.random.RandomState(11)
        sup = [r2.rand(77).astype(np.float32), r2.rand(77).astype(np.float32), r2.randn(77).astype(np.float32),
               r2.randn(77).astype(np.float32), r2.randn(77).astype(np.float32)]
        sup[4][::3] = np.nan
        c.update(sup=sup, alpha_s=2.0, kw=dict(alpha_s=2.0))
    return c


def model_step(c, dtype=torch.float64, vis_t=None):
    """The case's loss_and_grad by autograd in `dtype` (fp64: the reference; fp32: the check of the module docstring)."""
    model = fm.sine_net(c["flat"], c["L"], c["H"], dtype=dtype)
    net_e = None if c["flat_e"] is None else fm.tanh_net(c["flat_e"], 4, 40, dtype=dtype)
    if dtype == torch.float64:
        return fm.step(model, c["H"], c["x"], c["y"], c["Re"], *c["bc"], alpha_b=c["alpha_b"], alpha_e=c["alpha_e"],
                       scale=c["scale"], w=c["w"], net_e=net_e, vis_t=vis_t, sup=c["sup"], alpha_s=c["alpha_s"])
    # hardbc_model's statement builds fp64 inputs: the fp32 run goes through a model that rounds its input and computes
    # in fp32, returning fp64 so that the loss arithmetic around it stays exact
    class Cast(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def parameters(self, recurse=True):
            return self.m.parameters(recurse)

        def forward(self, X):
            return self.m(X.to(dtype)).double()

    r = fm.hm.constrained_step(Cast(model), c["x"], c["y"], c["Re"], *c["bc"], alpha_b=c["alpha_b"], alpha_e=c["alpha_e"],
                               scale=c["scale"], w=c["w"], net_e=None if net_e is None else Cast(net_e), vis_t=vis_t,
                               sup=c["sup"], alpha_s=c["alpha_s"])
    r["grad"] = fm.freeze(r["grad"], c["H"])
    return r


def make_engine(c, fourier=True):
    from nsfnet_amd import engine as eng
    E = eng.PinnEngine(torch.device(DEV), c["L"], c["H"], c["Re"], alpha_b=c["alpha_b"], alpha_e=c["alpha_e"],
                       precision=c["prec"], **c["kw"])
    E.net.set_flat(torch.tensor(c["flat"]))
    if fourier:
        E.set_fourier_features(frequencies=c["B"])
        assert torch.equal(E.net.params.cpu(), torch.tensor(c["flat"]))      # the same layer 0, bit for bit
    if c["flat_e"] is not None:
        E.net_e.set_flat(torch.tensor(c["flat_e"]))
        E.e_trainable = True
    E.set_collocation(c["x"], c["y"], weights=c["w"])
    E.set_boundary(*c["bc"])
    if c["sup"] is not None:
        E.set_supervised(*c["sup"])
    return E


def check_against_model(E, c, r):
    bar, f, H = BARS[c["prec"]], E.plan_f, c["H"]
    got = lambda name: np.concatenate([p.field(name).cpu().numpy() for _, p in _passes(f)])
    for name in ("u", "v", "p", "u_x", "u_y", "v_x", "v_y"):
        err = _rel_max(got(name), r["fields"][name])
        print("%s: max-abs / max|ref| = %.3e" % (name, err))
        assert err < bar["field"], name
    for k, ref in enumerate(r["eqs"]):
        err = _rel_max(got("eq%d" % (k + 1)), ref)
        print("eq%d: max-abs / max|ref| = %.3e" % (k + 1, err))
        assert err < bar["field"], k
    loss = float(E.loss_terms()["loss"])
    print("loss %.9e (model %.9e): relative %.3e" % (loss, r["loss"], abs(loss - r["loss"]) / r["loss"]))
    assert abs(loss - r["loss"]) < bar["loss"] * r["loss"]
    g = E.grads.cpu().numpy()
    print("gradient rel-L2 = %.3e" % _rel_l2(g, r["grad"]))
    assert _rel_l2(g, r["grad"]) < bar["grad"]
    assert _bits_zero(E.grads[:3 * H]) and E.grads[3 * H:].abs().max().item() > 0.0
    if "grad_e" in r:
        print("entropy-net gradient rel-L2 = %.3e" % _rel_l2(E.grads_e.cpu().numpy(), r["grad_e"]))
        assert _rel_l2(E.grads_e.cpu().numpy(), r["grad_e"]) < bar["grad"]


def _passes(plan):
    from nsfnet_amd import engine as eng
    return eng._passes(plan)


# ---- 5. every family against the fp64 model ----
@pytest.mark.parametrize("L,H,N,Nb,prec,extra,kernels", CASES, ids=IDS)
def test_loss_and_gradient_match_the_fp64_model(L, H, N, Nb, prec, extra, kernels, monkeypatch):
    if extra == "cols64":
        monkeypatch.setenv("PINN_TILE_COLS", "64")
    c = build_case(L, H, N, Nb, prec, extra)
    w0 = c["flat"][:2 * H].reshape(H, 2).astype(np.float64)
    print("sigma %g: max |z| = %.1f rad" % (c["sigma"], np.abs(np.outer(c["x"], w0[:, 0]) + np.outer(c["y"], w0[:, 1])).max()))
    E = make_engine(c)
    names = E.plan_f.kernel_names()
    if kernels is not None:
        assert names[:2] == kernels
    assert "split" not in names[0] + names[1] and "pipe" not in names[0] + names[1]
    assert E.fourier_info()["kind"] == "sine" and (E.net_e is None or E.net_e.first_layer == 0)
    E.loss_and_grad()
    torch.cuda.synchronize()
    vis_t = E.plan_f.vis_t.cpu().numpy().astype(np.float64) if extra == "ev" else None
    check_against_model(E, c, model_step(c, vis_t=vis_t))
    # the boundary plan's predictions are the model's
    assert _rel_max(E.plan_b.pred.cpu().numpy()[:2], _pred(c, c["bc"][0], c["bc"][1])[:2]) < BARS[prec]["field"]


def _pred(c, x, y):
    """(3, n) fp64 predictions of the case's model."""
    out, _ = fm.forward1(fr.unflatten(c["flat"].astype(np.float64), 2, 3, c["L"], c["H"]), np.asarray(x, np.float64),
                         np.asarray(y, np.float64))
    return out.T


# ---- 6. a looping tile count ----
def _grid_bound(L, H, n_probe, prec="fp32"):
    """What the plan says about its grid, from the C ABI without a workspace: the forward-only workspace is the loss
    partials (one row of NLOSS floats per workgroup of the largest forward grid, rounded up to 256 bytes) plus the
    output adjoints (16 bytes per padded point, rounded likewise).  Returns an upper bound within 8 of the grid."""
    from nsfnet_amd import _lib, engine as eng
    lib = _lib.load()
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.pinn_net_create(3, L, H, ctypes.byref(net)), "pinn_net_create")
    _lib.check(lib.pinn_net_set_precision(net, *[eng.PRECISIONS[prec]] * 3), "pinn_net_set_precision")
    _lib.check(lib.pinn_net_set_first_layer(net, 1), "pinn_net_set_first_layer")
    _lib.check(lib.pinn_plan_create(net, n_probe, 4, ctypes.byref(plan)), "pinn_plan_create")
    npad = int(lib.pinn_plan_padded_points(plan))
    fwd = int(lib.pinn_plan_workspace_bytes(plan, 0))
    lib.pinn_plan_destroy(plan); lib.pinn_net_destroy(net)
    return (fwd - (16 * npad + 255) // 256 * 256) // (eng.NLOSS * 4)


def test_looping_tile_count_matches_the_fp64_model():
    """2x32 in fp32 (32-point tiles, several workgroups per CU): an odd tile count above the plan's grid, so some
    workgroups take two tiles and some one; the model is evaluated in passes.  The same bars."""
    L, H = 2, 32
    grid = _grid_bound(L, H, 1 << 22)
    ntiles = grid + 9 + (grid % 2 == 0) - (grid % 2)      # odd and above the grid (the bound is within 8 of it)
    ntiles += 1 - ntiles % 2
    N = 32 * ntiles - 5
    assert _grid_bound(L, H, N) >= grid - 8 and ntiles > grid and ntiles % 2 == 1
    print("grid <= %d, %d tiles, %d points" % (grid, ntiles, N))
    c = build_case(L, H, N, 129, "fp32", "plain")
    E = make_engine(c)
    E.loss_and_grad()
    torch.cuda.synchronize()
    P = fr.unflatten(c["flat"].astype(np.float64), 2, 3, L, H)
    x, y = c["x"].astype(np.float64), c["y"].astype(np.float64)
    r = fm.pde_loss_and_grad(P, x, y, c["Re"], alpha_e=c["alpha_e"], chunk=8192)
    b = fm.bc_loss_and_grad(P, *[np.asarray(a, np.float64) for a in c["bc"]], alpha_b=c["alpha_b"])
    out = r["out"]
    ref = dict(fields=dict(u=out[:, 0, 0], v=out[:, 1, 0], p=out[:, 2, 0], u_x=out[:, 0, 1], u_y=out[:, 0, 2],
                           v_x=out[:, 1, 1], v_y=out[:, 1, 2]), eqs=r["eqs"], grad=r["grad"] + b["grad"],
               loss=c["alpha_e"] * sum(r["sums"]) / N + c["alpha_b"] * sum(b["sums"]) / len(c["bc"][0]))
    check_against_model(E, c, ref)


# ---- 7. the frozen layer ----
def _frozen_engine(setup=None):
    c = build_case(4, 50, 1000, 129, "bf16x3", "supervised")
    E = make_engine(c)
    if setup is not None:
        setup(E)
    return E, c["H"], E.net.params[:3 * c["H"]].clone()


def test_frozen_entries_have_no_bit_set_in_any_gradient_vector():
    E, H, _ = _frozen_engine()
    E.grads.fill_(7.0)
    E.loss_and_grad()
    torch.cuda.synchronize()
    assert _bits_zero(E.grads[:3 * H]) and E.grads[3 * H:].abs().min().item() >= 0.0 and E.grads.abs().max().item() > 0.0
    for setup, comb in ((lambda e: e.set_loss_balancing(every=1, beta=0.5), "_bal"), (lambda e: e.set_conflict_free_gradients(True), "_cfg")):
        E, H, _ = _frozen_engine(setup)
        t = getattr(E, comb)
        t.gb.fill_(7.0); t.gs.fill_(7.0); E.grads.fill_(7.0)
        E.loss_and_grad()
        torch.cuda.synchronize()
        for name, vec in (("g", E.grads), ("g_b", t.gb), ("g_s", t.gs)):
            assert _bits_zero(vec[:3 * H]), (comb, name)
            assert vec[3 * H:].abs().max().item() > 0.0 and bool(torch.isfinite(vec).all()), (comb, name)


@pytest.mark.parametrize("rwf", [False, True], ids=["plain", "rwf"])
def test_optimizers_leave_layer_0_where_it_is(rwf):
    from nsfnet_amd import schedule

    def setup(e):
        if rwf:
            e.set_weight_factorization(mean=0.5, std=0.1, seed=2)
        e.set_lr_schedule(schedule.LrSchedule("exponential", gamma=0.99))
        e.set_grad_clipping(0.5)

    E, H, first = _frozen_engine(setup)
    rest = E.net.params[3 * H:].clone()
    for _ in range(20):
        E.step(1e-3)
    torch.cuda.synchronize()
    if rwf:     # compose rebuilds W0 = fp32(exp(s)) * V0 with V0 = W0 / fp32(exp(s)): a one-off rounding of one ulp at most,
        # after which the frozen (V0, s0, b0) reproduce the same bits at every update
        after1 = E.net.params[:3 * H].clone()
        np.testing.assert_allclose(after1.cpu().numpy(), first.cpu().numpy(), rtol=2.0 ** -23, atol=0)
        assert torch.equal(after1[2 * H:], first[2 * H:])                        # the biases are copied
        E.step(1e-3)
        torch.cuda.synchronize()
        assert torch.equal(E.net.params[:3 * H], after1)
    else:
        assert torch.equal(E.net.params[:3 * H], first)
    assert not torch.equal(E.net.params[3 * H:], rest)
    frozen = E.net.params[:3 * H].clone()
    E.lbfgs_step(lr=1.0, max_iter=3)
    torch.cuda.synchronize()
    assert torch.equal(E.net.params[:3 * H], frozen)


# ---- 8. value paths ----
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_value_paths_match_the_model(prec):
    c = build_case(3, 40, 200, 70, prec, "plain")
    E = make_engine(c)
    rng = np.random.RandomState(4)
    x, y = rng.rand(300).astype(np.float32), rng.rand(300).astype(np.float32)
    got = np.stack([t.cpu().numpy() for t in E.predict(x, y)])
    ref = _pred(c, x, y)
    for k, name in enumerate("uvp"):
        print("predict %s: max-abs / max|ref| = %.3e" % (name, _rel_max(got[k], ref[k])))
        assert _rel_max(got[k], ref[k]) < BARS[prec]["field"]
    E.loss_and_grad()
    torch.cuda.synchronize()
    pb = E.plan_b.pred.cpu().numpy()
    rb = _pred(c, c["bc"][0], c["bc"][1])
    for k in range(2):
        assert _rel_max(pb[k], rb[k]) < BARS[prec]["field"]


def test_validation_on_a_grid_matches_its_numpy_model():
    c = build_case(3, 40, 200, 70, "bf16x3", "plain")
    from nsfnet_amd import engine as eng
    E = eng.PinnEngine(torch.device(DEV), c["L"], c["H"], c["Re"], alpha_b=10.0, precision="bf16x3")
    E.net.set_flat(torch.tensor(c["flat"]))
    E.set_fourier_features(frequencies=c["B"])
    g = np.linspace(0.0, 1.0, 17, dtype=np.float32)
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g))
    tgt = [np.sin(3 * x) * y + 0.5, np.cos(2 * y) * x + 0.5, (0.2 + x * y)]
    tgt = [t.astype(np.float32) for t in tgt]
    E.set_validation(x, y, *tgt, every=5, metric="uv")
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(*c["bc"])
    row = E.validate()
    pred = [t.cpu().numpy() for t in E.predict(x, y)]
    d = vm.direct_errors(pred, tgt)
    for name, want in (("e_u", d[0]), ("e_v", d[1]), ("e_p", d[2]), ("metric", d[4])):
        assert abs(row[name] - want) <= 1e-9 * abs(want), (name, row[name], want)
    ref = _pred(c, x, y)
    for k in range(3):
        assert _rel_max(pred[k], ref[k]) < BARS["bf16x3"]["field"]


# ---- 9. graph replay and mini-batching, bitwise ----
def test_ten_replayed_graph_steps_equal_ten_eager_ones(monkeypatch):
    c = build_case(3, 256, 320, 100, "bf16x3", "plain")

    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E = make_engine(c)
        for _ in range(10):
            E.step(1e-3)
        torch.cuda.synchronize()
        assert len(E._graphs) == (1 if graph else 0)
        return E.net.params.cpu().numpy().copy(), E.plan_f.fields.cpu().numpy().copy(), E.grads.cpu().numpy().copy()

    for a, b in zip(run(False), run(True)):
        assert a.tobytes() == b.tobytes()


def test_batch_step_is_a_plain_step_on_the_drawn_points_bitwise(monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    c = build_case(3, 40, 2000, 129, "bf16x3", "plain")
    E = make_engine(c)
    E.set_batching(384, seed=11)
    E.step(1e-3)
    params = E.net.params.clone()
    E.loss_and_grad()
    torch.cuda.synchronize()
    idx = E.batch_indices().cpu().numpy()
    R = make_engine(dict(c, x=c["x"][idx], y=c["y"][idx]))
    R.net.set_flat(params.cpu())
    R.loss_and_grad()
    torch.cuda.synchronize()
    assert torch.equal(E.sums, R.sums) and torch.equal(E.grads, R.grads)
    f, _ = E.eval_plans()
    assert torch.equal(f.field("eq1"), R.plan_f.field("eq1"))


# ---- 10. with the option off nothing moves ----
def test_a_tanh_net_does_not_notice_a_sine_net_beside_it(monkeypatch):
    """The headline shape's kernels (6x256 in bf16x3, the default fused sweeps) at N = 640: fields and gradient of a tanh
    net bit for bit, before and while a sine net of the same shape is alive and has run in the same process."""
    for k in ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_FUSE", "PINN_TILE_COLS"):
        monkeypatch.delenv(k, raising=False)
    c = build_case(6, 256, 640, 100, "bf16x3", "plain")
    tanh = dict(c, flat=_flat(3, 6, 256, seed=356))

    def run():
        E = make_engine(tanh, fourier=False)
        assert E.net.first_layer == 0 and E.fourier_info() is None
        assert E.plan_f.kernel_names()[:2] == ("fwd_split_kernel", "bwd_split_kernel")
        E.loss_and_grad()
        torch.cuda.synchronize()
        return E.plan_f.fields.cpu().numpy().copy(), E.grads.cpu().numpy().copy(), E.sums.cpu().numpy().copy()

    alone = run()
    S = make_engine(c)
    assert S.plan_f.kernel_names()[:2] == ("fwd_bf16_kernel", "bwd_bf16_kernel")
    S.loss_and_grad()
    torch.cuda.synchronize()
    beside = run()
    for a, b in zip(alone, beside):
        assert a.tobytes() == b.tobytes()
    assert alone[1][:3 * 256].any() and _bits_zero(S.grads[:3 * 256])      # a tanh net's layer 0 is trained as before
    del S
