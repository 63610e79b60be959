"""The frozen-sine variants of the role-split, fused and wide role-split sweeps ($PINN_FF_SPLIT=1, DESIGN.md section 7.13,
"Role-split and fused sweeps"): the FF instantiations of fwd_split / bwd_split / fwdbwd_split (hidden 256) and fwd_wsplit /
bwd_wsplit (hidden 288 .. 448), whose forward forms layer 0 by layer0_sine and whose reverse sweep ends at layer 1, and
the layer-1 workgroups of dw_bf16 (layer 0 recomputed from the point) and dw_bf16_wide (the stored 24-bit a-streams).

Method, cases' construction and bars are those of tests/test_fourier_gpu.py, imported from it (build_case, model_step,
make_engine, check_against_model, BARS) - no bar here is new: bf16x3 fields 5e-4, loss 1e-4, gradient 1e-4 against the
fp64 autograd model of tests/fourier_model.py, frequencies of sigma = 2.  Besides the whole-vector gradient bar the
gradient is judged per block (W_l, b_l for l = 1 .. L-1, the output layer), each at 1e-4 relative L2 of that block: a
wrong A operand in dW's layer-1 workgroups moves only W_1, a wrong cut of the reverse sweep only W_1 / b_1.

Shapes: pairs of 32-point tiles (16 for the wide nets); N = 69 is 3 tiles at hidden 256 (a dummy partner and a partial
last tile), 5 at the wide widths; L = 2 makes the whole reverse sweep the one seed phase, which must neither park nor
skip Z-bar_1; the tile-loop rows take N = (2 CUs + 2) x tile + 5, so that two workgroups take a second pair (the
next-tile hook of the new last phase) and the last pair has a dummy partner.

Condition on the inputs (the check of tests/test_fourier_gpu.py's docstring: model_step in fp32 against fp64 must stay
within a quarter of each bar), made on the CPU at sigma = 2 when the cases were settled: 3x256 / 69 (plain and ev),
6x256 / 320, 3x330 / 69, 2x400 / 150, 3x256 / 16 453 and 2x400 / 8 245 gave fields and residuals at most 1.5e-6, loss at
most 1.6e-7, gradient at most 8.3e-7; 2x256 / 69 gave fields 1.0e-6, residuals 1.1e-6, loss 1.9e-8, gradient 6.7e-7.  All
far inside (1.25e-4, 2.5e-5, 2.5e-5), so no case lowers its sigma (the SIGMA table of tests/test_fourier_gpu.py stays empty).

Then: the fused kernel against the two launches bit for bit, the frozen prefix in every gradient vector, layer 0 under
the optimizers, graph replay, the switch unseen by a tanh net, the split plan against the 8-wave plan, mini-batching
(bitwise) and plain bf16 finite.  Each row asserts the plan's kernel names and what its PINN_VERBOSE line says first."""
import functools
import os

import numpy as np
import pytest
import torch

from test_fourier_gpu import BARS, _bits_zero, _flat, _rel_l2, _rel_max, build_case, check_against_model, make_engine, model_step

pytestmark = pytest.mark.gpu

SWITCH = "PINN_FF_SPLIT"
SPLIT = ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
WSPLIT = ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")
EIGHT = ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")
FUSED, TWO, WIDE, PLAIN = ("fused role-split kernel", "role-split kernels, two launches", "wide role-split kernels",
                           "8-wave kernels")
X3 = "bf16x3"


def _env(monkeypatch, fuse=None, switch="1", **more):
    """Every switch unset, then PINN_FF_SPLIT (and PINN_FUSE) as the row has them; PINN_VERBOSE=1 for _built."""
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
    """The engine make() builds, after its collocation plan named `names` and said `path` of its sweeps (the value plans
    of the same net, created after it, say "8-wave kernels")."""
    capfd.readouterr()
    E = make()
    err = capfd.readouterr().err
    said = [line.split("frozen sine sweeps: ")[1] for line in err.splitlines() if "frozen sine sweeps: " in line]
    assert E.plan_f.kernel_names() == names, E.plan_f.kernel_names()
    tail = " (%s=%s)" % (SWITCH, os.environ[SWITCH])
    assert said and said[0] == path + tail and all(s in (path + tail, PLAIN + tail) for s in said), err
    assert "frozen sine first layer: 8-wave kernels" not in err
    i = E.fourier_info()
    assert i["kernels"] == names and i["split"] == int(os.environ[SWITCH])
    return E


def _loop_points(tile):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (2 * cus + 2) * tile + 5


def _n(N, H):
    return _loop_points(32 if H == 256 else 16) if N == "loop" else N


NB = {69: 40, 320: 100, 150: 70}


@functools.lru_cache(maxsize=None)
def _case(L, H, N, extra, prec=X3):
    """The case (tests/test_fourier_gpu.py build_case), built once and shared; nothing writes to it."""
    return build_case(L, H, N, NB.get(N, 100 if H == 256 else 70), prec, extra)


@functools.lru_cache(maxsize=None)
def _model(L, H, N, extra):
    """The fp64 model of a case without the lagged viscosity, computed once."""
    return model_step(_case(L, H, N, extra))


def _blocks(L, H):
    """(name, start, stop) of the trained blocks of the flat gradient: W_l, b_l for l = 1 .. L-1, then the output layer."""
    out, off = [], 3 * H
    for l in range(1, L):
        out.append(("W%d" % l, off, off + H * H)); off += H * H
        out.append(("b%d" % l, off, off + H)); off += H
    out.append(("out", off, off + 3 * H + 3))
    return out


def _check_blocks(E, c, r):
    g, ref, bar = E.grads.cpu().numpy(), r["grad"], BARS[c["prec"]]["grad"]
    blocks = _blocks(c["L"], c["H"])
    assert blocks[-1][2] == g.size == ref.size
    errs = [(name, _rel_l2(g[a:b], ref[a:b])) for name, a, b in blocks]
    print("gradient rel-L2 per block: " + "  ".join("%s %.3e" % e for e in errs))
    for name, err in errs:
        assert err < bar, name


# (L, H, N, what else the case carries, PINN_FUSE, names, what the plan says)
ROWS = [
    (3, 256, 69, "plain", None, SPLIT, FUSED),
    (3, 256, 69, "plain", "0", SPLIT, TWO),
    (2, 256, 69, "plain", None, SPLIT, FUSED),
    (2, 256, 69, "plain", "0", SPLIT, TWO),
    (6, 256, 320, "plain", None, SPLIT, FUSED),
    (3, 256, 69, "ev", None, SPLIT, FUSED),          # 3x256 + 4x40, weights, the coordinate map: vtm_old
    (3, 330, 69, "plain", None, WSPLIT, WIDE),
    (2, 400, 150, "plain", None, WSPLIT, WIDE),
    (3, 256, "loop", "plain", None, SPLIT, FUSED),
    (2, 400, "loop", "plain", None, WSPLIT, WIDE),
]
IDS = ["%dx%d_%s_%s%s" % (r[0], r[1], r[2], r[3], "" if r[4] is None else "_fuse0") for r in ROWS]


@pytest.mark.parametrize("L,H,N,extra,fuse,names,path", ROWS, ids=IDS)
def test_loss_and_gradient_match_the_fp64_model(monkeypatch, capfd, L, H, N, extra, fuse, names, path):
    N = _n(N, H)
    c = _case(L, H, N, extra)
    _env(monkeypatch, fuse, PINN_HBC_SPLIT="0", PINN_PTIME_SPLIT="0")       # (a sine net's plan never looks at those two)
    E = _built(capfd, lambda: make_engine(c), names, path)
    tile = 32 if H == 256 else 16
    assert E.plan_f.npad == -(-N // tile) * tile
    w0 = c["flat"][:2 * H].reshape(H, 2).astype(np.float64)
    print("sigma %g: max |z| = %.1f rad" % (c["sigma"], np.abs(np.outer(c["x"], w0[:, 0]) + np.outer(c["y"], w0[:, 1])).max()))
    E.grads.fill_(7.0)
    E.loss_and_grad()
    torch.cuda.synchronize()
    if extra == "ev":
        vis_t = E.plan_f.vis_t.cpu().numpy().astype(np.float64)
        assert float(np.abs(vis_t).max()) > 0.0
        r = model_step(c, vis_t=vis_t)
    else:
        r = _model(L, H, N, extra)
    check_against_model(E, c, r)
    _check_blocks(E, c, r)


# ---- the fused kernel equals the two launches on the same plan, bit for bit ----
def _evaluated(monkeypatch, capfd, c, fuse, path, names=SPLIT, switch="1"):
    _env(monkeypatch, fuse, switch)
    E = _built(capfd, lambda: make_engine(c), names, path) if switch == "1" else make_engine(c)
    E.loss_and_grad()
    torch.cuda.synchronize()
    f = E.plan_f
    out = dict(fields=f.fields, sums=E.sums, grads=E.grads, loss=E.loss_terms()["loss"])
    if c["extra"] == "ev":
        out.update(vis_t=f.vis_t, vis_t_minus=f.vis_t_minus, grads_e=E.grads_e, ebar=f.ebar)
    return E, {k: torch.as_tensor(v).clone() for k, v in out.items()}


@pytest.mark.parametrize("L,N,extra,prec", [(3, 69, "plain", X3), (3, "loop", "plain", X3), (2, 69, "plain", X3), (3, 69, "ev", X3),
                                            (3, 69, "plain", "bf16")],
                         ids=["3x256_69", "3x256_loop", "2x256_69", "3x256_69_ev", "3x256_69_bf16"])
def test_fused_equals_the_two_launches_bit_for_bit(monkeypatch, capfd, L, N, extra, prec):
    c = _case(L, 256, _n(N, 256), extra, prec)
    _, one = _evaluated(monkeypatch, capfd, c, None, FUSED)
    _, two = _evaluated(monkeypatch, capfd, c, "0", TWO)
    assert sorted(one) == sorted(two) and ("ebar" in one) == (extra == "ev")
    assert torch.isfinite(one["grads"]).all() and float(one["grads"].abs().max()) > 0 and float(one["sums"][:3].min()) > 0
    for k in sorted(one):
        np.testing.assert_array_equal(one[k].cpu().numpy(), two[k].cpu().numpy(), err_msg=k)


# ---- the frozen layer ----
def _frozen_engine(monkeypatch, capfd, H, setup=None):
    L, names, path = (3, SPLIT, FUSED) if H == 256 else (2, WSPLIT, WIDE)
    c = _case(L, H, 69, "supervised")
    _env(monkeypatch)

    def make():
        E = make_engine(c)
        if setup is not None:
            setup(E)
        return E

    E = _built(capfd, make, names, path)
    return E, E.net.params[:3 * H].clone()


@pytest.mark.parametrize("H", [256, 400])
def test_frozen_entries_have_no_bit_set_in_any_gradient_vector(monkeypatch, capfd, H):
    E, _ = _frozen_engine(monkeypatch, capfd, H)
    E.grads.fill_(7.0)
    E.loss_and_grad()
    torch.cuda.synchronize()
    assert _bits_zero(E.grads[:3 * H]) and E.grads[3 * H:].abs().max().item() > 0.0
    for setup, comb in ((lambda e: e.set_loss_balancing(every=1, beta=0.5), "_bal"), (lambda e: e.set_conflict_free_gradients(True), "_cfg")):
        E, _ = _frozen_engine(monkeypatch, capfd, H, setup)
        t = getattr(E, comb)
        t.gb.fill_(7.0); t.gs.fill_(7.0); E.grads.fill_(7.0)
        E.loss_and_grad()
        torch.cuda.synchronize()
        for name, vec in (("g", E.grads), ("g_b", t.gb), ("g_s", t.gs)):
            assert _bits_zero(vec[:3 * H]), (comb, name)
            assert vec[3 * H:].abs().max().item() > 0.0 and bool(torch.isfinite(vec).all()), (comb, name)


@pytest.mark.parametrize("H", [256, 400])
def test_optimizers_leave_layer_0_where_it_is(monkeypatch, capfd, H):
    from nsfnet_amd import schedule

    def setup(e):
        e.set_lr_schedule(schedule.LrSchedule("exponential", gamma=0.99))
        e.set_grad_clipping(0.5)

    E, first = _frozen_engine(monkeypatch, capfd, H, setup)
    rest = E.net.params[3 * H:].clone()
    for _ in range(20):
        E.step(1e-3)
    torch.cuda.synchronize()
    assert torch.equal(E.net.params[:3 * H], first)
    assert not torch.equal(E.net.params[3 * H:], rest) and bool(torch.isfinite(E.net.params).all())
    E.lbfgs_step(lr=1.0, max_iter=3)
    torch.cuda.synchronize()
    assert torch.equal(E.net.params[:3 * H], first)


# ---- graph replay and mini-batching, bitwise ----
@pytest.mark.parametrize("L,H,names,path", [(3, 256, SPLIT, FUSED), (2, 256, SPLIT, FUSED), (2, 400, WSPLIT, WIDE)], ids=["3x256", "2x256", "2x400"])
def test_ten_replayed_graph_steps_equal_ten_eager_ones(monkeypatch, capfd, L, H, names, path):
    c = _case(L, H, 69, "plain")

    def run(graph):
        _env(monkeypatch, NSFNET_GRAPH="1" if graph else "0")
        E = _built(capfd, lambda: make_engine(c), names, path)
        for _ in range(10):
            E.step(1e-3)
        torch.cuda.synchronize()
        assert len(E._graphs) == (1 if graph else 0)
        return E.net.params.cpu().numpy().copy(), E.plan_f.fields.cpu().numpy().copy(), E.grads.cpu().numpy().copy()

    for a, b in zip(run(False), run(True)):
        assert a.tobytes() == b.tobytes()


def test_batch_step_is_a_plain_step_on_the_drawn_points_bitwise(monkeypatch, capfd):
    c = build_case(3, 256, 500, 40, X3, "plain")
    _env(monkeypatch, NSFNET_GRAPH="0")
    E = _built(capfd, lambda: make_engine(c), SPLIT, FUSED)
    E.set_batching(101, seed=11)
    E.step(1e-3)
    params = E.net.params.clone()
    E.loss_and_grad()
    torch.cuda.synchronize()
    f, _ = E.eval_plans()
    assert f.kernel_names() == SPLIT and f.n == 101
    idx = E.batch_indices().cpu().numpy()
    R = make_engine(dict(c, x=c["x"][idx], y=c["y"][idx]))
    assert R.plan_f.kernel_names() == SPLIT
    R.net.set_flat(params.cpu())
    R.loss_and_grad()
    torch.cuda.synchronize()
    assert torch.equal(E.sums, R.sums) and torch.equal(E.grads, R.grads)
    assert torch.equal(f.field("eq1"), R.plan_f.field("eq1"))


# ---- with the option off, and for a tanh net, nothing moves ----
def test_a_tanh_net_does_not_notice_the_switch_or_a_sine_net_beside_it(monkeypatch, capfd):
    c = _case(3, 256, 69, "plain")
    tanh = dict(c, flat=_flat(3, 3, 256, seed=356))

    def run(switch):
        _env(monkeypatch, switch=switch)
        E = make_engine(tanh, fourier=False)
        assert E.net.first_layer == 0 and E.fourier_info() is None and E.plan_f.kernel_names() == SPLIT
        E.loss_and_grad()
        first = [t.cpu().numpy().copy() for t in (E.plan_f.fields, E.grads, E.sums)]
        for _ in range(3):
            E.step(1e-3)
        torch.cuda.synchronize()
        return first + [t.cpu().numpy().copy() for t in (E.plan_f.fields, E.grads, E.net.params)]

    off, on = run(None), run("1")
    _env(monkeypatch)
    S = _built(capfd, lambda: make_engine(c), SPLIT, FUSED)
    S.loss_and_grad()
    torch.cuda.synchronize()
    beside = run("1")
    for a, b, d in zip(off, on, beside):
        assert a.tobytes() == b.tobytes() == d.tobytes()
    assert off[1][:3 * 256].any() and _bits_zero(S.grads[:3 * 256])      # a tanh net's layer 0 is trained as before
    del S


@pytest.mark.parametrize("L,H,N,names,path", [(3, 256, 69, SPLIT, FUSED), (2, 400, 150, WSPLIT, WIDE)], ids=["3x256", "2x400"])
def test_split_plan_agrees_with_the_8_wave_plan_within_the_sum_of_their_bars(monkeypatch, capfd, L, H, N, names, path):
    """Not bit for bit: the 8-wave plan spills fp32 quads, the role-split plans 24-bit ones."""
    c, bar = _case(L, H, N, "plain"), BARS[X3]
    E, new = _evaluated(monkeypatch, capfd, c, None, path, names)
    O, old = _evaluated(monkeypatch, capfd, c, None, None, switch=None)
    assert "split" not in "".join(O.plan_f.kernel_names()) and O.fourier_info()["split"] == 0
    for name in ("u", "v", "p", "u_x", "u_y", "v_x", "v_y", "eq1", "eq2", "eq3"):
        err = _rel_max(E.plan_f.field(name).cpu().numpy(), O.plan_f.field(name).cpu().numpy())
        print("%s: max-abs / max|8-wave| = %.3e" % (name, err))
        assert err < 2 * bar["field"], name
    la, lb = float(new["loss"]), float(old["loss"])
    err = _rel_l2(new["grads"].cpu().numpy(), old["grads"].cpu().numpy())
    print("loss: relative difference %.3e; gradient rel-L2 = %.3e" % (abs(la - lb) / lb, err))
    assert abs(la - lb) < 2 * bar["loss"] * lb and err < 2 * bar["grad"]
    assert not torch.equal(new["grads"], old["grads"])


@pytest.mark.parametrize("L,H,fuse,names,path", [(3, 256, None, SPLIT, FUSED), (3, 256, "0", SPLIT, TWO), (2, 256, None, SPLIT, FUSED),
                                                 (2, 400, None, WSPLIT, WIDE)], ids=["fused", "two_launches", "2x256", "2x400"])
def test_plain_bf16_runs_and_is_finite(monkeypatch, capfd, L, H, fuse, names, path):
    c = _case(L, H, 69, "plain", "bf16")
    _env(monkeypatch, fuse)
    E = _built(capfd, lambda: make_engine(c), names, path)
    for _ in range(3):
        E.step(1e-3)
    torch.cuda.synchronize()
    assert np.isfinite(E.grads.cpu().numpy()).all() and np.isfinite(E.net.params.cpu().numpy()).all()
    assert np.isfinite(E.plan_f.fields.cpu().numpy()).all() and _bits_zero(E.grads[:3 * H])
    assert float(E.grads.abs().max()) > 0.0
