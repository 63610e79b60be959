"""The constrained role-split, wide role-split and fused sweeps ($PINN_HBC_SPLIT=1): the HBC
instantiations of fwd_split / bwd_split / fwdbwd_split (hidden 256) and fwd_wsplit / bwd_wsplit (hidden 288 .. 448).

They run the point stages of point_stage.h that the constrained 8-wave kernels run, so they are judged as those are,
by the methods of the files that judge those and at their bars - no bar here is new:
  * against the fp64 model at Re = 1 and N = 69, per plane, sum and layer block of the residual gradient alone, the
    descriptor's edges and the Re = 1e-3 planes among the rows (tests/test_hardbc_terms.py: bf16x3 planes 5e-4, sums
    2e-4, gradient block 1e-4); one ev row at width 256 whose inputs meet that file's conditions (a) and (b);
  * where every workgroup repeats its tile loop: an odd tile count with a dummy partner, a partial last tile, some
    workgroups taking a second pair;
  * the fused kernel against the two launches on the same constrained plan, bit for bit, on the quantities of
    tests/test_fused_step.py's _compare - points in [-1, 1]^2 under the coordinate map, since a constrained plan refuses
    that file's scale of 1.3;
  * the walls: u and v at the wall and corner collocation points equal the boundary data to 2e-6
    (tests/test_hardbc_gpu.py);
  * plain bf16 (TERMS == 1) against the emulation of its arithmetic at 4 x the emulation's own noise
    (tests/test_bf16_fast_mode.py), under that file's condition on the inputs;
  * a constrained engine's graph replay against its eager steps, and an unconstrained engine with the switch set
    against one without, bit for bit.
Each row asserts the kernel names and the descriptor its plan reports before it compares.  Measured figures: DESIGN.md
7.10, "Role-split and fused sweeps".
"""
import numpy as np
import pytest
import torch

import hardbc_model as hm
from oracle import autograd_ref as ar

import test_bf16_fast_mode as bm
import test_hardbc_terms as ht
from test_hardbc_terms import EDGE_NETS, EDGES, N, NETS, PLANES
from test_kernel_pairings import X3, _row
from test_residual_term import RE_LAP, SHARE_MIN, _case as _emul_case
from test_tile_loops import BARS, _cus, _rel_max

ON = (("PINN_HBC_SPLIT", "1"),)
UNFUSED = ON + (("PINN_FUSE", "0"),)
SPLIT = ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
WSPLIT = ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")
WALL_BAR = 2e-6           # tests/test_hardbc_gpu.py
_ids = lambda cases: [c["tag"] for c in cases]


def _case(net, env=ON, **kw):
    """A row of test_hardbc_terms' table (bf16x3) with the switch on, naming the role-split kernels of its width."""
    c = ht._case(*net, X3, env=env, **kw)
    wide = c["H"] > 256
    c.update(names=WSPLIT if wide else SPLIT, tile=16 if wide else 32)
    return c


# against the fp64 model, Re = 1: 3x256 fused and as two launches, the wide sweeps at two widths, the descriptor's edges
CASES_RE1 = ([_case(NETS[256]), _case(NETS[256], env=UNFUSED), _case(NETS[330]), _case(NETS[400])] +
             [_case(EDGE_NETS[256], m=m, r=r) for m, r in EDGES])
# Re = 1e-3, planes and sums only
CASES_LAP = [_case(NETS[H], Re=RE_LAP, grad=False) for H in (256, 400)]
CASES = CASES_RE1 + CASES_LAP
# ev at width 256: 3x256 + 4x40 with the coordinate map (origin (-1, -1), inv_len 1/2, scale 2), weights, and alpha_evm
# putting alpha_evm |e| on either side of 20 / Re.  Seed and gain as NETS[256]'s: the conditions below hold for them.
CASE_EV = _case(NETS[256], ev=dict(seed=62, alpha_evm=150.0))


# --------------------------------------------------------------------------------------------------------------------
# CPU: the table, and the conditions on the ev row's inputs (asserted on the fp64 model alone)
# --------------------------------------------------------------------------------------------------------------------
def test_the_table_is_what_the_module_says():
    assert [(c["L"], c["H"], c["names"][0], dict(c["env"]).get("PINN_FUSE")) for c in CASES_RE1[:4]] == [
        (3, 256, "fwd_split_kernel", None), (3, 256, "fwd_split_kernel", "0"), (3, 330, "fwd_wsplit_kernel", None),
        (2, 400, "fwd_wsplit_kernel", None)]
    assert [(c["H"], c["m"], c["r"]) for c in CASES_RE1[4:]] == [(256, m, r) for m, r in EDGES]
    assert [(c["H"], c["Re"], c["grad"]) for c in CASES_LAP] == [(256, RE_LAP, False), (400, RE_LAP, False)]
    assert all(dict(c["env"])["PINN_HBC_SPLIT"] == "1" and c["bar"] == X3 for c in CASES + [CASE_EV])
    assert len({c["tag"] for c in CASES}) == len(CASES)
    # the nets, points and descriptors are rows of test_hardbc_terms' table: its conditions (a) and (b) cover them
    theirs = {ht._key(c) for c in ht.CASES}
    assert all(ht._key(c) in theirs for c in CASES)
    assert ht._key(CASE_EV) not in theirs and (CASE_EV["L"], CASE_EV["H"]) == (3, 256)
    assert ht._bc_of(CASE_EV).inv_len == 0.5 and ht._inputs(CASE_EV)["scale"] == 2.0 and ht._inputs(CASE_EV)["w"] is not None


def test_ev_row_condition_a_the_viscous_term_carries_its_share():
    s = ht._shares(CASE_EV)
    print("[hardbc split] %s viscous share: %s" % (CASE_EV["tag"], " ".join("%s %.2f" % kv for kv in s.items())))
    assert min(s.values()) >= SHARE_MIN, s


def test_ev_row_takes_both_branches_of_the_viscosity_clamp():
    inp = ht._inputs(CASE_EV)
    clamped = CASE_EV["ev"]["alpha_evm"] * np.abs(inp["e"]) > 20.0 / CASE_EV["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()


def test_ev_row_condition_b_an_error_of_one_bf16_term_in_any_of_the_seven_leaves_a_bar():
    out = {t: ht._detected(CASE_EV, t) for t in hm.LAPLACIAN_TERMS}
    print("[hardbc split] %s: %s" % (CASE_EV["tag"], " ".join("%s %.1fx(%s)" % ((t,) + v) for t, v in out.items())))
    assert len(out) == 7
    for t, (ratio, name) in out.items():
        assert ratio > 1.0, (t, ratio, name)


# --------------------------------------------------------------------------------------------------------------------
# GPU: against the fp64 model, and the walls
# --------------------------------------------------------------------------------------------------------------------
def _walls(c, inp, got):
    """u and v at the wall and corner collocation points (the first eight of _points) equal the boundary data: the lid
    profile on the lid, zero elsewhere."""
    bc = ht._bc_of(c)
    x, y = inp["x"][:8].astype(np.float64), inp["y"][:8].astype(np.float64)
    h = hm.point_factors(bc, x, y)
    assert np.abs(h["D"]).max() == 0.0
    lid = (y - bc.y0) * bc.inv_len == 1.0
    X = (x - bc.x0) * bc.inv_len
    data = np.where(lid, 1.0 - np.cosh(bc.r * (X - 0.5)) / np.cosh(0.5 * bc.r), 0.0)
    assert lid.sum() == 3 and data.max() > 0.7 and np.abs(data - h["g"]).max() <= 1e-12
    eu, ev = np.abs(got["fields"]["u"][:8] - data).max(), np.abs(got["fields"]["v"][:8]).max()
    print("[hardbc split] %s walls: u %.2e v %.2e (bar %.0e)" % (c["tag"], eu, ev, WALL_BAR))
    assert eu <= WALL_BAR and ev <= WALL_BAR, (eu, ev)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_constrained_role_split_residual_term_vs_model(monkeypatch, c):
    """ht._run asserts the names, the descriptor and the padded points of the plan before it runs it."""
    inp, got = ht._run(monkeypatch, c)
    _walls(c, inp, got)
    ht._judge(c, got, ht._model(c))


@pytest.mark.gpu
def test_constrained_role_split_residual_term_ev_vs_model(monkeypatch):
    """vis_t is the run's own, so the model run is this case's; both branches of the clamp are taken on the device."""
    c = CASE_EV
    inp, got = ht._run(monkeypatch, c)
    assert _rel_max(got["vtm0"], c["ev"]["alpha_evm"] * np.abs(inp["e"])) <= BARS[c["bar"]]["eq"]
    vis_t = ht._vis_t(c, inp, got["vtm0"])
    np.testing.assert_allclose(got["vis_t"], vis_t, rtol=1e-6)
    clamped = got["vtm0"] > 20.0 / c["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()
    _walls(c, inp, got)
    ht._judge(c, got, ht._model_run(c, inp, vis_t=vis_t))


# --------------------------------------------------------------------------------------------------------------------
# GPU: workgroups that repeat their tile loop
# --------------------------------------------------------------------------------------------------------------------
# an odd tile count (a dummy partner), a partial last tile, more pairs than compute units: some take a second pair
LOOP_N = {"6x256": 32 * 601 - 5, "4x400": 12303}
LOOP_ROWS = [("6x256", ON), ("6x256", UNFUSED), ("4x400", ON)]
_LOOP_MODEL = {}


def _loop_case(shape, env):
    L, H, seed, pts, _ = ht.LOOPS[shape]
    return _case((L, H, seed, 1.0, pts), env=env)


def test_loop_sizes_are_what_the_module_says():
    for shape, tile in (("6x256", 32), ("4x400", 16)):
        n = LOOP_N[shape]
        tiles = -(-n // tile)
        assert tiles % 2 == 1 and n % tile != 0 and 256 < (tiles + 1) // 2 < 2 * 256, (shape, tiles)
        assert _loop_case(shape, ON)["tile"] == tile


@pytest.mark.gpu
@pytest.mark.parametrize("shape,env", LOOP_ROWS, ids=["%s%s" % (s, "" if e == ON else " PINN_FUSE=0") for s, e in LOOP_ROWS])
def test_constrained_role_split_sweeps_loop_vs_model(monkeypatch, shape, env):
    c, n = _loop_case(shape, env), LOOP_N[shape]
    inp = ht._inputs(c, n)
    E = ht._engine(monkeypatch, c, inp)
    E.set_collocation(inp["x"], inp["y"])
    E.set_boundary(*ht._boundary(c))
    assert E.plan_f.kernel_names() == c["names"]
    ht._is_constrained(E.plan_f, c)
    assert E.plan_f.npad == -(-n // c["tile"]) * c["tile"]
    pairs = (E.plan_f.npad // c["tile"] + 1) // 2
    assert _cus() < pairs < 2 * _cus(), (pairs, _cus())
    E.loss_and_grad()
    got = dict(grad=ht._residual_gradient(E, E.plan_f), sums=E.sums.cpu().numpy().astype(np.float64), **ht._planes(E.plan_f, 3))
    del E
    torch.cuda.empty_cache()
    if shape not in _LOOP_MODEL:
        _LOOP_MODEL[shape] = ht._model_run(c, inp)
    _walls(c, inp, got)
    ht._judge(c, got, _LOOP_MODEL[shape], n)


# --------------------------------------------------------------------------------------------------------------------
# GPU: the fused kernel equals the two launches on the same constrained plan, bit for bit
# --------------------------------------------------------------------------------------------------------------------
MAPPED = hm.HardBc(lift_power=2, lid_sharpness=10.0, origin=(-1.0, -1.0), inv_len=0.5)
SCALE = 2.0               # undoes MAPPED.inv_len: the plan's scale check passes


def _switch_on(monkeypatch):
    import os
    for k in list(os.environ):
        if k.startswith("PINN_") or k in ("NSFNET_GRAPH", "NSFNET_CHUNK_POINTS"):
            monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PINN_HBC_SPLIT", "1")


def _plan_pair(L, H, n, prec, ev, seed=11):
    """test_fused_step._plan_pair on a constrained net: two identically prepared plans, points in [-1, 1]^2 with the
    special points in front."""
    from nsfnet_amd import engine as eng
    dev = torch.device("cuda:0")
    net = eng.DeviceNet(3, L, H, dev, prec)
    net.hard_bc = MAPPED.struct()
    net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=seed)))
    x, y, rng = ht._points(n, seed, -1.0, 1.0)
    w = (0.5 + rng.rand(n)).astype(np.float32) if ev else None
    plans = [eng.ResidualPlan(net, x, y, weights=w) for _ in range(2)]
    e = None
    if ev:
        e = torch.tensor(rng.randn(n).astype(np.float32) * 0.1, device=dev)
        vtm = torch.tensor(rng.rand(n).astype(np.float32) * 0.01, device=dev)
        for p in plans:
            p.vis_t_minus = vtm.clone()
    return net, plans, e


def _compare(net, plans, e, ev, Re=1500.0):
    """test_fused_step._compare's quantities at the scale a constrained plan takes."""
    from nsfnet_amd import engine as eng
    c = 2.0 / plans[0].n
    coef = (c, c, c, 0.1 * c if ev else 0.0)
    kw = dict(e=e, vis_t0=0.02 if ev else 0.0, alpha_evm=0.05 if ev else 0.0, scale=SCALE)
    a, b = plans
    for p in plans:
        assert p.kernel_names() == SPLIT
        got = p.hard_bc()
        assert got is not None and (got["kind"], got["lift_power"], got["x0"], got["y0"], got["inv_len"]) == (1, 2, -1.0, -1.0, 0.5)
    a.forward(Re, save=True, **kw)
    a.backward(Re, coef, e=e, scale=SCALE, want_ebar=ev)
    b.forward_backward(Re, coef, want_ebar=ev, **kw)
    ga = torch.empty(net.num_params, dtype=torch.float32, device=net.device)
    gb = torch.empty_like(ga)
    eng.grad_reduce(net, [a], ga)
    eng.grad_reduce(net, [b], gb)
    torch.cuda.synchronize()
    assert torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    assert torch.equal(a.sums, b.sums)
    assert torch.equal(a.fields, b.fields)
    assert torch.equal(a.vis_t, b.vis_t)
    assert torch.equal(ga, gb)
    if ev:
        assert float(a.vis_t.abs().max()) > 0
        assert torch.equal(a.vis_t_minus, b.vis_t_minus)
        assert torch.equal(a.ebar, b.ebar)
    # the constraint is on: the wall points carry the boundary data
    u, v = a.field("u")[:8].cpu().numpy().astype(np.float64), a.field("v")[:8].cpu().numpy().astype(np.float64)
    g = hm.point_factors(MAPPED, a.x[:8].cpu().numpy().astype(np.float64), a.y[:8].cpu().numpy().astype(np.float64))["g"]
    assert np.abs(u - g).max() <= WALL_BAR and np.abs(v).max() <= WALL_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("n", [70, 32 * 5, 32 * 601 - 5])
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_constrained_fused_equals_the_two_launches(monkeypatch, prec, n):
    _switch_on(monkeypatch)
    net, plans, e = _plan_pair(6, 256, n, prec, ev=False)
    _compare(net, plans, e, ev=False)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_constrained_fused_equals_the_two_launches_shallow(monkeypatch, prec, L):
    _switch_on(monkeypatch)
    net, plans, e = _plan_pair(L, 256, 32 * 77 + 9, prec, ev=False)
    _compare(net, plans, e, ev=False)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_constrained_fused_equals_the_two_launches_ev_inputs(monkeypatch, prec):
    _switch_on(monkeypatch)
    net, plans, e = _plan_pair(6, 256, 32 * 311 + 17, prec, ev=True)
    _compare(net, plans, e, ev=True)


# --------------------------------------------------------------------------------------------------------------------
# plain bf16 (TERMS == 1) against the emulation of its arithmetic: the method of test_bf16_fast_mode's constrained rows
# --------------------------------------------------------------------------------------------------------------------
B16 = bm.B16
# (L, H, net seed, points seed): bm.HBC_NETS' rows; the condition below holds for them on the role-split spill formats
CASES_B16 = [_emul_case(*bm.HBC_NETS[256], _row(B16, SPLIT, 32, ON)), _emul_case(*bm.HBC_NETS[400], _row(B16, WSPLIT, 16, ON))]


@pytest.mark.parametrize("c", CASES_B16, ids=_ids(CASES_B16))
def test_the_plain_bf16_bar_is_four_times_sharper_than_the_format_error(c):
    """A condition on the inputs, not a measurement (bm.test_the_constrained_bar_is_four_times_sharper_...): 4 x noise
    <= format / 4 on every judged quantity, with the role-split kernels' spill format in the emulation."""
    assert bm._emul_options(c["row"]["names"])["spill"] == "p24" and bm._emul_options(c["row"]["names"])["out"] == "fp32"
    noise, fmt = bm._hbc_noise(c), bm._hbc_format(c)
    print("[hardbc split] plain bf16 %s noise %s | format %s | bar / format %s" % (
        c["tag"], " ".join("%s %.1e" % (q, noise[q]) for q in bm.QS), " ".join("%s %.1e" % (q, fmt[q]) for q in bm.QS),
        " ".join("%s %.3f" % (q, bm.FACTOR * noise[q] / fmt[q]) for q in bm.QS)))
    for q in bm._conditioned(c):
        assert noise[q] > 0.0 and bm.FACTOR * bm.FACTOR * noise[q] <= fmt[q], (q, noise[q], fmt[q])
    r, r0 = bm._hbc_model(c), bm._hbc_model(c, 1.0e30)
    assert min(_rel_max(r0["eqs"][k], r["eqs"][k]) for k in (0, 1)) >= SHARE_MIN


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES_B16, ids=_ids(CASES_B16))
def test_constrained_plain_bf16_role_split_kernels_vs_their_arithmetic(monkeypatch, c):
    row, inp = c["row"], bm._inputs(c)
    eng, E = bm._engine(monkeypatch, c["L"], c["H"], c["Re"], row["prec"], row["env"], inp["flat"], inp["x"], inp["y"],
                        bm._boundary(), constrain=True)
    assert E.plan_f.kernel_names() == row["names"] and E.plan_f.hard_bc() is not None
    assert E.plan_f.npad == -(-bm.N // row["tile"]) * row["tile"]
    E.loss_and_grad()
    got = dict(grad=bm._alone(eng, E, E.plan_f), sums=list(E.sums.cpu().numpy().astype(np.float64)[:3]),
               eqs=[E.plan_f.field(k).cpu().numpy().astype(np.float64) for k in ("eq1", "eq2", "eq3")])
    del E
    torch.cuda.empty_cache()
    ref, emu, noise, fmt = bm._hbc_model(c), bm._hbc_emul(c), bm._hbc_noise(c), bm._hbc_format(c)
    bar = {q: bm.FACTOR * noise[q] for q in bm.QS}
    d, blocks = bm._dist(c, got, emu, ref)
    far, _ = bm._dist(c, got, ref, ref)
    print("[hardbc split] plain bf16 %s: from the emulation %s | bar %s | format %s | from the model %s" % (
        c["tag"], " ".join("%s %.2e" % (q, d[q]) for q in bm.QS), " ".join("%.1e" % bar[q] for q in bm.QS),
        " ".join("%.1e" % fmt[q] for q in bm.QS), " ".join("%.1e" % far[q] for q in bm.QS)))
    for q in bm.QS:
        assert d[q] <= bar[q], (q, d[q], bar[q], blocks if q == "grad" else None)
    for q in ("eq", "sums"):        # the forward role really ran one term (triangle inequality)
        assert far[q] >= fmt[q] - bar[q], (q, far[q], fmt[q], bar[q])


# --------------------------------------------------------------------------------------------------------------------
# GPU: the engine
# --------------------------------------------------------------------------------------------------------------------
def _engine_steps(constrain, steps=2):
    from nsfnet_amd import engine as eng
    E = eng.PinnEngine(torch.device("cuda:0"), 6, 256, 400.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3")
    if constrain:
        E.set_hard_boundary(True)
    E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=21)))
    x, y, _ = ht._points(320, 5)
    E.set_collocation(x, y)
    E.set_boundary(*(a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary()))
    assert E.plan_f.kernel_names() == SPLIT and (E.plan_f.hard_bc() is not None) == constrain
    for _ in range(steps):
        E.step(1e-3)
    torch.cuda.synchronize()
    out = [t.clone() for t in (E.net.params, E.sums, E.plan_f.fields)], len(E._graphs)
    del E
    torch.cuda.empty_cache()
    return out


@pytest.mark.gpu
def test_constrained_engine_graph_replay_equals_eager(monkeypatch):
    """6x256, 320 points, boundary set, the switch on: two Adam steps captured and replayed equal the eager ones."""
    _switch_on(monkeypatch)
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    eager, graphs = _engine_steps(True)
    assert graphs == 0
    monkeypatch.setenv("NSFNET_GRAPH", "1")
    replay, graphs = _engine_steps(True)
    assert graphs == 1
    for a, b in zip(eager, replay):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_unconstrained_engine_never_looks_at_the_switch(monkeypatch):
    _switch_on(monkeypatch)
    on, _ = _engine_steps(False)
    monkeypatch.delenv("PINN_HBC_SPLIT")
    off, _ = _engine_steps(False)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
