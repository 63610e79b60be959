"""The hard-wall point stages judged per term, width and precision against the fp64 model.

tests/test_hardbc_gpu.py compares the constrained step at Re = 400 and judges the whole gradient vector.  The
Laplacian stream enters the loss with weight nu only, and the constrained stages add seven terms of that kind:
    forward    Lap c = Lap g + Lap D N + 2 (D_X N_X + D_Y N_Y) + D Lap N          (hardbc_model.FORWARD_TERMS)
    transpose  N_ += Lap D a_D,   N_X_ += 2 D_X a_D (Y alike),   N_D_ = D a_D     (hardbc_model.TRANSPOSE_TERMS)
At Re = 400 a 2^-8 relative error of any of them moves the whole gradient by 6e-8 .. 5e-6: `D a_D` or `D Lap N` could
be missing altogether and the 1e-4 bar would hold (test_control_c_... records that).  Here, as in
tests/test_residual_term.py for the unconstrained kernels:
  * Re = 1 (and Re = 1e-3 for the planes), N = 69 points: three 32-point tiles with a ragged last one, five 16-point
    tiles; the four corners, a point on each wall and the centre are among them;
  * the gradient is the residual term's alone (grad_reduce over plan_f) and judged per layer weight and bias block
    (_block_errs / GRAD_BAR of test_residual_term.py); the planes u, v, u_x .. v_y, eq1..3 and the three sums are judged
    at BARS of test_tile_loops.py.  No bar is new and none comes from a kernel's output;
  * the reference is hardbc_model.constrained_fwdmode (fr.forward4 -> the closed-form map -> fr.residuals -> the seeds
    -> the transpose -> fr.backward4), pinned on the CPU to the autograd statement of the ansatz at 1e-10.
Rows: fp32 and bf16x3 at ten widths from 8 to 512 (every launcher's width switch between them, the shipped ev shape's
96 among them), the 64-column bf16 tiles, three mixed precision triples at 256 and 400, an ev row with the coordinate
map, and the descriptor's edges (lift_power 1 and 8, lid_sharpness 4 and 25).  Further down: value mode with D != 0
per family value kernel, constrained workgroups that repeat their tile loop, and the chunked, forward-only and
batch-gathered plans.

The CPU tests keep the table honest: the model pins; every row resolves, constrained, to the kernels and the workspace
it names; every net carries its viscous share; and per row and term a 2^-8 error leaves a bar of that row's precision
(DETECT holds the exceptions: the smallest power of two that does).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import hardbc_model as hm
from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr

from test_tile_loops import (BARS, _cus, _net, _rel_l2, _rel_max, bpc_max, families_of, geometry, loop_violations,
                             pick_n)
from test_kernel_pairings import CODE, F32, X3
from test_residual_term import EPS8, GRAD_BAR, RE_LAP, SHARE_MIN, SHARE_MIN_LAP, _block_errs
from test_value_loops import PRED_BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import plan_census  # noqa: E402

N = 69
PLANES = ("u", "v", "u_x", "u_y", "v_x", "v_y")
# what a constrained plan resolves as: the 8-wave families
EIGHT_WAVE = {"PINN_SCHED": "0", "PINN_WSPLIT": "0", "PINN_FUSE": "0"}


# --------------------------------------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------------------------------------
def _hp(H):
    return (H + 31) // 32 * 32


def _family(H, p):
    """Kernel family of one sweep (or dW) of a constrained plan from its own precision."""
    if p == F32:
        return "_wide" if _hp(H) >= 256 else ""
    return "_bf16_wide" if _hp(H) > 256 else "_bf16"


def _names(H, triple):
    """A constrained plan's kernel triple.  Hidden 256 in a mixed triple: the fp32 members are the 128-column kernels
    (fwd / bwd / dw), which share the 32-point tile of the bf16 ones."""
    mixed = len(set(triple)) > 1
    fam = [("" if mixed and _hp(H) == 256 and p == F32 else _family(H, p)) for p in triple]
    return tuple("%s%s_kernel" % (k, f) for k, f in zip(("fwd", "bwd", "dw"), fam))


def _tile(H, triple, env):
    if dict(env).get("PINN_TILE_COLS") == "64" or _hp(H) > 256:
        return 16
    return 16 if _hp(H) == 256 and set(triple) == {F32} else 32


def _case(L, H, seed, gain, pts, prec, Re=1.0, env=(), ev=None, m=2, r=10.0, grad=True):
    triple = tuple(prec.split(",")) if "," in prec else (prec,) * 3
    tag = "%dx%d%s %s%s Re=%g m=%d r=%g" % (L, H, "+4x40 ev" if ev else "", prec,
                                           "".join(" %s=%s" % kv for kv in env), Re, m, r)
    return dict(L=L, H=H, seed=seed, gain=gain, pts=pts, prec=prec, triple=triple, env=tuple(env), Re=Re, ev=ev, m=m,
                r=r, grad=grad, tag=tag, names=_names(H, triple), tile=_tile(H, triple, env),
                bar=F32 if set(triple) == {F32} else X3)


# (L, H, net seed, layer-0 weight gain, points seed): shallow nets as test_residual_term.NARROW / WIDE; seed and gain
# chosen so that the conditions (a) and (b) of the CPU tests hold - never anything else
NETS = {
    8: (1, 8, 153, 2.0, 31), 16: (2, 16, 153, 1.0, 32), 50: (3, 50, 153, 2.0, 33), 80: (3, 80, 155, 2.0, 34),
    128: (3, 128, 154, 2.0, 35), 200: (3, 200, 155, 1.0, 36), 256: (3, 256, 154, 2.0, 37), 330: (3, 330, 174, 2.0, 38),
    400: (2, 400, 173, 1.0, 39), 512: (2, 512, 172, 2.0, 40),
}
CASES_WIDTH = [_case(*NETS[H], p) for H in sorted(NETS) for p in (F32, X3)]
CASES_COLS64 = [_case(*NETS[H], X3, env=(("PINN_TILE_COLS", "64"),)) for H in (128, 256)]
MIXED = ("fp32,bf16x3,bf16x3", "bf16x3,fp32,bf16x3", "bf16x3,bf16x3,fp32")
CASES_MIXED = [_case(*NETS[H], p) for H in (256, 400) for p in MIXED]
# ev: 4x50 + 4x40 with the coordinate map (origin (-1, -1), inv_len 1/2, scale 2), weights, and alpha_evm putting
# alpha_evm |e| on either side of 20 / Re (test_residual_term.CASES_EV)
CASES_EV = [_case(4, 50, 161, 2.0, 41, F32, ev=dict(seed=62, alpha_evm=150.0))]
# the descriptor's edges: lift_power 1 (the m (m-1) Y^(m-2) coefficient is zero, pm1 = 1) and 8 (six multiplies),
# lid_sharpness 4 and 25
EDGES = ((1, 4.0), (8, 25.0), (1, 25.0), (8, 4.0))
EDGE_NETS = {50: (3, 50, 154, 2.0, 33), 256: (3, 256, 158, 2.0, 37)}       # seeds at which (b) holds for all four pairs
CASES_EDGE = [_case(*EDGE_NETS[H], p, m=m, r=r) for H, p in ((50, F32), (256, X3)) for m, r in EDGES]
# Re = 1e-3, planes and sums only: eq1 / eq2 are the Laplacian planes to 1e-3.  One row per forward kernel name.
CASES_LAP = [_case(*NETS[H], p, Re=RE_LAP, grad=False) for H, p in ((50, F32), (256, F32), (50, X3), (400, X3))]
CASES_RE1 = CASES_WIDTH + CASES_COLS64 + CASES_MIXED + CASES_EV + CASES_EDGE
CASES = CASES_RE1 + CASES_LAP
_ids = lambda cases: [c["tag"] for c in cases]

# (b): the smallest relative error of a term, a power of two, that leaves a bar of the row's precision where 2^-8 does
# not, for every input among {seeds, Re 1 / 1e-3, gain 1-3, depth <= 3} tried: {(bar, term): exponent}.
DETECT = {}


# --------------------------------------------------------------------------------------------------------------------
# inputs and the model
# --------------------------------------------------------------------------------------------------------------------
def _bc_of(c):
    if c["ev"]:
        return hm.HardBc(lift_power=c["m"], lid_sharpness=c["r"], origin=(-1.0, -1.0), inv_len=0.5)
    return hm.HardBc(lift_power=c["m"], lid_sharpness=c["r"])


def _points(n, seed, lo=0.0, hi=1.0):
    """n points: the four corners, one point on each wall, the centre, then random ones (and the generator)."""
    rng = np.random.RandomState(seed)
    sx, sy = hm.special_points(lo, hi)
    x = np.concatenate([sx, (lo + (hi - lo) * rng.rand(n - sx.size)).astype(np.float32)])
    y = np.concatenate([sy, (lo + (hi - lo) * rng.rand(n - sy.size)).astype(np.float32)])
    return x, y, rng


def _flat(L, H, seed, gain):
    flat = _net(L, H, seed)
    flat[:2 * H] *= np.float32(gain)        # layer_0.weight
    return flat


def _inputs(c, n=N):
    ev = c["ev"]
    x, y, rng = _points(n, c["pts"], *((-1.0, 1.0) if ev else (0.0, 1.0)))
    out = dict(flat=_flat(c["L"], c["H"], c["seed"], c["gain"]), x=x, y=y, w=None, scale=1.0, flat_e=None, e=None, Pe=None)
    if ev:
        out.update(w=(0.3 + rng.rand(n)).astype(np.float32), scale=2.0, flat_e=_net(4, 40, ev["seed"], n_out=1))
        out["Pe"] = fr.unflatten(out["flat_e"].astype(np.float64), 2, 1, 4, 40)
        out["e"] = fr.forward1(out["Pe"], x.astype(np.float64), y.astype(np.float64))[0][:, 0]
    return out


def _vis_t(c, inp, vtm=None):
    if not c["ev"]:
        return None
    vtm = c["ev"]["alpha_evm"] * np.abs(inp["e"]) if vtm is None else vtm
    return np.minimum(np.float32(20.0 / c["Re"]), vtm)


def _model_run(c, inp, Re=None, vis_t=None, rel=None, chunk=8192, factor_dtype=np.float64):
    P = fr.unflatten(inp["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
    kw = {}
    if c["ev"]:
        kw = dict(vis_t=None if vis_t is None else np.asarray(vis_t, np.float64), w=inp["w"].astype(np.float64),
                  scale=inp["scale"], params_e=inp["Pe"])
    return hm.constrained_fwdmode(P, _bc_of(c), inp["x"], inp["y"], c["Re"] if Re is None else Re, rel=rel, chunk=chunk,
                                  factor_dtype=factor_dtype, **kw)


_CACHE = {}


def _key(c):
    return (c["L"], c["H"], c["seed"], c["gain"], c["pts"], c["Re"], c["m"], c["r"],
            None if not c["ev"] else tuple(sorted(c["ev"].items())))


def _model(c, what="ref"):
    """Model runs of a case's net, points, Re and descriptor, shared by the rows that differ only in kernels: 'ref',
    'inviscid' (Re = 1e30, no vis_t), 'fp32' (the point factors computed in fp32), or a term of
    hm.LAPLACIAN_TERMS (that term off by 2^-8), or (term, exponent)."""
    k = _key(c) + (what,)
    if k not in _CACHE:
        inp = _inputs(c)
        vt = _vis_t(c, inp)
        if what == "ref":
            _CACHE[k] = _model_run(c, inp, vis_t=vt)
        elif what == "inviscid":
            _CACHE[k] = _model_run(c, inp, Re=1.0e30, vis_t=None if vt is None else 0.0 * vt)
        elif what == "fp32":
            _CACHE[k] = _model_run(c, inp, vis_t=vt, factor_dtype=np.float32)
        else:
            term, ex = what if isinstance(what, tuple) else (what, -8)
            _CACHE[k] = _model_run(c, inp, vis_t=vt, rel={term: 2.0 ** ex})
    return _CACHE[k]


def _nets(cases):
    seen = {}
    for c in cases:
        seen.setdefault(_key(c), c)
    return list(seen.values())


def _errs(c, got, ref):
    """Every judged quantity of a row as {name: (error, bar)}: the planes and eq planes (max-abs / max|ref|), the sums
    (relative) and, where the row judges it, the worst layer block of the residual gradient (and the entropy net's)."""
    bar, gbar = BARS[c["bar"]], GRAD_BAR[c["bar"]]
    out = {k: (_rel_max(got["fields"][k], ref["fields"][k]), bar["eq"]) for k in PLANES}
    for k, q in enumerate(got["eqs"]):
        out["eq%d" % (k + 1)] = (_rel_max(q, ref["eqs"][k]), bar["eq"])
    nq = len(got["eqs"])
    out["sums"] = (_rel_max(np.asarray(got["sums"][:nq], np.float64), np.asarray(ref["sums"])), bar["sums"])
    if c["grad"]:
        out["grad_r"] = (max(_block_errs(got["grad"], ref["grad"], 3, c["L"], c["H"])), gbar)
        if c["ev"]:
            out["grad_e"] = (max(_block_errs(got["grad_e"], ref["grad_e"], 1, 4, 40)), gbar)
    return out


def _worst(errs):
    """The judged quantity furthest out, as (error / bar, name)."""
    return max((e / b, k) for k, (e, b) in errs.items())


# --------------------------------------------------------------------------------------------------------------------
# CPU: the model pins
# --------------------------------------------------------------------------------------------------------------------
def _pin_case(ev, n=40):
    L, H = 3, 20
    flat = _net(L, H, 7).astype(np.float64)
    rng = np.random.RandomState(5)
    xb, yb, ub, vb = (a.reshape(-1)[::64] for a in ar.cavity_boundary())
    if not ev:
        bc = hm.HardBc(lift_power=3, lid_sharpness=7.0)
        sx, sy = hm.special_points()
        x, y = np.concatenate([sx, rng.rand(n)]), np.concatenate([sy, rng.rand(n)])
        return dict(L=L, H=H, flat=flat, bc=bc, x=x, y=y, kw={}, step={}, bnd=(xb, yb, ub, vb))
    bc = hm.HardBc(lift_power=2, origin=(-1.0, -1.0), inv_len=0.5)
    sx, sy = hm.special_points(-1.0, 1.0)
    x, y = np.concatenate([sx, 2 * rng.rand(n) - 1]), np.concatenate([sy, 2 * rng.rand(n) - 1])
    flat_e = _net(2, 8, 9, n_out=1).astype(np.float64)
    net_e = ar.RefFCNet(2, 1, 2, 8).double()
    torch.nn.utils.vector_to_parameters(torch.tensor(flat_e), net_e.parameters())
    w, vt = 0.5 + rng.rand(x.size), 0.3 * rng.rand(x.size)
    return dict(L=L, H=H, flat=flat, bc=bc, x=x, y=y, bnd=(2 * xb - 1, 2 * yb - 1, ub, vb),
                kw=dict(vis_t=vt, w=w, scale=2.0, params_e=fr.unflatten(flat_e, 2, 1, 2, 8)),
                step=dict(vis_t=vt, w=w, scale=2.0, net_e=net_e))


@pytest.mark.parametrize("ev", [False, True], ids=["plain", "ev_mapped"])
@pytest.mark.parametrize("chunk", [8192, 7, 1])
def test_forward_mode_model_equals_autograd_through_the_ansatz(ev, chunk):
    """constrained_fwdmode against constrained_step to 1e-10 on fields, sums and gradient, in one pass and chunked."""
    p = _pin_case(ev)
    r = hm.constrained_step(hm.constrained_net(p["flat"], p["L"], p["H"], p["bc"]), p["x"], p["y"], 1.0, *p["bnd"],
                            alpha_b=0.0, alpha_e=1.3, **p["step"])
    P = fr.unflatten(p["flat"], 2, 3, p["L"], p["H"])
    m = hm.constrained_fwdmode(P, p["bc"], p["x"], p["y"], 1.0, alpha_e=1.3, chunk=chunk, **p["kw"])
    for k in PLANES + ("p", "u_d", "v_d", "p_x", "p_y"):
        assert _rel_max(m["fields"][k], r["fields"][k]) <= 1e-10, k
    assert len(m["eqs"]) == len(r["eqs"]) == (4 if ev else 3)
    for a, b in zip(m["eqs"], r["eqs"]):
        assert _rel_max(a, b) <= 1e-10
    assert _rel_max(np.asarray(m["sums"]), np.asarray(r["sums_eq"])) <= 1e-10
    assert _rel_max(m["grad"], r["grad"]) <= 1e-10
    assert max(_block_errs(m["grad"], r["grad"], 3, p["L"], p["H"])) <= 1e-10
    if ev:
        assert _rel_max(m["grad_e"], r["grad_e"]) <= 1e-10
    else:
        assert "grad_e" not in m


@pytest.mark.parametrize("chunk", [8192, 11])
def test_value_mode_model_equals_autograd_through_the_ansatz(chunk):
    """constrained_value against the supervised term of constrained_step (NaN-masked p) to 1e-10."""
    p = _pin_case(False)
    rng = np.random.RandomState(3)
    n = p["x"].size
    sup = [p["x"], p["y"], rng.randn(n), rng.randn(n), rng.randn(n)]
    sup[4][::3] = np.nan
    n_p = int(np.isfinite(sup[4]).sum())
    r = hm.constrained_step(hm.constrained_net(p["flat"], p["L"], p["H"], p["bc"]), [0.3], [0.6], 1.0, *p["bnd"],
                            alpha_b=0.0, alpha_e=0.0, sup=sup, alpha_s=1.7)
    P = fr.unflatten(p["flat"], 2, 3, p["L"], p["H"])
    coef = (2 * 1.7 / n, 2 * 1.7 / n, 2 * 1.7 / n_p)
    m = hm.constrained_value(P, p["bc"], p["x"], p["y"], targets=sup[2:], coef=coef, chunk=chunk)
    loss_s = (m["sums"][0] + m["sums"][1]) / n + m["sums"][2] / n_p
    assert abs(loss_s - r["loss_s"]) <= 1e-10 * r["loss_s"] and m["sums"][3] == n_p
    assert _rel_max(m["grad"], r["grad"]) <= 1e-10
    with torch.no_grad():
        model = hm.constrained_net(p["flat"], p["L"], p["H"], p["bc"])
        want = model(torch.cat((hm._col(p["x"]), hm._col(p["y"])), dim=1)).numpy()
    assert _rel_max(m["pred"], want) <= 1e-10
    # the wall points carry no gradient: D = 0 there
    walls = slice(0, 8)
    t = [q.copy() for q in sup[2:]]
    for q in t[:2]:
        q[walls] += 5.0
    m2 = hm.constrained_value(P, p["bc"], p["x"], p["y"], targets=[t[0], t[1], sup[4]], coef=coef, chunk=chunk)
    assert _rel_max(m2["grad"], m["grad"]) <= 1e-12


def test_a_relative_error_of_each_term_is_what_the_model_applies():
    """rel = {term: eps} scales that term alone: the Laplacian the map returns, or the transpose's output, moves by
    eps times the term and nothing else moves."""
    rng = np.random.RandomState(1)
    x, y = rng.rand(30), rng.rand(30)
    h = hm.point_factors(hm.HardBc(lift_power=3), x, y)
    n = [rng.randn(30) for _ in range(4)]
    base = hm.transform_streams(h, *n, lift=True)
    terms = dict(lap_g=h["gd"], lapD_N=h["Dd"] * n[0], cross=2.0 * (h["Dx"] * n[1] + h["Dy"] * n[2]), D_lapN=h["D"] * n[3])
    assert tuple(terms) == hm.FORWARD_TERMS
    for k, t in terms.items():
        got = hm.transform_streams(h, *n, lift=True, rel={k: EPS8})
        for a, b in zip(got[:3], base[:3]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_allclose(got[3] - base[3], EPS8 * t, rtol=0, atol=1e-13)
    assert np.abs(hm.transform_streams(h, *n, lift=False, rel={"lap_g": 1.0})[3] - hm.transform_streams(h, *n, lift=False)[3]).max() == 0
    base = hm.transpose_streams(h, *n)
    moved = dict(t_lapD=(h["Dd"] * n[3], 0, 0, 0), t_cross=(0, 2.0 * h["Dx"] * n[3], 2.0 * h["Dy"] * n[3], 0),
                 t_D=(0, 0, 0, h["D"] * n[3]))
    assert tuple(moved) == hm.TRANSPOSE_TERMS and hm.LAPLACIAN_TERMS == hm.FORWARD_TERMS + hm.TRANSPOSE_TERMS
    for k, t in moved.items():
        got = hm.transpose_streams(h, *n, rel={k: EPS8})
        for a, b, d in zip(got, base, t):
            np.testing.assert_allclose(a - b, EPS8 * d, rtol=0, atol=1e-13)


# --------------------------------------------------------------------------------------------------------------------
# CPU: the table against the library, without a device
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def _constrained_census(lib, case, bc):
    """plan_census.run_case's row for the same case created constrained (pinn_plan_create_constrained)."""
    H, L, prec, streams, n, env = case
    old = {k: os.environ.pop(k, None) for k in plan_census.SWITCHES}
    os.environ.update(env)
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        assert lib.pinn_net_create(3, L, H, ctypes.byref(net)) == 0, lib.pinn_last_error()
        assert lib.pinn_net_set_precision(net, *prec) == 0, lib.pinn_last_error()
        rc = lib.pinn_plan_create_constrained(net, n, streams, ctypes.byref(bc), ctypes.byref(plan))
        if rc != 0:
            return [plan_census.key(case), rc, lib.pinn_last_error().decode()]
        row = [plan_census.key(case), 0, lib.pinn_plan_padded_points(plan), lib.pinn_plan_workspace_bytes(plan, 0),
               lib.pinn_plan_workspace_bytes(plan, 1)] + [lib.pinn_plan_kernel(plan, k).decode() for k in (0, 1, 2)]
        lib.pinn_plan_destroy(plan)
        return row
    finally:
        if net:
            lib.pinn_net_destroy(net)
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _resolves(lib, c, streams, n, names, tile):
    """A constrained plan of the row's net names these kernels and pads to this tile; its padded points, workspace
    bytes (which the spill format decides) and names are the census row of the unconstrained plan under
    PINN_SCHED=0 PINN_WSPLIT=0 PINN_FUSE=0, here and at the census's own point count."""
    prec = tuple(CODE[p] for p in c["triple"])
    for pts in (n, 360000):
        got = _constrained_census(lib, (c["H"], c["L"], prec, streams, pts, dict(c["env"])), _bc_of(c).struct())
        assert got[1] == 0, got
        assert tuple(got[5:8]) == names, got
        plain = plan_census.run_case(lib, (c["H"], c["L"], prec, streams, pts, dict(EIGHT_WAVE, **dict(c["env"]))))
        assert got[1:] == plain[1:], (got, plain)
    got = _constrained_census(lib, (c["H"], c["L"], prec, streams, n, dict(c["env"])), _bc_of(c).struct())
    assert got[2] == -(-n // tile) * tile, got


def test_the_table_is_what_the_module_says():
    assert [c["H"] for c in CASES_WIDTH] == [h for h in (8, 16, 50, 80, 128, 200, 256, 330, 400, 512) for _ in (0, 1)]
    assert {c["L"] for c in CASES_RE1 if not c["ev"]} <= {1, 2, 3}
    assert len(CASES_COLS64) == 2 and len(CASES_MIXED) == 6 and len(CASES_EV) == 1 and len(CASES_EDGE) == 8
    assert {(c["m"], c["r"]) for c in CASES_EDGE} == set(EDGES) and {m for m, _ in EDGES} == {1, 8}
    assert {r for _, r in EDGES} == {4.0, 25.0}
    # every launcher's width switch: padded widths 32 .. 256 and 288 .. 512, the shipped ev shape's 96 among them
    assert sorted({_hp(c["H"]) for c in CASES_WIDTH}) == [32, 64, 96, 128, 224, 256, 352, 416, 512]
    assert [c["names"][0] for c in CASES_LAP] == ["fwd_kernel", "fwd_wide_kernel", "fwd_bf16_kernel", "fwd_bf16_wide_kernel"]
    assert {c["names"][0] for c in CASES} == {c["names"][0] for c in CASES_LAP}
    assert len({c["tag"] for c in CASES}) == len(CASES)
    assert all(1.0 <= c["gain"] <= 3.0 for c in CASES)
    assert (-(-N // 32), N % 32, -(-N // 16), N % 16) == (3, 5, 5, 5)
    x, y, _ = _points(N, 1)
    sx, sy = hm.special_points()
    assert x.size == N and np.array_equal(x[:9], sx) and np.array_equal(y[:9], sy)


@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_every_row_resolves_to_the_names_it_lists(lib, c):
    _resolves(lib, c, 4, N, c["names"], c["tile"])


def test_mixed_triples_and_64_column_rows_name_what_they_are_for():
    assert [c["names"] for c in CASES_MIXED] == [
        ("fwd_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"), ("fwd_bf16_kernel", "bwd_kernel", "dw_bf16_kernel"),
        ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_kernel"),
        ("fwd_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel"),
        ("fwd_bf16_wide_kernel", "bwd_wide_kernel", "dw_bf16_wide_kernel"),
        ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_wide_kernel")]
    assert [(c["names"][:2], c["tile"]) for c in CASES_COLS64] == [(("fwd_bf16_kernel", "bwd_bf16_kernel"), 16)] * 2


# --------------------------------------------------------------------------------------------------------------------
# CPU: conditions on the inputs, asserted on the model alone
# --------------------------------------------------------------------------------------------------------------------
def _shares(c):
    r, r0 = _model(c), _model(c, "inviscid")
    return dict(eq1=_rel_max(r0["eqs"][0], r["eqs"][0]), eq2=_rel_max(r0["eqs"][1], r["eqs"][1]),
                grad=_rel_l2(r0["grad"], r["grad"]))


@pytest.mark.parametrize("c", _nets(CASES), ids=_ids(_nets(CASES)))
def test_condition_a_the_viscous_term_carries_its_share(c):
    """A condition on the inputs, not a measurement: a row that does not meet it gets another seed or gain."""
    s = _shares(c)
    print("[hardbc terms] %s viscous share: %s" % (c["tag"], " ".join("%s %.2f" % kv for kv in s.items())))
    assert min(s.values()) >= SHARE_MIN, s
    if c["Re"] == RE_LAP:
        assert min(s["eq1"], s["eq2"]) >= SHARE_MIN_LAP, s


@pytest.mark.parametrize("c", CASES_EV, ids=_ids(CASES_EV))
def test_ev_case_takes_both_branches_of_the_viscosity_clamp(c):
    inp = _inputs(c)
    clamped = c["ev"]["alpha_evm"] * np.abs(inp["e"]) > 20.0 / c["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()


def _detected(c, term):
    """(error / bar, quantity) of the judged quantity a relative error of `term` moves furthest, at 2^-8 or at the
    power of two DETECT names for the row's bars."""
    ex = DETECT.get((c["bar"], term), -8)
    return _worst(_errs(c, _model(c, (term, ex)), _model(c)))


def _rows_b():
    """One row per net and bar of the Re = 1 table (rows that differ only in kernels share both)."""
    seen = {}
    for c in CASES_RE1:
        seen.setdefault(_key(c) + (c["bar"],), c)
    return list(seen.values())


@pytest.mark.parametrize("c", _rows_b(), ids=_ids(_rows_b()))
def test_condition_b_an_error_of_one_bf16_term_in_any_of_the_seven_leaves_a_bar(c):
    """Per row: a 2^-8 relative error (one dropped low bf16 term) of each of the seven Laplacian terms moves at least
    one judged quantity of the row's precision past its bar."""
    out = {t: _detected(c, t) for t in hm.LAPLACIAN_TERMS}
    print("[hardbc terms] %s: %s" % (c["tag"], " ".join("%s %.1fx(%s)" % ((t,) + v) for t, v in out.items())))
    for t, (ratio, name) in out.items():
        assert ratio > 1.0, (t, ratio, name)


def test_detect_holds_smallest_powers_of_two_only():
    """An exception in DETECT is the smallest power of two that is seen: half of it is not, on any row of that bar."""
    for (bar, term), ex in DETECT.items():
        assert ex > -8 and term in hm.LAPLACIAN_TERMS
        rows = [c for c in _rows_b() if c["bar"] == bar]
        assert any(_worst(_errs(c, _model(c, (term, ex - 1)), _model(c)))[0] <= 1.0 for c in rows), (bar, term)


def _re400_case():
    """The comparison tests/test_hardbc_gpu.py makes: 4x50, Re = 400, 200 points, unit weights, the whole vector."""
    c = _case(4, 50, 150, 1.0, 54, X3, Re=400.0)
    inp = _inputs(c, 200)
    return c, inp


def test_control_c_the_same_errors_pass_the_whole_vector_comparison_at_re_400():
    """Why the rows above exist: at Re = 400 each of the seven 2^-8 errors stays inside the bars test_hardbc_gpu.py
    judges by - fields 5e-4 (bf16x3), gradient rel-L2 1e-4 on the whole vector (the boundary term adds nothing: its
    gradient is zero under the constraint) - and `D a_D` or `D Lap N` could be missing altogether."""
    c, inp = _re400_case()
    ref = _model_run(c, inp)
    for term in hm.LAPLACIAN_TERMS:
        got = _model_run(c, inp, rel={term: EPS8})
        fields = max([_rel_max(got["fields"][k], ref["fields"][k]) for k in PLANES] +
                     [_rel_max(a, b) for a, b in zip(got["eqs"], ref["eqs"])])
        loss = abs(sum(got["sums"]) - sum(ref["sums"])) / sum(ref["sums"])
        grad = _rel_l2(got["grad"], ref["grad"])
        print("[hardbc terms] Re=400 4x50 %s * (1 + 2^-8): fields %.1e loss %.1e gradient %.1e" % (term, fields, loss, grad))
        assert fields < 5e-4 and loss < 1e-4 and grad < 1e-4, (term, fields, loss, grad)
    for term in ("t_D", "D_lapN"):
        got = _model_run(c, inp, rel={term: -1.0})
        assert _rel_l2(got["grad"], ref["grad"]) < 1e-4, term


@pytest.mark.parametrize("c", CASES_EDGE, ids=_ids(CASES_EDGE))
def test_fp32_point_factors_stay_within_a_quarter_of_every_bar(c):
    """The descriptor's edges: hm.point_factors in fp32 (the stage's arithmetic: expf, Y^m by repeated multiplication)
    against fp64, pushed through the fp64 model, uses at most a quarter of each bar - what is left belongs to the
    kernels."""
    errs = _errs(c, _model(c, "fp32"), _model(c))
    ratio, name = _worst(errs)
    print("[hardbc terms] %s fp32 factors: worst %s at %.3f of its bar" % (c["tag"], name, ratio))
    assert ratio <= 0.25, (name, ratio, errs)


# --------------------------------------------------------------------------------------------------------------------
# GPU: one constrained loss_and_grad per row, the residual term's planes, sums and gradient against the model
# --------------------------------------------------------------------------------------------------------------------
def _clear_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("PINN_") or k == "NSFNET_CHUNK_POINTS":
            monkeypatch.delenv(k, raising=False)


def _boundary(c):
    xb, yb, ub, vb = (a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())
    return (2.0 * xb - 1.0, 2.0 * yb - 1.0, ub, vb) if c["ev"] else (xb, yb, ub, vb)


def _engine(monkeypatch, c, inp, **kw):
    """A constrained engine of the row's net, precision, switches and descriptor; no point set yet."""
    from nsfnet_amd import engine as eng
    _clear_env(monkeypatch)
    for k, v in c["env"]:
        monkeypatch.setenv(k, v)
    ev = c["ev"]
    if ev:
        kw = dict(kw, flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=ev["alpha_evm"], coord_scale=inp["scale"])
    E = eng.PinnEngine(torch.device("cuda:0"), c["L"], c["H"], c["Re"], alpha_b=10.0, alpha_e=1.0, precision=c["prec"], **kw)
    bc = _bc_of(c)
    E.set_hard_boundary(True, lift_power=bc.m, lid_sharpness=bc.r, origin=(bc.x0, bc.y0), inv_len=bc.inv_len)
    E.net.set_flat(torch.tensor(inp["flat"]))
    if ev:
        E.net_e.set_flat(torch.tensor(inp["flat_e"]))
        E.e_trainable = True
    return E


def _is_constrained(plan, c):
    got = plan.hard_bc()
    bc = _bc_of(c)
    assert got is not None and got["kind"] == 1 and got["lift_power"] == bc.m
    assert (got["x0"], got["y0"], got["inv_len"]) == (bc.x0, bc.y0, bc.inv_len)
    assert got["lid_sharpness"] == np.float32(bc.r)


def _planes(plan, nq):
    f = lambda k: plan.field(k).cpu().numpy().astype(np.float64)
    return dict(fields={k: f(k) for k in PLANES}, eqs=[f("eq%d" % (k + 1)) for k in range(nq)])


def _residual_gradient(E, plan):
    """The residual term's gradient alone: the assembly over the residual plan only (loss_and_grad's own assembly has
    added the value plans')."""
    from nsfnet_amd import engine as eng
    gr = torch.full((E.net.num_params,), float("nan"), dtype=torch.float32, device=E.device)
    eng.grad_reduce(E.net, [plan], gr)
    torch.cuda.synchronize()
    g = gr.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    return g


def _run(monkeypatch, c):
    inp = _inputs(c)
    E = _engine(monkeypatch, c, inp)
    E.set_collocation(inp["x"], inp["y"], weights=inp["w"])
    E.set_boundary(*_boundary(c))
    assert E.plan_f.kernel_names() == c["names"]
    _is_constrained(E.plan_f, c)
    assert E.plan_f.npad == -(-N // c["tile"]) * c["tile"]
    ev = c["ev"]
    got = dict(vtm0=E.plan_f.vis_t_minus.cpu().numpy().astype(np.float64) if ev else None)
    E.loss_and_grad()
    got["grad"] = _residual_gradient(E, E.plan_f)
    got.update(_planes(E.plan_f, 4 if ev else 3), sums=E.sums.cpu().numpy().astype(np.float64))
    if ev:
        got["grad_e"] = E.grads_e.cpu().numpy().astype(np.float64)
        got["vis_t"] = E.plan_f.vis_t.cpu().numpy().astype(np.float64)
    del E
    torch.cuda.empty_cache()
    return inp, got


def _judge(c, got, ref, n=N):
    errs = _errs(c, got, ref)
    worst = lambda keys: max(errs[k][0] for k in keys)
    print("[hardbc terms] %s N=%d: planes %.2e eqs %.2e (bar %.0e) sums %.2e (bar %.0e)%s | %s" % (
        c["tag"], n, worst(PLANES), worst([k for k in errs if k.startswith("eq")]), BARS[c["bar"]]["eq"], errs["sums"][0],
        BARS[c["bar"]]["sums"], "".join(" %s %.2e (bar %.0e)" % ((k,) + errs[k]) for k in ("grad_r", "grad_e") if k in errs),
        " ".join("%s %.2e" % (k, e) for k, (e, _) in errs.items())))
    for k, (e, b) in errs.items():
        assert e <= b, (k, e, b)


_GPU_PLAIN = [c for c in CASES if not c["ev"]]


@pytest.mark.gpu
@pytest.mark.parametrize("c", _GPU_PLAIN, ids=_ids(_GPU_PLAIN))
def test_constrained_residual_term_vs_model(monkeypatch, c):
    _, got = _run(monkeypatch, c)
    _judge(c, got, _model(c))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES_EV, ids=_ids(CASES_EV))
def test_constrained_residual_term_ev_vs_model(monkeypatch, c):
    """vis_t is the run's own, so the model run is this case's; both branches of the clamp are taken on the device."""
    inp, got = _run(monkeypatch, c)
    assert _rel_max(got["vtm0"], c["ev"]["alpha_evm"] * np.abs(inp["e"])) <= BARS[c["bar"]]["eq"]
    vis_t = _vis_t(c, inp, got["vtm0"])
    np.testing.assert_allclose(got["vis_t"], vis_t, rtol=1e-6)
    clamped = got["vtm0"] > 20.0 / c["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()
    _judge(c, got, _model_run(c, inp, vis_t=vis_t))


# --------------------------------------------------------------------------------------------------------------------
# value mode with D != 0: the supervised term alone, per family value kernel
# --------------------------------------------------------------------------------------------------------------------
N_SUP = 150
ALPHA_S = 2.0
# (hidden, precision): fwd_kernel, fwd_bf16_kernel at 128 and at 256, fwd_wide_kernel, fwd_bf16_wide_kernel
VALUE_ROWS = [(50, F32), (128, X3), (256, F32), (256, X3), (400, X3)]
CASES_VALUE = [_case(*NETS[H], p) for H, p in VALUE_ROWS]


def _value_inputs(c):
    """150 interior points with random u, v, p targets, a third of the p targets NaN."""
    rng = np.random.RandomState(500 + c["H"])
    x, y = (0.02 + 0.96 * rng.rand(N_SUP)).astype(np.float32), (0.02 + 0.96 * rng.rand(N_SUP)).astype(np.float32)
    u, v, p = (rng.randn(N_SUP).astype(np.float32) for _ in range(3))
    p[::3] = np.nan
    n_p = int(np.isfinite(p).sum())
    coef = (2.0 * ALPHA_S / N_SUP, 2.0 * ALPHA_S / N_SUP, 2.0 * ALPHA_S / n_p)
    return dict(flat=_flat(c["L"], c["H"], c["seed"], c["gain"]), x=x, y=y, targets=[u, v, p], coef=coef, n_p=n_p)


_VALUE_CACHE = {}


def _value_model(c, rel=None):
    k = (c["L"], c["H"], c["seed"], c["gain"], None if rel is None else tuple(rel.items()))
    if k not in _VALUE_CACHE:
        inp = _value_inputs(c)
        P = fr.unflatten(inp["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
        _VALUE_CACHE[k] = hm.constrained_value(P, _bc_of(c), inp["x"], inp["y"], targets=inp["targets"], coef=inp["coef"],
                                               rel=rel)
    return _VALUE_CACHE[k]


@pytest.mark.parametrize("c", _nets(CASES_VALUE), ids=_ids(_nets(CASES_VALUE)))
def test_value_control_an_error_of_one_bf16_term_in_the_adjoints_d_leaves_the_bar(c):
    """D is nowhere zero on the points (the wall-point checks elsewhere see a zero gradient whatever the code does),
    and a 2^-8 relative error of the adjoint's D moves every layer block of the supervised gradient past the bar."""
    inp = _value_inputs(c)
    D = hm.point_factors(_bc_of(c), inp["x"].astype(np.float64), inp["y"].astype(np.float64))["D"]
    assert D.min() > 1e-3 and inp["n_p"] == N_SUP - len(range(0, N_SUP, 3))
    ref, off = _value_model(c), _value_model(c, {hm.VALUE_TERM: EPS8})
    assert np.linalg.norm(ref["grad"]) > 0.0
    moved = _block_errs(off["grad"], ref["grad"], 3, c["L"], c["H"])
    print("[hardbc terms] value %dx%d, adjoint's D * (1 + 2^-8): blocks move %.2e .. %.2e" % (c["L"], c["H"], min(moved), max(moved)))
    assert min(moved) > max(GRAD_BAR.values()), moved
    np.testing.assert_array_equal(off["pred"], ref["pred"])


@pytest.mark.parametrize("c", CASES_VALUE, ids=_ids(CASES_VALUE))
def test_every_value_row_resolves_to_the_names_it_lists(lib, c):
    _resolves(lib, c, 1, N_SUP, c["names"], 4 * c["tile"])
    assert [k["names"][0] for k in CASES_VALUE] == ["fwd_kernel", "fwd_bf16_kernel", "fwd_wide_kernel", "fwd_bf16_kernel",
                                                    "fwd_bf16_wide_kernel"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES_VALUE, ids=_ids(CASES_VALUE))
def test_constrained_value_mode_vs_model(monkeypatch, c):
    """Through set_supervised: pred, the three sums and the supervised gradient alone (grad_reduce over plan_s), per
    layer block, against hm.constrained_value."""
    from nsfnet_amd import engine as eng
    inp, ref = _value_inputs(c), _value_model(c)
    E = _engine(monkeypatch, c, inp, alpha_s=ALPHA_S)
    x, y, _ = _points(N, c["pts"])
    E.set_collocation(x, y)
    E.set_boundary(*_boundary(c))
    E.set_supervised(inp["x"], inp["y"], *inp["targets"])
    s = E.plan_s
    assert s.kernel_names() == c["names"] and s.npad == -(-N_SUP // (4 * c["tile"])) * 4 * c["tile"]
    _is_constrained(s, c)
    E.loss_and_grad()
    g = _residual_gradient(E, s)
    pred = s.pred.cpu().numpy().astype(np.float64).T
    sums = E.sums[eng.S_SUP:eng.S_SUP + 4].cpu().numpy().astype(np.float64)
    del E, s
    torch.cuda.empty_cache()
    prec = c["bar"]
    pred_bar = PRED_BAR[prec] * (1.0 if prec == F32 else max(1.0, float(np.abs(ref["pred"]).max())))
    blocks = _block_errs(g, ref["grad"], 3, c["L"], c["H"])
    errs = dict(pred=float(np.abs(pred - ref["pred"]).max()), sums=_rel_max(sums[:3], np.asarray(ref["sums"][:3])), grad=max(blocks))
    print("[hardbc terms] value %s: pred %.2e (bar %.1e) sums %.2e (bar %.0e) gradient block %.2e (bar %.0e)" % (
        c["tag"], errs["pred"], pred_bar, errs["sums"], BARS[prec]["sums"], errs["grad"], GRAD_BAR[prec]))
    assert errs["pred"] <= pred_bar
    assert errs["sums"] <= BARS[prec]["sums"] and sums[3] == ref["sums"][3] == inp["n_p"]
    assert errs["grad"] <= GRAD_BAR[prec], blocks


# --------------------------------------------------------------------------------------------------------------------
# constrained workgroups that repeat their tile loop; chunked, forward-only and batch-gathered plans
# --------------------------------------------------------------------------------------------------------------------
# (L, H, net seed, points seed, (tile, paired, bpc) of test_tile_loops): the 8-wave bf16 sweeps at 256, the wide ones
LOOPS = {"6x256": (6, 256, 1234, 11, (32, False, 1)), "4x400": (4, 400, 31, 13, (16, False, 1))}


def _loop_case(shape):
    L, H, seed, pts, _ = LOOPS[shape]
    return _case(L, H, seed, 1.0, pts, X3)


@pytest.mark.parametrize("shape", sorted(LOOPS))
def test_looping_rows_resolve_and_loop(lib, shape):
    c, fam = _loop_case(shape), LOOPS[shape][4]
    assert families_of(c["names"], c["H"], False, c["tile"]) == [fam, fam]
    assert c["names"][:2] == (("fwd_bf16_kernel", "bwd_bf16_kernel") if shape == "6x256" else
                              ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel"))
    for cus in (256, 304):
        n = pick_n(cus, [fam], c["L"])
        assert loop_violations(n, cus, *fam, c["L"]) == []
        _resolves(lib, c, 4, n, c["names"], c["tile"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(LOOPS))
def test_constrained_sweeps_loop_vs_model(monkeypatch, shape):
    """Every workgroup of the constrained 8-wave sweeps takes 3-4 trips round its tile loop; Re = 1."""
    c, fam = _loop_case(shape), LOOPS[shape][4]
    cus = _cus()
    n = pick_n(cus, [fam], c["L"])
    inp = _inputs(c, n)
    E = _engine(monkeypatch, c, inp)
    E.set_collocation(inp["x"], inp["y"])
    E.set_boundary(*_boundary(c))
    assert E.plan_f.kernel_names() == c["names"]
    _is_constrained(E.plan_f, c)
    assert E.plan_f.npad == -(-n // c["tile"]) * c["tile"]
    for f in families_of(c["names"], c["H"], False, c["tile"]):
        assert f == fam and loop_violations(n, cus, *f, c["L"]) == [], f
    g = geometry(n, cus, *fam, c["L"])
    assert g["loop"] >= 3 * g["grid"] + 1
    E.loss_and_grad()
    got = dict(grad=_residual_gradient(E, E.plan_f), sums=E.sums.cpu().numpy().astype(np.float64), **_planes(E.plan_f, 3))
    del E
    torch.cuda.empty_cache()
    _judge(c, got, _model_run(c, inp), n)


N_PASS = 300


def _pass_case():
    return _case(*NETS[50], F32)


def _pass_engine(monkeypatch, chunk_points=None):
    c = _pass_case()
    inp = _inputs(c, N_PASS)
    E = _engine(monkeypatch, c, inp)
    E.set_collocation(inp["x"], inp["y"], chunk_points=chunk_points)
    E.set_boundary(*_boundary(c))
    return c, inp, E


@pytest.mark.gpu
def test_chunked_constrained_passes_vs_model_and_the_unchunked_engine(monkeypatch):
    """set_collocation(chunk_points=128) at N = 300: three passes sharing one workspace.  The boundary term's gradient
    is zero under the constraint, so E.grads is the residual term's."""
    from nsfnet_amd import engine as eng
    c, inp, E = _pass_engine(monkeypatch, chunk_points=128)
    assert isinstance(E.plan_f, eng.ChunkedResidual) and [b - a for a, b in E.plan_f.bounds] == [128, 128, 44]
    for ck in E.plan_f.chunks:
        _is_constrained(ck, c)
        assert ck.kernel_names() == c["names"]
    E.loss_and_grad()
    torch.cuda.synchronize()
    got = dict(grad=E.grads.cpu().numpy().astype(np.float64), sums=E.sums.cpu().numpy().astype(np.float64),
               **_planes(E.plan_f, 3))
    del E
    c, inp, E = _pass_engine(monkeypatch)
    assert isinstance(E.plan_f, eng.ResidualPlan)
    E.loss_and_grad()
    whole = _residual_gradient(E, E.plan_f)
    total = E.grads.cpu().numpy().astype(np.float64)
    del E
    torch.cuda.empty_cache()
    np.testing.assert_array_equal(total, whole)         # the boundary plan added exact zeros
    _judge(c, got, _model_run(c, inp, chunk=128), N_PASS)
    blocks = _block_errs(got["grad"], whole, 3, c["L"], c["H"])
    print("[hardbc terms] chunked against unchunked engine: gradient blocks %.2e .. %.2e" % (min(blocks), max(blocks)))
    assert max(blocks) <= GRAD_BAR[F32], blocks


@pytest.mark.gpu
def test_forward_only_pool_plan_returns_the_constrained_eq_planes(monkeypatch):
    c, inp, E = _pass_engine(monkeypatch)
    xp, yp, _ = _points(217, 77)
    E.set_resample_pool(xp, yp)
    pool = E._pool
    assert not pool.with_backward and pool.kernel_names() == c["names"]
    _is_constrained(pool, c)
    E.resample(k=1.0, c=1.0, seed=3)        # evaluates the pool under the current parameters
    torch.cuda.synchronize()
    got = _planes(pool, 3)
    del E, pool
    torch.cuda.empty_cache()
    ref = _model_run(c, dict(inp, x=xp, y=yp))
    for k in PLANES:
        assert _rel_max(got["fields"][k], ref["fields"][k]) <= BARS[F32]["eq"], k
    errs = [_rel_max(a, b) for a, b in zip(got["eqs"], ref["eqs"])]
    print("[hardbc terms] forward-only pool plan, 217 points: eq planes %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) <= BARS[F32]["eq"], errs


@pytest.mark.gpu
def test_batch_gathered_plan_evaluates_the_constrained_residual_of_its_points(monkeypatch):
    c, inp, E = _pass_engine(monkeypatch)
    B = 100
    E.set_batching(B, seed=5)
    E.loss_and_grad()
    torch.cuda.synchronize()
    assert E.evaluated_batch
    idx = E.batch_indices().cpu().numpy()
    assert idx.size == B and (np.diff(idx) > 0).all()
    f, _ = E.eval_plans()
    _is_constrained(f, c)
    np.testing.assert_array_equal(f.x.cpu().numpy(), inp["x"][idx])
    got = dict(grad=_residual_gradient(E, f), sums=E.sums.cpu().numpy().astype(np.float64), **_planes(f, 3))
    del E, f
    torch.cuda.empty_cache()
    _judge(c, got, _model_run(c, dict(inp, x=inp["x"][idx], y=inp["y"][idx])), B)
