"""The pseudo-time point stages judged per term, rate regime and layer block against the fp64 model (DESIGN.md section
7.11, "Judged per term").

The pseudo-time term is written out by hand twice - under PT in point_stage.h (the 8-wave, role-split and wide
role-split sweeps) and in the fused kernel's own point stage - and each copy has ten pieces (ptime_model.TERMS): the
drift sigma_k (c_k - c_k*) as it enters the three loss sums, the same drift as the reverse sweep rebuilds it for g_k,
and the value seeds sigma g1, sigma g2, sigma_p g3, the last of which is the only non-zero value adjoint the pressure
output ever carries and the only contribution to the pressure entry of the output-bias gradient.
tests/test_pseudo_time_gpu.py and tests/test_pseudo_time_split_gpu.py compare the whole gradient vector with the
boundary gradient added at alpha_b = 10, at Re = 400, with both rates on: `sigma_p g3` or both of `sigma g1`,
`sigma g2` could be missing altogether and their bar would hold (test_control_c_... records that).  Here, as in
tests/test_residual_term.py and tests/test_hardbc_terms.py:
  * Re = 1, N = 69 points (three 32-point tiles with a ragged last one and a dummy partner for the paired sweeps, five
    16-point tiles), the four corners, a point on each wall and the centre among them; anchors = the fp32 fields of an
    independently seeded net of the same shape;
  * two rate regimes per row, from ptime_model.balanced_rates at (1, 1): V = (k sb, 0), the engine's default shape
    (pressure_dtau=None), and P = (0, k spb), where the pressure seed is alone; k = 4, but 2 with walls and 12 on the ev
    rows (K_WALLS, K_EV say why);
  * the gradient is the residual term's alone (grad_reduce over plan_f) and judged per layer weight and bias block, the
    three sums each alone, the pressure entry of the output-bias gradient alone (== 0.0 in regime V), the planes and the
    steady eq planes unscaled.  Bars: BARS of test_tile_loops.py and GRAD_BAR of test_residual_term.py, the sums and the
    gradient times max(1, A) with A of ptime_model.amplification (<= 8, asserted on the model).  No bar is new and none
    comes from a kernel's output.
Rows: fp32 and bf16x3 at the ten widths of test_hardbc_terms.NETS, the 64-column bf16 tiles, three mixed precision
triples at 256 and 400, the role-split, fused and wide role-split sweeps under PINN_PTIME_SPLIT=1, one row with hard
walls per instantiation family, two ev rows with weights and the coordinate map, and three rows whose workgroups repeat
their tile loop.

The CPU tests keep the table honest, on the model alone: every row resolves, as a pseudo-time plan, to the kernels and
the path it names; (a) A <= 8, the pressure entry carries its block in regime P, the nets that are not
test_hardbc_terms.NETS's carry their viscous share; (b) per row, regime and term a 2^-8 relative error moves a judged
quantity past 1.5 of its bar (DETECT holds the exceptions); eq4 built on q1, q2 is seen on the ev rows.
"""
import os

import numpy as np
import pytest
import torch

import hardbc_model as hm
import ptime_model as pm
from oracle import fwdmode_ref as fr

import test_hardbc_terms as hb
import test_pseudo_time_gpu as ptg
from test_hardbc_split_cpu import FUSED, PLAIN, SPLIT, TWO, WIDE, WSPLIT
from test_hardbc_terms import MIXED, NETS, _flat, _names, _points, _tile, lib  # noqa: F401
from test_kernel_pairings import CODE, F32, X3
from test_pseudo_time_split_cpu import SWITCH, _path
from test_residual_term import EPS8, GRAD_BAR, SHARE_MIN, _block_errs, _blocks
from test_tile_loops import BARS, _cus, _rel_l2, _rel_max, geometry

N = 69
RE = 1.0
K = 4                     # the regimes' rates in units of the balanced ones
# ... but where a condition of (a) forces another whole number.  Walls, k = 2: with the lid's lift max|u| is 1 while
# q1 stays small, so A grows with the rate - at k = 4 the MODEL has A = 8.5 .. 10.2 on the 3x50, 3x256 and 3x330 rows
# (k = 3: 8.6 .. 10.5 on the 3x50 and 3x256 ones; k = 2: 4.5 .. 7.5 on all seven), the effect the 2x400 walls row of tests/test_pseudo_time_split_gpu.py
# records; the bound A <= 8 stays.  ev, k = 12: with the coordinate map and the weights the pressure entry is 0.11 /
# 0.15 of the output-bias block at k = 4 and 0.46 / 0.59 at k = 8; at 12 it is 0.77 / 0.87, A = 1.4.
K_WALLS, K_EV = 2, 12
MARGIN = 1.5              # (b): an error of one bf16 term moves a judged quantity by more than this many bars
CUS = 256                 # the compute units of an MI355X: where the CPU tests evaluate the looping rows
PLANES = ("u", "v", "p", "u_x", "u_y", "v_x", "v_y")
REGIMES = ("V", "P")
ACTIVE = {"V": ("fwd_q1", "fwd_q2", "bwd_q1", "bwd_q2", "seed_u", "seed_v"), "P": ("fwd_q3", "bwd_q3", "seed_p")}
ON = ((SWITCH, "1"),)


# --------------------------------------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------------------------------------
def _row(L, H, seed, gain, pts, prec, env=(), names=None, path=PLAIN, m=None, ev=None, n=N, k=K, own=False):
    """(L, H, net seed, layer-0 weight gain, points seed) as test_hardbc_terms.NETS; m: lift_power of the hard walls or
    None; n: a point count, or the looping count "4cu" (test_pseudo_time_gpu) / "loop" (test_pseudo_time_split_gpu); k:
    the rates' multiple of the balanced ones; own: the net is not one of NETS."""
    triple = tuple(prec.split(",")) if "," in prec else (prec,) * 3
    tag = "%dx%d%s %s%s%s%s" % (L, H, "+4x40 ev" if ev else "", prec, "".join(" %s=%s" % kv for kv in env),
                                "" if m is None else " walls m=%d" % m, "" if n == N else " N=%s" % n)
    return dict(L=L, H=H, seed=seed, gain=gain, pts=pts, prec=prec, triple=triple, env=tuple(env), Re=RE, ev=ev, m=m, n=n,
                k=k, own=own, tag=tag, names=_names(H, triple) if names is None else tuple(names), path=path,
                tile=_tile(H, triple, env), bar=F32 if set(triple) == {F32} else X3)


ROWS_WIDTH = [_row(*NETS[H], p) for H in sorted(NETS) for p in (F32, X3)]
ROWS_COLS64 = [_row(*NETS[H], X3, env=(("PINN_TILE_COLS", "64"),)) for H in (128, 256)]
ROWS_MIXED = [_row(*NETS[H], p) for H in (256, 400) for p in MIXED]
# the wide role-split widths: 330 of NETS; 288 and 448 as test_residual_term.WIDE has them (2 layers, net seed 72)
WIDE_NETS = {288: (2, 288, 72, 1.0, 42), 330: NETS[330], 448: (2, 448, 72, 1.0, 43)}
ROWS_SPLIT = [_row(*NETS[256], X3, env=ON, names=SPLIT, path=FUSED),
              _row(*NETS[256], X3, env=ON + (("PINN_FUSE", "0"),), names=SPLIT, path=TWO)] + \
             [_row(*WIDE_NETS[H], X3, env=ON, names=WSPLIT, path=WIDE, own=H != 330) for H in (288, 330, 448)]
# hard walls, one row per instantiation family (PT and HBC together), lift_power 2 and 3 in turn
ROWS_WALLS = [_row(*NETS[50], F32, m=3, k=K_WALLS), _row(*NETS[256], F32, m=2, k=K_WALLS), _row(*NETS[256], X3, m=3, k=K_WALLS),
              _row(*NETS[400], X3, m=2, k=K_WALLS), _row(*NETS[256], X3, env=ON, names=SPLIT, path=FUSED, m=3, k=K_WALLS),
              _row(*NETS[256], X3, env=ON + (("PINN_FUSE", "0"),), names=SPLIT, path=TWO, m=2, k=K_WALLS),
              _row(*NETS[330], X3, env=ON, names=WSPLIT, path=WIDE, m=3, k=K_WALLS)]
# ev: per-point weights, the coordinate map (scale 2, origin -1), a trainable 4x40 entropy net, and alpha_evm putting
# alpha_evm |e| on either side of 20 / Re (test_residual_term.CASES_EV)
ROWS_EV = [_row(4, 50, 161, 2.0, 41, F32, ev=dict(seed=62, alpha_evm=150.0), k=K_EV, own=True),
           _row(3, 256, 154, 2.0, 44, X3, env=ON, names=SPLIT, path=FUSED, ev=dict(seed=22, alpha_evm=600.0), k=K_EV,
                own=True)]
# workgroups that repeat their tile loop, at the counts of the existing modules (which judge them as one vector)
ROWS_LOOP = [_row(4, 50, 161, 2.0, 45, X3, n="4cu", own=True),
             _row(*NETS[256][:4], 46, X3, env=ON, names=SPLIT, path=FUSED, n="loop"),
             _row(*NETS[400][:4], 47, X3, env=ON, names=WSPLIT, path=WIDE, n="loop")]
ROWS_69 = ROWS_WIDTH + ROWS_COLS64 + ROWS_MIXED + ROWS_SPLIT + ROWS_WALLS + ROWS_EV
ROWS = ROWS_69 + ROWS_LOOP
_ids = lambda rows: [c["tag"] for c in rows]

# (b): the smallest relative error of a term, a power of two, that moves a judged quantity of the row past MARGIN bars
# where 2^-8 does not: {(row tag, regime, term): exponent}, none weaker than 2^-6
DETECT = {}


# --------------------------------------------------------------------------------------------------------------------
# inputs and the model
# --------------------------------------------------------------------------------------------------------------------
def _n(c, cus=CUS):
    if c["n"] == "4cu":
        return 4 * cus * 32 + 5
    if c["n"] == "loop":
        return (2 * cus + 2) * c["tile"] + 5
    return c["n"]


def _bc_of(c):
    return None if c["m"] is None else hm.HardBc(lift_power=c["m"])


def _key(c, cus=CUS):
    return (c["L"], c["H"], c["seed"], c["gain"], c["pts"], c["m"], _n(c, cus), c["k"],
            None if not c["ev"] else tuple(sorted(c["ev"].items())))


_INPUTS = {}


def _inputs(c, cus=CUS):
    """Net, points, anchors (and the ev flavour's weights, scale and entropy net) of a row: float32, as the engine
    holds them.  Computed once per net and point set, shared, never written."""
    key = _key(c, cus)
    if key not in _INPUTS:
        _INPUTS[key] = _make_inputs(c, _n(c, cus))
    return _INPUTS[key]


def _make_inputs(c, n):
    inp = hb._inputs(c, n)
    inp["n"] = n
    inp["P"] = fr.unflatten(inp["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
    # anchors: the fp32 fields of an independently seeded net of the same shape (test_pseudo_time_gpu._problem)
    other = fr.unflatten(_flat(c["L"], c["H"], c["seed"] + 100, c["gain"]).astype(np.float64), 2, 3, c["L"], c["H"])
    if c["m"] is None:
        out = fr.forward4(other, inp["x"].astype(np.float64), inp["y"].astype(np.float64))[0]
        u, v, p = out[:, 0, 0], out[:, 1, 0], out[:, 2, 0]
    else:
        f = pm.residual_term(other, inp["x"], inp["y"], RE, np.zeros((3, n)), 0.0, 0.0, bc=_bc_of(c))["fields"]
        u, v, p = f["u"], f["v"], f["p"]
    inp["anchor"] = np.stack([u, v, p]).astype(np.float32)
    return inp


def _run_model(c, inp, rates, errors=None, vis_t="own", Re=RE):
    kw = {}
    if c["ev"]:
        vt = hb._vis_t(c, inp) if isinstance(vis_t, str) else vis_t
        kw = dict(vis_t=np.asarray(vt, np.float64), w=inp["w"].astype(np.float64), scale=inp["scale"], params_e=inp["Pe"])
    return pm.residual_term(inp["P"], inp["x"], inp["y"], Re, inp["anchor"], rates[0], rates[1], bc=_bc_of(c), errors=errors,
                            **kw)


_CACHE = {}


def _model(c, what, errors=None, cus=CUS):
    """Model runs of a row's net, points, anchors and walls, shared by the rows that differ only in kernels: what =
    'one' (rates (1, 1), which the balanced rates come from), 'inviscid' (zero rates, Re = 1e30, no vis_t), 'steady'
    (zero rates) or a regime, there with errors = ((term, factor), ...) on single terms."""
    k = _key(c, cus) + (what, errors)
    if k not in _CACHE:
        inp = _inputs(c, cus)
        if what == "one":
            _CACHE[k] = _run_model(c, inp, (1.0, 1.0))
        elif what == "steady":
            _CACHE[k] = _run_model(c, inp, (0.0, 0.0))
        elif what == "inviscid":
            _CACHE[k] = _run_model(c, inp, (0.0, 0.0), vis_t=0.0 * hb._vis_t(c, inp) if c["ev"] else None, Re=1.0e30)
        else:
            _CACHE[k] = _run_model(c, inp, _rates(c, what, cus), errors=None if errors is None else dict(errors))
    return _CACHE[k]


def _rates(c, regime, cus=CUS):
    """The regime's rates as the fp32 launch constants the plan holds: V = (k sb, 0), P = (0, k spb)."""
    sb, spb = pm.balanced_rates(_model(c, "one", cus=cus))
    return (float(np.float32(c["k"] * sb)), 0.0) if regime == "V" else (0.0, float(np.float32(c["k"] * spb)))


def _nets(rows):
    seen = {}
    for c in rows:
        seen.setdefault(_key(c) + (c["bar"],), c)
    return list(seen.values())


def _p_entry(g, c):
    """The pressure entry of the output-bias block of a flat gradient, and the block's norm."""
    b = _blocks(g, 3, c["L"], c["H"])[-1].reshape(-1)
    assert b.size == 3
    return float(b[2]), float(np.linalg.norm(b))


def _errs(c, regime, got, ref, A, planes=True):
    """Every judged quantity of a row and regime as {name: (error, bar)}: the planes and the steady eq planes (max-abs
    / max|ref|, unscaled), each loss sum alone (relative), every layer's weight block (W0 ..) and bias block (b0 ..) of
    the residual gradient, the worst block of the entropy net's and, in regime P, the pressure entry of the output-bias
    gradient alone - the sums of q and the gradient at their bar times max(1, A)."""
    bar, gbar, grow = BARS[c["bar"]], GRAD_BAR[c["bar"]], max(1.0, A)
    out = {}
    if planes:
        for k in PLANES:
            out[k] = (_rel_max(got["fields"][k], ref["fields"][k]), bar["eq"])
        for k, q in enumerate(got["eqs"]):
            out["eq%d" % (k + 1)] = (_rel_max(q, ref["eqs"][k]), bar["eq"])
    for k in range(3):
        out["sum%d" % (k + 1)] = (abs(got["sums"][k] - ref["sums"][k]) / ref["sums"][k], bar["sums"] * grow)
    steady = (2,) if regime == "V" else (0, 1)          # where the rate is off the sum is the steady one
    for k in steady:
        out["sum%d_steady" % (k + 1)] = (abs(got["sums"][k] - ref["steady_sums"][k]) / ref["steady_sums"][k], bar["sums"] * grow)
    if c["ev"]:
        out["sum4"] = (abs(got["sums"][3] - ref["sums"][3]) / ref["sums"][3], bar["sums"])
        out["grad_e"] = (max(_block_errs(got["grad_e"], ref["grad_e"], 1, 4, 40)), gbar * grow)
    for j, e in enumerate(_block_errs(got["grad"], ref["grad"], 3, c["L"], c["H"])):    # layer j's weights, then its bias
        out["%s%d" % ("Wb"[j % 2], j // 2)] = (e, gbar * grow)
    if regime == "P":
        g, r = _p_entry(got["grad"], c)[0], _p_entry(ref["grad"], c)[0]
        out["dbo2"] = (abs(g - r) / abs(r), gbar * grow)
    return out


def _worst(errs):
    """The judged quantity furthest out, as (error / bar, name)."""
    return max((e / b, k) for k, (e, b) in errs.items())


def _amp(c, regime, cus=CUS):
    return pm.amplification(_model(c, regime, cus=cus), _inputs(c, cus)["anchor"], *_rates(c, regime, cus))


# --------------------------------------------------------------------------------------------------------------------
# CPU: the model's knobs
# --------------------------------------------------------------------------------------------------------------------
def test_no_errors_changes_no_bit_and_each_knob_moves_its_own_term():
    """errors=None, {} and factors of 1 are bit for bit the model; a factor on a forward term moves its sum and nothing
    else, on a reverse term or a seed the gradient and no sum; a seed's change is the seed's share, linear in it."""
    c = ROWS_EV[0]
    inp = _inputs(c)
    rates = (0.7, 0.3)
    ref = _run_model(c, inp, rates)
    for same in ({}, {t: 1.0 for t in pm.TERMS[:-1]}, {"eq4_on_q": False}):
        got = _run_model(c, inp, rates, errors=same)
        assert got["sums"] == ref["sums"] and got["loss_e"] == ref["loss_e"]
        for k in ("grad", "grad_e"):
            np.testing.assert_array_equal(got[k], ref[k])
    assert pm.TERMS == pm.FORWARD_TERMS + pm.REVERSE_TERMS + pm.SEED_TERMS + ("eq4_on_q",) and len(pm.TERMS) == 10
    assert sorted(ACTIVE["V"] + ACTIVE["P"]) == sorted(pm.TERMS[:-1])
    for k, t in enumerate(pm.FORWARD_TERMS):
        got = _run_model(c, inp, rates, errors={t: 1.0 + EPS8})
        assert [a != b for a, b in zip(got["sums"], ref["sums"])] == [j == k for j in range(4)]
        np.testing.assert_array_equal(got["grad"], ref["grad"])
        np.testing.assert_array_equal(got["q"][k], ref["q"][k])
    for t in pm.REVERSE_TERMS + pm.SEED_TERMS:
        got = _run_model(c, inp, rates, errors={t: 1.0 + EPS8})
        assert got["sums"] == ref["sums"] and np.abs(got["grad"] - ref["grad"]).max() > 0.0
        np.testing.assert_array_equal(got["grad_e"], ref["grad_e"])
    for t in pm.SEED_TERMS:
        off = _run_model(c, inp, rates, errors={t: 0.0})["grad"] - ref["grad"]
        eps = _run_model(c, inp, rates, errors={t: 1.0 + EPS8})["grad"] - ref["grad"]
        assert _rel_l2(eps, -EPS8 * off) <= 1e-6         # (a difference of two fp64 gradients 2^-8 of a share apart)
    # the pressure entry of the output-bias gradient is the pressure seed's sum, and nothing else's
    assert _p_entry(_run_model(c, inp, rates, errors={"seed_p": 0.0})["grad"], c)[0] == 0.0
    assert _p_entry(ref["grad"], c)[0] != 0.0
    with pytest.raises(AssertionError):
        _run_model(c, inp, rates, errors={"seed_w": 1.0})


def test_eq4_on_q_is_the_gradient_of_its_own_loss():
    """eq4_on_q=True is a consistent other loss - eq4 on q1, q2 - so the knob is the mistake itself, not noise: its
    gradient equals central differences of its loss_e along a random direction."""
    c = ROWS_EV[0]
    inp = _inputs(c)
    kw = dict(vis_t=np.asarray(hb._vis_t(c, inp), np.float64), w=inp["w"].astype(np.float64), scale=inp["scale"],
              e=inp["e"], errors={"eq4_on_q": True})
    flat = inp["flat"].astype(np.float64)
    term = lambda p: pm.residual_term(fr.unflatten(p, 2, 3, c["L"], c["H"]), inp["x"], inp["y"], RE, inp["anchor"], 0.7, 0.3, **kw)
    d = np.random.RandomState(1).randn(flat.size)
    d /= np.linalg.norm(d)
    h = 1e-6
    fd = (term(flat + h * d)["loss_e"] - term(flat - h * d)["loss_e"]) / (2.0 * h)
    g = float(term(flat)["grad"] @ d)
    assert abs(fd - g) <= 1e-7 * abs(g), (fd, g)


# --------------------------------------------------------------------------------------------------------------------
# CPU: the table against the library, without a device
# --------------------------------------------------------------------------------------------------------------------
def test_the_table_is_what_the_module_says():
    assert [c["H"] for c in ROWS_WIDTH] == [h for h in (8, 16, 50, 80, 128, 200, 256, 330, 400, 512) for _ in (0, 1)]
    assert len(ROWS_COLS64) == 2 and len(ROWS_MIXED) == 6 and len(ROWS_SPLIT) == 5 and len(ROWS_WALLS) == 7
    assert len(ROWS_EV) == 2 and len(ROWS_LOOP) == 3 and len({c["tag"] for c in ROWS}) == len(ROWS)
    assert [c["names"][:2] + (c["path"],) for c in ROWS_WALLS] == [
        ("fwd_kernel", "bwd_kernel", PLAIN), ("fwd_wide_kernel", "bwd_wide_kernel", PLAIN),
        ("fwd_bf16_kernel", "bwd_bf16_kernel", PLAIN), ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", PLAIN),
        ("fwd_split_kernel", "bwd_split_kernel", FUSED), ("fwd_split_kernel", "bwd_split_kernel", TWO),
        ("fwd_wsplit_kernel", "bwd_wsplit_kernel", WIDE)]
    assert {c["m"] for c in ROWS_WALLS} == {2, 3} and all(c["m"] is None for c in ROWS if c not in ROWS_WALLS)
    assert [(c["H"], c["path"]) for c in ROWS_SPLIT] == [(256, FUSED), (256, TWO), (288, WIDE), (330, WIDE), (448, WIDE)]
    assert [(c["L"], c["H"], c["n"], c["path"]) for c in ROWS_LOOP] == [(4, 50, "4cu", PLAIN), (3, 256, "loop", FUSED),
                                                                       (2, 400, "loop", WIDE)]
    assert [(c["L"], c["H"], c["prec"], c["path"]) for c in ROWS_EV] == [(4, 50, F32, PLAIN), (3, 256, X3, FUSED)]
    assert all(c["k"] == (K_WALLS if c["m"] is not None else K_EV if c["ev"] else K) for c in ROWS) and K == 4
    assert all(1.0 <= c["gain"] <= 3.0 and c["Re"] == 1.0 for c in ROWS)
    assert (-(-N // 32), N % 32, -(-N // 16), N % 16) == (3, 5, 5, 5)
    x, y, _ = _points(N, 1)
    sx, sy = hm.special_points()
    assert x.size == N and np.array_equal(x[:9], sx) and np.array_equal(y[:9], sy)
    inp = _inputs(ROWS_WALLS[0])
    assert inp["anchor"].shape == (3, N) and inp["anchor"].dtype == np.float32 and np.array_equal(inp["x"][:9], sx)
    # the looping counts: every workgroup of the 4x50 sweeps (4 per compute unit) takes a second tile, two workgroups
    # of the paired sweeps take a second pair and the last pair has a dummy partner
    assert _n(ROWS_LOOP[0]) == 4 * CUS * 32 + 5 and _n(ROWS_LOOP[1]) == (2 * CUS + 2) * 32 + 5
    assert _n(ROWS_LOOP[2]) == (2 * CUS + 2) * 16 + 5
    for c in ROWS_LOOP[1:]:
        g = geometry(_n(c), CUS, c["tile"], True, 1, c["L"])
        assert g["ntiles"] % 2 == 1 and g["loop"] == g["grid"] + 2, g


@pytest.mark.parametrize("c", ROWS, ids=_ids(ROWS))
def test_every_row_resolves_to_the_names_and_the_path_it_lists(lib, monkeypatch, capfd, c):
    """Through pinn_plan_create_pseudo_time (host-only) under the row's environment, with the row's walls."""
    for k in list(os.environ):
        if k.startswith("PINN_"):
            monkeypatch.delenv(k, raising=False)
    env = dict(c["env"])
    if env.pop(SWITCH, None) is not None:
        monkeypatch.setenv(SWITCH, "1")
    prec = tuple(CODE[p] for p in c["triple"])
    for n in sorted({_n(c), _n(c, 304)}):
        got, said = _path(lib, (c["H"], c["L"], prec, 4, n, env), _bc_of(c), capfd)
        assert got[1] == 0, got
        assert tuple(got[5:8]) == c["names"] and said == c["path"], (got, said)
        assert got[2] == -(-n // c["tile"]) * c["tile"], got


# --------------------------------------------------------------------------------------------------------------------
# CPU: conditions on the inputs, asserted on the model alone
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _nets(ROWS), ids=_ids(_nets(ROWS)))
def test_condition_a_no_cancellation_and_the_pressure_entry_carries_its_block(c):
    """A condition on the inputs, not a measurement: a row that does not meet it gets another seed or k."""
    A = {r: _amp(c, r) for r in REGIMES}
    pe, norm = _p_entry(_model(c, "P")["grad"], c)
    print("[ptime terms] %s: A %.2f (V) %.2f (P); pressure entry %.2f of the output-bias block in P" % (
        c["tag"], A["V"], A["P"], abs(pe) / norm))
    assert max(A.values()) <= 8.0, A
    assert abs(pe) >= 0.5 * norm, (pe, norm)
    assert _p_entry(_model(c, "V")["grad"], c)[0] == 0.0
    # the rates carry weight where they are on, and the sums are the steady ones where they are off
    for r, on in (("V", (0, 1)), ("P", (2,))):
        m = _model(c, r)
        for k in range(3):
            ratio = m["sums"][k] / m["steady_sums"][k]
            assert (abs(ratio - 1.0) > 0.05) if k in on else (ratio == 1.0), (r, k, ratio)


_OWN = [c for c in _nets(ROWS) if c["own"]]


@pytest.mark.parametrize("c", _OWN, ids=_ids(_OWN))
def test_condition_a_own_nets_carry_the_viscous_share(c):
    """The viscous-share condition of test_hardbc_terms for the nets that are not taken from its NETS."""
    r, r0 = _model(c, "steady"), _model(c, "inviscid")
    s = dict(eq1=_rel_max(r0["eqs"][0], r["eqs"][0]), eq2=_rel_max(r0["eqs"][1], r["eqs"][1]),
             grad=_rel_l2(r0["grad"], r["grad"]))
    print("[ptime terms] %s viscous share: %s" % (c["tag"], " ".join("%s %.2f" % kv for kv in s.items())))
    assert min(s.values()) >= SHARE_MIN, s


@pytest.mark.parametrize("c", ROWS_EV, ids=_ids(ROWS_EV))
def test_ev_rows_take_both_branches_of_the_viscosity_clamp(c):
    inp = _inputs(c)
    clamped = c["ev"]["alpha_evm"] * np.abs(inp["e"]) > 20.0 / c["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()


def _detected(c, regime, term, ex=None):
    """(error / bar, quantity) of the judged quantity a relative error 2^ex of `term` moves furthest (ex: 2^-8, or the
    power of two DETECT names for the row)."""
    ex = DETECT.get((c["tag"], regime, term), -8) if ex is None else ex
    got = _model(c, regime, ((term, 1.0 + 2.0 ** ex),))
    return _worst(_errs(c, regime, got, _model(c, regime), _amp(c, regime), planes=False))


@pytest.mark.parametrize("c", _nets(ROWS), ids=_ids(_nets(ROWS)))
def test_condition_b_an_error_of_one_bf16_term_in_any_piece_leaves_a_bar(c):
    """Per row, regime and term active in it: a 2^-8 relative error (one dropped low bf16 term) moves at least one
    judged quantity - a sum, a layer block, the pressure entry, grads_e - by more than 1.5 of its bar."""
    for regime in REGIMES:
        out = {t: _detected(c, regime, t) for t in ACTIVE[regime]}
        print("[ptime terms] %s %s: %s" % (c["tag"], regime, " ".join("%s %.1fx(%s)" % ((t,) + v) for t, v in out.items())))
        for t, (ratio, name) in out.items():
            assert ratio > MARGIN, (regime, t, ratio, name)


def test_detect_holds_smallest_powers_of_two_only():
    """An exception in DETECT is the smallest power of two that is seen on its row, and none is weaker than 2^-6."""
    tags = {c["tag"]: c for c in _nets(ROWS)}
    for (tag, regime, term), ex in DETECT.items():
        assert -8 < ex <= -6 and term in ACTIVE[regime] and tag in tags
        assert _detected(tags[tag], regime, term, ex - 1)[0] <= MARGIN, (tag, regime, term)


@pytest.mark.parametrize("c", ROWS_EV, ids=_ids(ROWS_EV))
def test_eq4_built_on_q_leaves_a_bar_on_the_ev_rows(c):
    """The mistake the header warns of - eq4 and its seeds on q1, q2 instead of the steady eq1, eq2 - moves a judged
    quantity of the ev rows past 1.5 bars (regime V: in regime P q1, q2 are the steady residuals)."""
    got = _model(c, "V", (("eq4_on_q", True),))
    ratio, name = _worst(_errs(c, "V", got, _model(c, "V"), _amp(c, "V")))
    print("[ptime terms] %s V eq4 on q: %s at %.1f bars" % (c["tag"], name, ratio))
    assert ratio > MARGIN, (ratio, name)
    same = _model(c, "P", (("eq4_on_q", True),))
    np.testing.assert_array_equal(same["grad"], _model(c, "P")["grad"])


@pytest.mark.parametrize("L,H,n", [(6, 256, 320), (3, 400, 150)], ids=["6x256", "3x400"])
def test_control_c_the_whole_vector_comparison_at_re_400_lets_the_seeds_go_missing(L, H, n):
    """Why the rows above exist: on the inputs of tests/test_pseudo_time_gpu.py, with its comparison - the whole
    gradient vector, the boundary gradient at alpha_b = 10 added, Re = 400, both rates on, bar 1e-4 max(1, A) - the
    pressure seed, or both velocity seeds, can be missing altogether at 1x the balanced rates (6x256), and a 2^-8
    relative error of either stays under the bar at 1x and at 10x (3x400: at 1x)."""
    c = ptg._problem(L, H, n, "plain")
    model = lambda s, sp, errors=None: pm.residual_term(c.P, c.x, c.y, ptg.RE, c.anchor, s, sp, alpha_e=ptg.ALPHA_E, errors=errors)
    sb, spb = pm.balanced_rates(model(1.0, 1.0))
    for mult in (1.0, 10.0):
        s, sp = float(np.float32(mult * sb)), float(np.float32(mult * spb))
        ref = model(s, sp)
        bar = ptg.BARS[X3]["grad"] * max(1.0, pm.amplification(ref, c.anchor, s, sp))
        share = _rel_l2(c.grad_v, c.grad_v + ref["grad"])
        moved = {}
        for name, errors in (("seed_p 2^-8", {"seed_p": 1.0 + EPS8}), ("seed_u, seed_v 2^-8", {"seed_u": 1.0 + EPS8, "seed_v": 1.0 + EPS8}),
                             ("seed_p off", {"seed_p": 0.0}), ("seed_u, seed_v off", {"seed_u": 0.0, "seed_v": 0.0})):
            moved[name] = _rel_l2(c.grad_v + model(s, sp, errors)["grad"], c.grad_v + ref["grad"])
        print("[ptime terms] Re=400 %dx%d N=%d %gx, boundary gradient %.4f of the judged vector, bar %.1e: %s" % (
            L, H, n, mult, share, bar, " ".join("%s %.1e" % kv for kv in moved.items())))
        if L == 6 or mult == 1.0:       # (3x400 at 10x, where the residual term is 0.1 of the vector, does see them)
            assert moved["seed_p 2^-8"] < bar and moved["seed_u, seed_v 2^-8"] < bar, moved
        if (L, mult) == (6, 1.0):
            assert moved["seed_p off"] < bar and moved["seed_u, seed_v off"] < bar, moved


# --------------------------------------------------------------------------------------------------------------------
# GPU: one pseudo-time loss_and_grad per row and regime against the model
# --------------------------------------------------------------------------------------------------------------------
def _engine(monkeypatch, capfd, c, inp):
    """A pseudo-time engine of the row's net, precision, switches and walls, after its plan named the row's kernels and
    said the row's path (test_pseudo_time_split_gpu._built)."""
    from nsfnet_amd import engine as eng
    from test_pseudo_time_split_gpu import _built
    hb._clear_env(monkeypatch)
    monkeypatch.delenv("NSFNET_GRAPH", raising=False)
    for k, v in c["env"]:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PINN_VERBOSE", "1")
    ev = c["ev"]
    kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=ev["alpha_evm"], coord_scale=inp["scale"]) if ev else {}

    def make():
        E = eng.PinnEngine(torch.device("cuda:0"), c["L"], c["H"], c["Re"], alpha_b=10.0, alpha_e=1.0, precision=c["prec"], **kw)
        if c["m"] is not None:
            E.set_hard_boundary(True, lift_power=c["m"])
        E.set_pseudo_time(dtau=1.0, every=1000, pressure_dtau=1.0)      # (placeholders: the plan gets the regime's rates)
        E.net.set_flat(torch.tensor(inp["flat"]))
        if ev:
            E.net_e.set_flat(torch.tensor(inp["flat_e"]))
            E.e_trainable = True
        E.set_collocation(inp["x"], inp["y"], weights=inp["w"])
        E.set_boundary(*hb._boundary(c))
        return E

    return _built(capfd, make, c["names"], c["path"])


def _evaluate(monkeypatch, capfd, c, regime):
    cus = _cus()
    inp, rates, n = _inputs(c, cus), _rates(c, regime, cus), _n(c, cus)
    if c["n"] == "4cu":
        assert n == ptg._points("4cu")
    if c["n"] == "loop":
        from test_pseudo_time_split_gpu import _n as split_n
        assert n == split_n("loop", c["H"])
    E = _engine(monkeypatch, capfd, c, inp)
    f = E.plan_f
    assert f.npad == -(-n // c["tile"]) * c["tile"] and (f.hard_bc() is not None) == (c["m"] is not None)
    if c["m"] is not None:
        assert f.hard_bc()["lift_power"] == c["m"]
    f.anchor[:, :n].copy_(torch.tensor(inp["anchor"]))
    f.set_pseudo_time(*rates)
    assert tuple(f.pseudo_time()) == rates              # the fp32 launch constants, as the model takes them
    before = f.anchor.clone()
    ev = c["ev"]
    got = dict(vtm0=f.vis_t_minus.cpu().numpy().astype(np.float64) if ev else None)
    E.loss_and_grad()
    got["grad"] = hb._residual_gradient(E, f)
    assert torch.equal(f.anchor, before)                # an evaluation never writes the anchors
    fld = lambda k: f.field(k).cpu().numpy().astype(np.float64)
    got.update(fields={k: fld(k) for k in PLANES}, eqs=[fld("eq%d" % (k + 1)) for k in range(4 if ev else 3)],
               sums=E.sums.cpu().numpy().astype(np.float64))
    if ev:
        got["grad_e"] = E.grads_e.cpu().numpy().astype(np.float64)
        got["vis_t"] = f.vis_t.cpu().numpy().astype(np.float64)
    del E, f
    torch.cuda.empty_cache()
    return inp, rates, n, got


def _judge(c, regime, rates, n, got, ref, inp):
    A = pm.amplification(ref, inp["anchor"], *rates)
    assert A <= 8.0, A
    errs = _errs(c, regime, got, ref, A)
    pe = _p_entry(got["grad"], c)[0]
    worst = lambda keys: max((errs[k][0], k) for k in keys)
    planes, sums = worst(PLANES + tuple(k for k in errs if k.startswith("eq"))), worst([k for k in errs if k.startswith("sum")])
    block = worst([k for k in errs if k[0] in "Wb"])
    print("[ptime terms] %s N=%d %s rates %.4g / %.4g A %.2f: plane %.2e (%s, bar %.0e) sum %.2e (%s, bar %.1e) "
          "block %.2e (%s%s, bar %.1e) pressure entry %s" % (
              c["tag"], n, regime, rates[0], rates[1], A, planes[0], planes[1], errs[planes[1]][1], sums[0], sums[1],
              errs[sums[1]][1], block[0], block[1], "; grads_e %.2e" % errs["grad_e"][0] if c["ev"] else "", errs[block[1]][1],
              "%.1e == 0" % pe if regime == "V" else "%.3e, off by %.2e" % (pe, errs["dbo2"][0])))
    if regime == "V":
        assert pe == 0.0, pe                            # ap is 0 times a finite number
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


_GPU_PLAIN = [(c, r) for c in ROWS if not c["ev"] for r in REGIMES]
_GPU_EV = [(c, r) for c in ROWS_EV for r in REGIMES]
_gpu_ids = lambda cases: ["%s %s" % (c["tag"], r) for c, r in cases]


@pytest.mark.gpu
@pytest.mark.parametrize("c,regime", _GPU_PLAIN, ids=_gpu_ids(_GPU_PLAIN))
def test_pseudo_time_term_vs_model(monkeypatch, capfd, c, regime):
    inp, rates, n, got = _evaluate(monkeypatch, capfd, c, regime)
    _judge(c, regime, rates, n, got, _model(c, regime, cus=_cus()), inp)


@pytest.mark.gpu
@pytest.mark.parametrize("c,regime", _GPU_EV, ids=_gpu_ids(_GPU_EV))
def test_pseudo_time_term_ev_vs_model(monkeypatch, capfd, c, regime):
    """vis_t is the run's own, so the model run is this case's; both branches of the clamp are taken on the device,
    and the evaluation leaves vis_t as the plain path does: min(20 / Re, vis_t_minus)."""
    inp, rates, n, got = _evaluate(monkeypatch, capfd, c, regime)
    assert _rel_max(got["vtm0"], c["ev"]["alpha_evm"] * np.abs(inp["e"])) <= BARS[c["bar"]]["eq"]
    vis_t = hb._vis_t(c, inp, got["vtm0"])
    np.testing.assert_allclose(got["vis_t"], vis_t, rtol=1e-6)
    clamped = got["vtm0"] > 20.0 / c["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()
    _judge(c, regime, rates, n, got, _run_model(c, inp, rates, vis_t=vis_t), inp)
