"""The residual term judged alone, where the viscous term dominates: Re = 1 (and Re = 1e-3 for the field planes).

Every other oracle comparison of the hot-path kernels runs at Re >= 100 and compares the total gradient at
alpha_b = 10.  Two blind spots follow ("The residual term alone"):
  * The Laplacian stream z_D - the d2 * (zx*zx + zy*zy) + d1 * zd chain, the d3 term of the reverse chain, the
    -nu * r * sc2 seeds - enters nothing but eq1 / eq2 with weight nu = 1/Re + vis_t.  At Re = 400..2000 the whole
    viscous term is 3e-4..4e-3 of max|eq| and 2e-4..1e-3 of the residual gradient: it could be zero and the bf16x3 field
    bar would still hold.
  * On a freshly seeded net the boundary term owns the total gradient: the residual term's share of a layer block is
    1e-5..7e-2, so a 1e-4 bar on the total judges the reverse sweep and dW - the step's cost - at a weight of ~1 %.
Here nu is 1 (1000), where the viscous term is >= 0.25 of max|eq1|, of max|eq2| and of the residual gradient on every
net used (>= 0.99 of the eq planes at Re = 1e-3), and the residual gradient is taken alone (grad_reduce over plan_f
only) and compared per layer block with the oracle's pde_loss_and_grad, no boundary term added.

N = 69 for every case: three tiles of 32 (the paired sweeps get an odd tile count, hence a dummy partner, and a ragged
last tile of 5 points), five tiles of 16 for the 64-column kernels.  Looping point counts are test_tile_loops.py's and
test_kernel_pairings.py's business, not this module's.

The CPU tests keep the table honest: every row resolves to the kernels it names, every case meets the viscous-share
condition on the oracle, and three sensitivity controls show that a 2^-8 relative error of the viscous term leaves the
bars here while the existing comparisons (Re = 1500..2000, boundary gradient added) would let it pass.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fwdmode_ref as fr

from test_tile_loops import BARS, _bc, _net, _points, _rel_l2, _rel_max
from test_kernel_pairings import CODE, F32, ROWS_256, ROWS_400, TILE_LOOPS_256, X3, _row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import plan_census  # noqa: E402

N = 69
EPS8 = 2.0 ** -8          # one dropped low bf16 term of a bf16x3 operand
SHARE_MIN = 0.25          # the viscous term's share of max|eq1|, max|eq2| and the residual gradient at Re = 1
SHARE_MIN_LAP = 0.99      # ... of max|eq1| and max|eq2| at Re = 1e-3: the planes are the Laplacian's
RE_LAP = 1.0e-3

# Residual-gradient bar per layer block (rel-L2 against that block of the oracle's residual gradient).  fp32 triples:
# the project's gradient bar; a numpy-fp32 restatement of the oracle sits at 2.3e-7, a margin of > 400.  Rows with a
# bf16 member: the same bar, BARS["bf16x3"]["grad"] - no bar here is set from the emulation.  What bf16x3 arithmetic
# itself gives (oracle/bf16x3_emul.py against the fp64 oracle, the plain cases of this table): worst gradient block
# 2.0e-7 (1x8) .. 3.0e-5 (3x330; 2.0e-5 at 6x256, 7.2e-6 at 4x400), fields <= 7.3e-5 of max, sums <= 3.9e-5 - inside the
# bars by 3.4x (gradient), 6.9x (fields) and 5x (sums) at the least; test_bf16x3_arithmetic_reaches_the_bars keeps that.
GRAD_BAR = {F32: BARS[F32]["grad"], X3: BARS[X3]["grad"]}
EMUL_MARGIN = 3.0         # the emulation's error stays this factor inside every bf16x3 bar of a plain case


def _tile(H, fp32):
    hp = (H + 31) // 32 * 32
    return 16 if hp > 256 or (hp == 256 and fp32) else 32


def _names(H, prec):
    """The default kernel triple of a uniform precision at N = 69 (pinn_plan_create; pinned by the census test)."""
    hp = (H + 31) // 32 * 32
    if prec == F32:
        return ("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel") if hp >= 256 else \
            ("fwd_kernel", "bwd_kernel", "dw_kernel")
    if hp < 256:
        return ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")
    if hp == 256:
        return ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
    if hp <= 448:
        return ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")
    return ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel")


def _plain(H, prec):
    return _row(prec, _names(H, prec), _tile(H, prec == F32))


def _case(L, H, seed, pts, row, Re=1.0, ev=None, grad=True):
    tag = "%dx%d%s %s Re=%g" % (L, H, "+4x40 ev" if ev else "", row["tag"], Re)
    return dict(L=L, H=H, seed=seed, pts=pts, row=row, Re=Re, ev=ev, grad=grad, tag=tag)


# 6x256, net seed 1234: every name triple of ROWS_256 and of test_tile_loops.py (the fused role-split default, the
# 8-wave bf16 kernels, fp32's 64-column kernels)
_TILE_LOOPS_ROWS = [_row(X3, TILE_LOOPS_256[0], 32), _row(X3, TILE_LOOPS_256[1], 32, (("PINN_SCHED", "0"),)),
                    _row(F32, TILE_LOOPS_256[2], 16)]
CASES_256 = [_case(6, 256, 1234, 11, r) for r in _TILE_LOOPS_ROWS + ROWS_256]
# 4x400, net seed 31: ROWS_400 and the two $PINN_WSPLIT rows of test_wide_4x400_loops_vs_oracle
_WSPLIT_ROWS = [_row(X3, ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel"), 16, (("PINN_WSPLIT", "1"),)),
                _row(X3, ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel"), 16,
                     (("PINN_WSPLIT", "0"),))]
CASES_400 = [_case(4, 400, 31, 13, r) for r in _WSPLIT_ROWS + ROWS_400]
# the narrow families (one to eight waves, 32-point tiles) and the wide widths (role-split 288..448, 8-wave wide 512)
# (L, H, net seed): seeds 50 + L (70 + L), but 1x8 and 6x128, whose viscous share of max|eq1| those seeds leave at 0.14 / 0.23
NARROW = [(1, 8, 52), (2, 16, 52), (4, 50, 54), (3, 96, 53), (6, 128, 57), (3, 200, 53)]
WIDE = [(2, 288, 72), (3, 330, 73), (2, 448, 72), (2, 512, 72)]
CASES_NARROW = [_case(L, H, seed, 15, _plain(H, p)) for L, H, seed in NARROW for p in (F32, X3)]
CASES_WIDE = [_case(L, H, seed, 17, _plain(H, p)) for L, H, seed in WIDE for p in (F32, X3)]
# ev flavour: per-point weights, coord_scale 2, a trainable 4x40 entropy net; alpha_evm puts alpha_evm * |e| on either
# side of 20 / Re, so that vis_t = min(20 / Re, vis_t_minus) takes both branches (asserted on the oracle's e)
CASES_EV = [
    _case(6, 256, 21, 12, _plain(256, X3), ev=dict(seed=22, alpha_evm=600.0)),
    _case(4, 50, 61, 18, _plain(50, F32), ev=dict(seed=62, alpha_evm=150.0)),
    _case(3, 400, 71, 19, _plain(400, X3), ev=dict(seed=72, alpha_evm=80.0)),
]
# Re = 1e-3, field planes and sums only: eq1 / eq2 are the Laplacian planes to 1e-3.  One row per forward kernel name.
CASES_LAP = [
    _case(4, 50, 54, 15, _plain(50, F32), Re=RE_LAP, grad=False),                       # fwd_kernel
    _case(6, 256, 1234, 11, _TILE_LOOPS_ROWS[2], Re=RE_LAP, grad=False),                # fwd_wide_kernel
    _case(4, 50, 54, 15, _plain(50, X3), Re=RE_LAP, grad=False),                        # fwd_bf16_kernel
    _case(6, 256, 1234, 11, ROWS_256[6], Re=RE_LAP, grad=False),                        # fwd_pipe_kernel
    _case(6, 256, 1234, 11, _TILE_LOOPS_ROWS[0], Re=RE_LAP, grad=False),                # fwd_split_kernel
    _case(4, 400, 31, 13, _WSPLIT_ROWS[1], Re=RE_LAP, grad=False),                      # fwd_bf16_wide_kernel
    _case(4, 400, 31, 13, _WSPLIT_ROWS[0], Re=RE_LAP, grad=False),                      # fwd_wsplit_kernel
]
CASES_RE1 = CASES_256 + CASES_400 + CASES_NARROW + CASES_WIDE + CASES_EV
CASES = CASES_RE1 + CASES_LAP
_ids = lambda cases: [c["tag"] for c in cases]


# --------------------------------------------------------------------------------------------------------------------
# inputs and the oracle
# --------------------------------------------------------------------------------------------------------------------
def _inputs(c):
    """Net, points (and the ev flavour's weights, scale and entropy net) of a case: float32, as the engine holds them."""
    ev = c["ev"]
    x, y, rng = _points(N, c["pts"], *((-1.0, 1.0) if ev else (0.0, 1.0)))
    out = dict(flat=_net(c["L"], c["H"], c["seed"]), x=x, y=y, w=None, scale=1.0, flat_e=None, e=None, Pe=None)
    if ev:
        out.update(w=(0.3 + rng.rand(N)).astype(np.float32), scale=2.0, flat_e=_net(4, 40, ev["seed"], n_out=1))
        out["Pe"] = fr.unflatten(out["flat_e"].astype(np.float64), 2, 1, 4, 40)
        out["e"] = fr.forward1(out["Pe"], x.astype(np.float64), y.astype(np.float64))[0][:, 0]
    return out


def _vis_t(c, inp, vtm=None):
    """min(20 / Re, alpha_evm |e|) as the forward sweep takes it, from the oracle's e (or a plan's vis_t_minus)."""
    if not c["ev"]:
        return None
    vtm = c["ev"]["alpha_evm"] * np.abs(inp["e"]) if vtm is None else vtm
    return np.minimum(np.float32(20.0 / c["Re"]), vtm)


def _oracle_run(c, inp, Re, vis_t, nu_factor=1.0):
    """pde_loss_and_grad of a case at nu = nu_factor * (1 / Re + vis_t), no boundary term."""
    P = fr.unflatten(inp["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
    kw = {}
    if c["ev"]:
        kw = dict(vis_t=nu_factor * np.asarray(vis_t, np.float64), w=inp["w"].astype(np.float64), scale=inp["scale"],
                  params_e=inp["Pe"])
    return fr.pde_loss_and_grad_chunked(P, inp["x"], inp["y"], Re / nu_factor, **kw)


_CACHE = {}


def _key(c):
    return (c["L"], c["H"], c["seed"], c["pts"], c["Re"], None if not c["ev"] else tuple(sorted(c["ev"].items())))


def _oracle(c, what="ref"):
    """Oracle runs of a case's net, points and Re, shared by the rows that differ only in kernels: 'ref' at nu,
    'inviscid' at Re = 1e30 without vis_t, 'eps' at nu * (1 + 2^-8)."""
    k = _key(c) + (what,)
    if k not in _CACHE:
        inp = _inputs(c)
        vt = _vis_t(c, inp)
        if what == "ref":
            _CACHE[k] = _oracle_run(c, inp, c["Re"], vt)
        elif what == "inviscid":
            _CACHE[k] = _oracle_run(c, inp, 1.0e30, None if vt is None else 0.0 * vt)
        else:
            _CACHE[k] = _oracle_run(c, inp, c["Re"], vt, 1.0 + EPS8)
    return _CACHE[k]


def _blocks(g, n_out, L, H):
    return [q for wb in fr.unflatten(np.asarray(g, np.float64), 2, n_out, L, H) for q in wb]


def _block_errs(a, b, n_out, L, H, ref=None):
    """rel-L2 distance of a from b in every layer's weight and bias block, against that block of ref (default b)."""
    ref = b if ref is None else ref
    return [float(np.linalg.norm(p - q) / max(np.linalg.norm(r), 1e-300))
            for p, q, r in zip(_blocks(a, n_out, L, H), _blocks(b, n_out, L, H), _blocks(ref, n_out, L, H))]


def _shares(c):
    """The viscous term's share of max|eq1|, max|eq2| and of the residual gradient: the run at Re against Re = 1e30."""
    r, r0 = _oracle(c), _oracle(c, "inviscid")
    return dict(eq1=_rel_max(r0["eqs"][0], r["eqs"][0]), eq2=_rel_max(r0["eqs"][1], r["eqs"][1]),
                grad=_rel_l2(r0["grad"], r["grad"]))


def _nets(cases):
    """One case per distinct net / points / Re / ev setting."""
    seen = {}
    for c in cases:
        seen.setdefault(_key(c), c)
    return list(seen.values())


# --------------------------------------------------------------------------------------------------------------------
# CPU: the table, the viscous-share condition, the sensitivity controls
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def test_the_table_is_what_the_module_says():
    assert len(CASES_256) == 16 and len({c["row"]["names"] + c["row"]["env"] for c in CASES_256}) == 16
    assert {c["row"]["names"] for c in CASES_256} == {r["names"] for r in ROWS_256} | set(TILE_LOOPS_256)
    assert len(CASES_400) == 7 and len(CASES_NARROW) == 12 and len(CASES_WIDE) == 8 and len(CASES_EV) == 3
    assert [c["row"]["names"][0] for c in CASES_LAP] == [
        "fwd_kernel", "fwd_wide_kernel", "fwd_bf16_kernel", "fwd_pipe_kernel", "fwd_split_kernel",
        "fwd_bf16_wide_kernel", "fwd_wsplit_kernel"]
    assert len({c["tag"] for c in CASES}) == len(CASES)
    # three tiles of 32 with a ragged last one of 5; five tiles of 16
    assert (-(-N // 32), N % 32, -(-N // 16), N % 16) == (3, 5, 5, 5)


@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_every_row_resolves_to_the_names_it_lists(lib, c):
    row = c["row"]
    got = plan_census.run_case(lib, (c["H"], c["L"], tuple(CODE[p] for p in row["triple"]), 4, N, dict(row["env"])))
    assert got[1] == 0, got
    assert tuple(got[5:8]) == row["names"]
    assert got[2] == -(-N // row["tile"]) * row["tile"]


@pytest.mark.parametrize("c", _nets(CASES), ids=_ids(_nets(CASES)))
def test_the_viscous_term_carries_its_share(c):
    """A condition on the inputs, not a measurement: a row that does not meet it gets another seed."""
    s = _shares(c)
    print("[residual term] %dx%d seed %d Re=%g viscous share: %s" % (
        c["L"], c["H"], c["seed"], c["Re"], " ".join("%s %.2f" % kv for kv in s.items())))
    assert min(s.values()) >= SHARE_MIN, s
    if c["Re"] == RE_LAP:
        assert min(s["eq1"], s["eq2"]) >= SHARE_MIN_LAP, s


@pytest.mark.parametrize("c", CASES_EV, ids=_ids(CASES_EV))
def test_ev_cases_take_both_branches_of_the_viscosity_clamp(c):
    inp = _inputs(c)
    clamped = c["ev"]["alpha_evm"] * np.abs(inp["e"]) > 20.0 / c["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()


def _eq_moves(c):
    """max-abs / max|ref| distance of eq1 and eq2 from themselves with the viscous part scaled by 1 + 2^-8."""
    r, r0 = _oracle(c), _oracle(c, "inviscid")
    return [_rel_max(r["eqs"][k] + EPS8 * (r["eqs"][k] - r0["eqs"][k]), r["eqs"][k]) for k in (0, 1)]


@pytest.mark.parametrize("c", _nets(CASES_RE1), ids=_ids(_nets(CASES_RE1)))
def test_control_a_viscous_error_of_one_bf16_term_leaves_the_field_bar(c):
    assert min(_eq_moves(c)) > BARS[X3]["eq"], _eq_moves(c)


@pytest.mark.parametrize("shape,Re", [("6x256", 2000.0), ("4x400", 1500.0)])
def test_control_a_the_same_error_passes_at_the_existing_reynolds_numbers(shape, Re):
    c = dict((CASES_256 if shape == "6x256" else CASES_400)[0], Re=Re)
    assert max(_eq_moves(c)) < BARS[X3]["eq"], _eq_moves(c)


def _grad_moves(c, plus=None):
    """Per-block rel-L2 change of the residual gradient from nu to nu * (1 + 2^-8), against the residual gradient's
    block (or that of the residual gradient + plus)."""
    r, r1 = _oracle(c), _oracle(c, "eps")
    return _block_errs(r1["grad"], r["grad"], 3, c["L"], c["H"], None if plus is None else r["grad"] + plus)


@pytest.mark.parametrize("c", _nets(CASES_RE1), ids=_ids(_nets(CASES_RE1)))
def test_control_b_viscous_error_of_one_bf16_term_moves_every_gradient_block(c):
    moved = _grad_moves(c)
    print("[residual term] %dx%d Re=%g nu * (1 + 2^-8): blocks move %.2e .. %.2e" % (
        c["L"], c["H"], c["Re"], min(moved), max(moved)))
    assert min(moved) > max(GRAD_BAR.values()), moved


def test_control_c_the_boundary_gradient_hides_the_same_error_at_re_2000():
    c = dict(CASES_256[0], Re=2000.0)
    inp = _inputs(c)
    P = fr.unflatten(inp["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
    xb, yb, ub, vb = _bc()
    b = fr.bc_loss_and_grad(P, xb.astype(np.float64), yb.astype(np.float64), ub, vb, alpha_b=10.0)
    moved = _grad_moves(c, plus=b["grad"])
    print("[residual term] 6x256 Re=2000 + boundary gradient, nu * (1 + 2^-8): blocks move %.2e .. %.2e" % (
        min(moved), max(moved)))
    assert max(moved) < 1e-4, moved


_PLAIN_NETS = [c for c in _nets(CASES) if not c["ev"]]


@pytest.mark.parametrize("c", _PLAIN_NETS, ids=_ids(_PLAIN_NETS))
def test_bf16x3_arithmetic_reaches_the_bars(c):
    """The bf16x3 bars are reachable here by correct arithmetic: a numpy emulation of the number formats (operands
    split in two bf16 terms, three products, fp32 accumulation, the 24-bit spill), which is not the kernels' code,
    stays EMUL_MARGIN inside them on every plain net of the table."""
    from oracle import bf16x3_emul as em
    inp, r = _inputs(c), _oracle(c)
    e = em.residual_loss_and_grad(inp["flat"], inp["x"], inp["y"], c["Re"], c["L"], c["H"])
    errs = dict(eq=max(_rel_max(e["eqs"][k], r["eqs"][k]) for k in range(3)),
                sums=_rel_max(e["sums"], np.asarray(r["sums"])),
                grad=max(_block_errs(e["grad"], r["grad"], 3, c["L"], c["H"])))
    print("[residual term] %dx%d Re=%g bf16x3 emulation: %s" % (
        c["L"], c["H"], c["Re"], " ".join("%s %.2e" % kv for kv in errs.items())))
    assert EMUL_MARGIN * errs["eq"] <= BARS[X3]["eq"] and EMUL_MARGIN * errs["sums"] <= BARS[X3]["sums"], errs
    assert EMUL_MARGIN * errs["grad"] <= GRAD_BAR[X3], errs


def test_bf16x3_emulation_formats():
    from oracle import bf16x3_emul as em
    one = np.float32(1.0)
    x = np.array([one + 2.0 ** -8, one + 3 * 2.0 ** -8, one + 2.0 ** -8 + 2.0 ** -20, -(one + 2.0 ** -7)], np.float32)
    # round to nearest even on 8 significant bits: ties to 1 and to 1 + 2^-6, above the tie up, exact kept
    np.testing.assert_array_equal(em.bf16(x), np.array([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)], np.float32))
    rng = np.random.RandomState(0)
    v = (rng.randn(4096) * 10.0 ** rng.uniform(-6, 3, 4096)).astype(np.float32)
    hi, lo = em.split(v)
    assert np.abs((hi.astype(np.float64) + lo) - v).max() / np.abs(v).max() <= 2.0 ** -17
    assert (np.abs(hi.astype(np.float64) + lo - v) <= 2.0 ** -17 * np.abs(v)).all()
    r24 = em.round24(v)
    assert (r24.view(np.uint32) & 0xFF == 0).all() and (np.abs(r24.astype(np.float64) - v) <= 2.0 ** -16 * np.abs(v)).all()
    a, b = rng.randn(7, 33).astype(np.float32), rng.randn(33, 5).astype(np.float32)
    exact = a.astype(np.float64) @ b
    assert 1e-8 < np.abs(em.mm3(a, b) - exact).max() / np.abs(exact).max() < 2.0 ** -15


# --------------------------------------------------------------------------------------------------------------------
# GPU: one loss_and_grad per case, the residual term's fields, sums and gradient against the oracle
# --------------------------------------------------------------------------------------------------------------------
def _run(monkeypatch, c):
    from nsfnet_amd import engine as eng
    for k in list(os.environ):
        if k.startswith("PINN_") or k == "NSFNET_CHUNK_POINTS":
            monkeypatch.delenv(k, raising=False)
    row, ev, inp = c["row"], c["ev"], _inputs(c)
    for k, v in row["env"]:
        monkeypatch.setenv(k, v)
    kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=ev["alpha_evm"], coord_scale=inp["scale"]) if ev else {}
    dev = torch.device("cuda:0")
    E = eng.PinnEngine(dev, c["L"], c["H"], c["Re"], alpha_b=10.0, alpha_e=1.0, precision=row["prec"], **kw)
    E.net.set_flat(torch.tensor(inp["flat"]))
    if ev:
        E.net_e.set_flat(torch.tensor(inp["flat_e"]))
        E.e_trainable = True
    E.set_collocation(inp["x"], inp["y"], weights=inp["w"])
    E.set_boundary(*_bc())
    assert E.plan_f.kernel_names() == row["names"]
    assert E.plan_f.npad == -(-N // row["tile"]) * row["tile"]
    got = dict(vtm0=E.plan_f.vis_t_minus.cpu().numpy().astype(np.float64) if ev else None)
    E.loss_and_grad()
    # the residual term's gradient alone: the assembly over the residual plan only, as test_value_loops.py isolates a
    # value plan (loss_and_grad's own assembly has added the boundary plan's)
    gr = torch.full((E.net.num_params,), float("nan"), dtype=torch.float32, device=dev)
    eng.grad_reduce(E.net, [E.plan_f], gr)
    torch.cuda.synchronize()
    fields = ("eq1", "eq2", "eq3", "eq4") if ev else ("eq1", "eq2", "eq3")
    got.update(eqs=[E.plan_f.field(k).cpu().numpy().astype(np.float64) for k in fields],
               sums=E.sums.cpu().numpy().astype(np.float64), grad=gr.cpu().numpy().astype(np.float64))
    if ev:
        got["grad_e"] = E.grads_e.cpu().numpy().astype(np.float64)
        got["vis_t"] = E.plan_f.vis_t.cpu().numpy().astype(np.float64)
    del E
    torch.cuda.empty_cache()
    return inp, got


def _compare(c, got, ref):
    bar, gbar = BARS[c["row"]["bar"]], GRAD_BAR[c["row"]["bar"]]
    errs = {}
    for k, q in enumerate(got["eqs"]):
        errs["eq%d" % (k + 1)] = _rel_max(q, ref["eqs"][k])
    nq = len(got["eqs"])
    errs["sums"] = _rel_max(got["sums"][:nq], np.asarray(ref["sums"]))
    blocks = blocks_e = []
    if c["grad"]:
        assert np.isfinite(got["grad"]).all()
        blocks = _block_errs(got["grad"], ref["grad"], 3, c["L"], c["H"])
        errs["grad_r"] = max(blocks)
        if c["ev"]:
            blocks_e = _block_errs(got["grad_e"], ref["grad_e"], 1, 4, 40)
            errs["grad_e"] = max(blocks_e)
    print("[residual term] %s N=%d: %s" % (c["tag"], N, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k in [k for k in errs if k.startswith("eq")]:
        assert errs[k] <= bar["eq"], (k, errs[k])
    assert errs["sums"] <= bar["sums"], ("sums", errs["sums"])
    if c["grad"]:
        assert errs["grad_r"] <= gbar, ("residual gradient blocks", blocks)
        if c["ev"]:
            assert errs["grad_e"] <= gbar, ("entropy net gradient blocks", blocks_e)


_GPU_PLAIN = [c for c in CASES if not c["ev"]]


@pytest.mark.gpu
@pytest.mark.parametrize("c", _GPU_PLAIN, ids=_ids(_GPU_PLAIN))
def test_residual_term_vs_oracle(monkeypatch, c):
    _, got = _run(monkeypatch, c)
    _compare(c, got, _oracle(c))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES_EV, ids=_ids(CASES_EV))
def test_residual_term_ev_vs_oracle(monkeypatch, c):
    """vis_t is the run's own (the entropy net runs in the row's precision: its output carries that mode's field
    error), so the oracle run is this case's; both branches of the clamp are taken on the device too."""
    inp, got = _run(monkeypatch, c)
    assert _rel_max(got["vtm0"], c["ev"]["alpha_evm"] * np.abs(inp["e"])) <= BARS[c["row"]["bar"]]["eq"]
    vis_t = _vis_t(c, inp, got["vtm0"])
    np.testing.assert_allclose(got["vis_t"], vis_t, rtol=1e-6)
    clamped = got["vtm0"] > 20.0 / c["Re"]
    assert 0.1 * N <= clamped.sum() <= 0.9 * N, clamped.sum()
    _compare(c, got, _oracle_run(c, inp, c["Re"], vis_t))
