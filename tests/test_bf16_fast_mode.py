"""The plain-bf16 kernels (precision "bf16", code 2: one MFMA per product) against an emulation of their arithmetic.

What is blind without this module.  Half of the bf16 template instantiations are the TERMS == 1 ones, with their own
branches (no lo image restaged, no lo weight ring, one MFMA per k-step), and bench.py times the mode next to the
headline.  The suite judged them by four oracle comparisons at 3-6 %, all on default kernels: the pipelined, unfused,
8-wave-at-256, 64-column and classic-spill wide sweeps, dw_bf16 recomputing layer 0, every mixed triple with a code-2
member and the value-mode instantiations had never run in plain bf16 under a test.  An oracle comparison cannot close
that: the format's own error is 0.4-5 %, so a stream dropped by 1 % passes, and a role that ignores `terms` and runs
three products is MORE accurate than asked for (controls below) while bench.py reports its time as one product's.

The reference here is oracle/bf16x3_emul.py run with one term: the same number formats as the kernels, in numpy, in its
own summation order.  Two correct implementations of one format differ only where fp32 summation order flips a bf16
rounding.  That spread is measured on the emulation itself:
  noise[q]   the largest pairwise distance among twelve variants (accumulation fp32 / fp64 / fp32 in k-blocks of 16,
             tanh from libm / the kernels' exp2 form, layer 0 as rounded products / as the kernels' two fmaf), all at the
             row's precisions and spill;
  format[q]  the distance of the row's emulation (fp32 accumulation, fmaf layer 0; the exp2 tanh where the forward role
             is not fp32) from the fp64 oracle;
  bar[q]     4 * noise[q] - factor 4 for the kernels' own summation order, as test_rwf_gpu.TRAJECTORY_BARS sets 4 x the
             reference's own divergence.  No bar comes from what a kernel gave.
for q = eq (worst rel-L2 of the planes eq1..3), sums (worst relative error of the three sums), grad (worst rel-L2 over
the weight and bias block of each layer of the residual gradient taken alone) and gradw (the same over the hidden
layers' weight blocks, the dW GEMMs' own output); value mode: pred, the two boundary sums, the boundary gradient's
blocks.  Every distance is in units of the ORACLE's norm of that plane, sum or block, so the triangle inequality holds
between kernel, emulation and oracle.  Planes are judged in rel-L2: one flipped rounding moves one point of a plane by
up to 2e-2 of its max (max-abs is printed only).  Conditions on the inputs, met by choosing seed and depth:
4 * noise <= format / 4 wherever a plain-bf16 role feeds the quantity (the comparison is then
>= 4 x sharper than any oracle comparison could be), and the viscous share of test_residual_term (>= 0.25 at Re = 1).
The seeds are also chosen where the variants DO differ by flipped roundings (noise of the planes >= 3e-5): on a net
where none of them flips one the bar collapses to fp32 rounding and a single flip on the device would leave it.
A quantity that passes through no bf16 split - eq and sums behind an fp32 forward sweep - is an fp32 kernel's, not this
module's subject: it keeps the fp32 bar against the oracle that test_residual_term holds it to.

Cases: N = 69 residual points (three 32-point tiles with a ragged last one of 5, five 16-point tiles, an odd tile count
for the paired sweeps' dummy partner), Re = 1, three hidden layers (noise grows with depth; here it is 18 x or more
below the format error; hidden 512 runs depth 2, see WIDE).  Rows: the plain-bf16 twin of every row with a bf16x3 member
that test_kernel_pairings.ROWS_256 / ROWS_400 / TILE_LOOPS_256 and the $PINN_WSPLIT rows run, the mixed triples with
code 2 in one role only, the narrow widths 16..200 and the wide widths 288..512, and the boundary (value) plan at hidden 50,
128, 256, 400 with 150 points.

What the emulation had to learn from the kernels (each an option of the emulation, chosen per row from the kernel
names the census reports, csrc/spill.h and the forward kernels' output layers):
  * the 8-wave sweeps fwd_bf16 / fwd_bf16_wide feed the output layer from the LDS operand image - in plain bf16 the last
    a-streams rounded to bf16, with fp32 weights - while the pipelined and role-split sweeps feed it the fp32 streams;
  * in SPILL_P24_WIDE layer 0's saved quad passes through the 24-bit spill on its way to dw_bf16_wide, and behind the
    8-wave wide sweeps on its way to bwd_bf16_wide too; the hidden-256 role-split plans recompute it everywhere.

Measured on an MI355X, 2026-10-19 (eq / sums / grad; the whole table is in DESIGN.md section 6, "The plain-bf16 kernels
against their arithmetic"): all 34 residual and 4 value rows inside their bars.  Distance of the device from the
emulation | bar | format error:
  3x256 fused and unfused role-split    5.2e-5 / 1.6e-5 / 5.8e-5 | 3.4e-4 / 1.1e-4 / 2.1e-4 | 7.1e-3 / 1.0e-2 / 4.7e-3
  3x256 pipelined                       5.2e-5 / 1.6e-5 / 5.9e-5 | 3.4e-4 / 1.1e-4 / 2.0e-4 | 7.1e-3 / 1.0e-2 / 4.7e-3
  3x256 8-wave, 128 and 64 columns      1.7e-4 / 2.9e-5 / 7.1e-5 | 6.0e-4 / 1.5e-4 / 2.8e-4 | 7.4e-3 / 1.1e-2 / 5.1e-3
  3x400 wide role-split                 1.3e-5 / 1.7e-6 / 2.3e-5 | 1.5e-4 / 1.6e-5 / 1.3e-4 | 1.4e-2 / 5.5e-3 / 4.4e-3
  3x400 8-wave wide, either spill       7.5e-5 / 8.7e-6 / 6.4e-5 | 6.1e-4 / 3.0e-4 / 4.2e-4 | 1.8e-2 / 5.7e-3 / 4.4e-3
  3x50, the row closest to its bar      3.4e-4 / 1.2e-5 / 6.0e-5 | 4.7e-4 / 1.1e-4 / 1.5e-4 | 7.4e-3 / 6.6e-3 / 9.5e-3
  3x16, the row closest to the emulation 8.7e-9 / 7.3e-8 / 2.3e-7 | 1.8e-4 / 2.6e-5 / 8.8e-5 | 5.7e-3 / 1.7e-3 / 2.7e-3
  value 3x50 .. 3x400, pred/sums/grad <= 1.6e-4 / 3.0e-5 / 8.9e-5 | <= 1.1e-3 / 2.5e-4 / 2.3e-4 | >= 5.3e-3 / 7.5e-4 / 2.1e-3
No kernel was changed.

The constrained twins of the 8-wave rows (hard wall conditions) are judged the same way at the
end of the module: 3x50, 3x256 at 128 and 64 columns, 3x400 wide on either spill and four value rows; measured figures
in DESIGN.md 7.10, "Tests".
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import autograd_ref as ar
from oracle import bf16x3_emul as em
from oracle import fwdmode_ref as fr

from test_tile_loops import BARS, _net, _rel_l2
from test_kernel_pairings import CODE as _CODE, F32, ROWS_256, ROWS_400, X3, _row
from test_residual_term import (N, SHARE_MIN, _TILE_LOOPS_ROWS, _WSPLIT_ROWS, _block_errs, _case, _inputs, _key, _nets,
                                _oracle, _plain, _shares)
from test_value_loops import value_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import plan_census  # noqa: E402

B16 = "bf16"
CODE = dict(_CODE, bf16=2)
FACTOR = 4.0              # bar = FACTOR * noise; FACTOR * bar <= format is the condition on the inputs
CONTROL = 1.5             # a wrong term count or rounding mode moves its quantity past CONTROL * bar
N_B = 150                 # boundary points of the value rows
ALPHA_B = 10.0
QS = ("eq", "sums", "grad", "gradw")
VQS = ("pred", "sums", "grad")
VARIANTS = [dict(acc=a, tanh=t, layer0=z) for z in ("fma", "plain") for t in ("fast", "libm")
            for a in ("fp32", "fp64", "k16")]


def _twin(row):
    """A row of the bf16x3 tables with every bf16x3 member replaced by plain bf16: same names, tile and switches."""
    assert X3 in row["triple"]
    return _row(row["prec"].replace(X3, B16), row["names"], row["tile"], row["env"])


SPLIT = ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
WSPLIT = ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")
# code 2 in one role only, beside bf16x3 (terms_of per role; forward and reverse differ, so the pair is not fused)
MIXED_256 = [_row("bf16,bf16x3,bf16x3", SPLIT, 32), _row("bf16x3,bf16,bf16x3", SPLIT, 32),
             _row("bf16x3,bf16x3,bf16", SPLIT, 32)]
MIXED_400 = [_row("bf16,bf16x3,bf16x3", WSPLIT, 16), _row("bf16x3,bf16,bf16x3", WSPLIT, 16),
             _row("bf16x3,bf16x3,bf16", WSPLIT, 16)]
# ... and beside fp32: the twins of the fp32 / bf16x3 rows, "fp32,fp32,bf16" among them at either width
TWINS_256 = [_twin(r) for r in _TILE_LOOPS_ROWS[:2] + ROWS_256 if X3 in r["triple"]]
TWINS_400 = [_twin(r) for r in _WSPLIT_ROWS + ROWS_400 if X3 in r["triple"]]
# (L, H, net seed, points seed).  The seeds meet the conditions below.  Three hidden layers, but two at hidden 512: at
# depth 3 its gradient noise (1.1e-4 .. 1.4e-4 on 60 seeds) leaves a three-term dW role, 3e-4 away, inside 4 * noise.
NET_256 = (3, 256, 1236, 11)
NET_400 = (3, 400, 44, 13)
NARROW = [(3, 16, 74, 15), (3, 50, 58, 15), (3, 96, 61, 15), (3, 128, 65, 15), (3, 200, 58, 15)]
WIDE = [(3, 288, 77, 17), (3, 330, 76, 17), (3, 448, 82, 17), (2, 512, 75, 17)]
CASES_256 = [_case(*NET_256, r) for r in TWINS_256 + MIXED_256]
CASES_400 = [_case(*NET_400, r) for r in TWINS_400 + MIXED_400]
CASES_WIDTHS = [_case(L, H, seed, pts, _twin(_plain(H, X3))) for L, H, seed, pts in NARROW + WIDE]
CASES = CASES_256 + CASES_400 + CASES_WIDTHS
# value mode: the boundary plan, all three roles in plain bf16 (L, H, net seed; seeds chosen as above)
VALUE = [(3, 50, 51), (3, 128, 50), (3, 256, 52), (3, 400, 52)]
_ids = lambda cases: [c["tag"] for c in cases]


# --------------------------------------------------------------------------------------------------------------------
# the emulation of a row: its options from the kernel names, its variants, noise, format and bar
# --------------------------------------------------------------------------------------------------------------------
def _emul_options(names):
    """spill / spill0 / out of oracle.bf16x3_emul for the residual kernels a census row names (csrc/spill.h's table:
    the role-split sweeps only exist on their 24-bit layouts, the three wide bf16 kernels meet only in an all-bf16
    plan, which is SPILL_P24_WIDE; everything else spills fp32 planes)."""
    fwd, bwd, dw = names
    image = "image" if fwd in ("fwd_bf16_kernel", "fwd_bf16_wide_kernel") else "fp32"
    if fwd == "fwd_split_kernel":
        assert (bwd, dw) == SPLIT[1:]
        return dict(spill="p24", spill0="none", out=image)
    if fwd == "fwd_wsplit_kernel":
        assert (bwd, dw) == WSPLIT[1:]
        return dict(spill="p24", spill0="dw", out=image)
    if names == ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel"):
        return dict(spill="p24", spill0="all", out=image)
    return dict(spill="f32", spill0="none", out=image)


def _default(triple):
    return dict(acc="fp32", tanh="libm" if triple[0] == F32 else "fast", layer0="fma")


_EMUL = {}


def _emul(c, triple=None, fault=None, **variant):
    """The emulation of a case's net at a precision triple (default: the row's) in one variant (default: the row's
    emulation), once per process."""
    row = c["row"]
    triple = row["triple"] if triple is None else triple
    opts = dict(_emul_options(row["names"]), **(variant or _default(row["triple"])))
    k = _key(c) + (triple, fault) + tuple(sorted(opts.items()))
    if k not in _EMUL:
        inp = _inputs(c)
        _EMUL[k] = em.residual_loss_and_grad(inp["flat"], inp["x"], inp["y"], c["Re"], c["L"], c["H"], prec=triple,
                                             fault=fault, **opts)
    return _EMUL[k]


def _dist(c, a, b, ref=None):
    """Distances of two results of a case in units of the oracle's norms (ref: another reference's), and the gradient's
    per block."""
    ref = _oracle(c) if ref is None else ref
    blocks = _block_errs(a["grad"], b["grad"], 3, c["L"], c["H"], ref=ref["grad"])
    d = dict(eq=max(float(np.linalg.norm(a["eqs"][k] - b["eqs"][k]) / np.linalg.norm(ref["eqs"][k])) for k in range(3)),
             sums=max(abs(a["sums"][k] - b["sums"][k]) / ref["sums"][k] for k in range(3)), grad=max(blocks),
             gradw=max(blocks[2 * l] for l in range(1, c["L"])))
    return d, blocks


def _noise(c):
    runs = [_emul(c, **v) for v in VARIANTS]
    ds = [_dist(c, a, b)[0] for i, a in enumerate(runs) for b in runs[:i]]
    return {q: max(d[q] for d in ds) for q in QS}


def _format(c):
    return _dist(c, _emul(c), _oracle(c))[0]


def _judged(c):
    """The quantities held to the emulation at 4 * noise: those that pass through a bf16 operand split, where two
    correct implementations differ by flipped roundings.  Behind an fp32 forward sweep eq and sums do not: there the
    kernel's contractions and libm enter directly at the size of the variants' spread, for which the factor has no
    footing - they keep the fp32 bars against the oracle."""
    return QS if c["row"]["triple"][0] != F32 else ("grad", "gradw")


def _conditioned(c):
    """The quantities a PLAIN-bf16 role feeds, where 4 * noise <= format / 4 is asked of the inputs."""
    return QS if c["row"]["triple"][0] == B16 else ("grad", "gradw")


def _bars(c):
    noise = _noise(c)
    return {q: FACTOR * noise[q] for q in QS}


def _rows_of_nets(cases):
    """One case per distinct net x precision triple x emulation options: the rows that share a noise measurement."""
    seen = {}
    for c in cases:
        seen.setdefault(_key(c) + (c["row"]["triple"],) + tuple(sorted(_emul_options(c["row"]["names"]).items())), c)
    return list(seen.values())


# --------------------------------------------------------------------------------------------------------------------
# CPU: the table
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def test_the_table_is_what_the_module_says():
    x3_rows = [r for r in _TILE_LOOPS_ROWS + ROWS_256 + _WSPLIT_ROWS + ROWS_400 if X3 in r["triple"]]
    assert len(x3_rows) == 2 + 11 + 2 + 4 == len(TWINS_256) + len(TWINS_400)
    for r, t in zip(x3_rows, TWINS_256 + TWINS_400):
        assert (t["names"], t["env"], t["tile"]) == (r["names"], r["env"], r["tile"])
        assert t["triple"] == tuple(B16 if p == X3 else p for p in r["triple"]) and X3 not in t["triple"]
    # every forward / reverse / dW kernel name of the bf16 families runs in plain bf16
    names = {c["row"]["names"][k] for c in CASES for k in range(3) if c["row"]["triple"][k] == B16}
    assert names == {"fwd_%s_kernel" % f for f in ("split", "pipe", "bf16", "wsplit", "bf16_wide")} | \
        {"bwd_%s_kernel" % f for f in ("split", "pipe", "bf16", "wsplit", "bf16_wide")} | \
        {"dw_bf16_kernel", "dw_bf16_wide_kernel"}
    # code 2 in one role only, beside bf16x3 and beside fp32
    triples = {c["row"]["triple"] for c in CASES}
    for t in ((B16, X3, X3), (X3, B16, X3), (X3, X3, B16), (F32, F32, B16)):
        assert t in triples
    assert {c["H"] for c in CASES_WIDTHS} == {16, 50, 96, 128, 200, 288, 330, 448, 512}
    assert all(c["L"] == (2 if c["H"] == 512 else 3) and c["Re"] == 1.0 for c in CASES)
    assert len({c["tag"] for c in CASES}) == len(CASES)
    assert (-(-N // 32), N % 32, -(-N // 16), N % 16) == (3, 5, 5, 5)
    # value tiles: two of 128 with the second ragged (three of 64 on the wide kernels)
    assert [-(-N_B // value_tile(H, False)) for _, H, _ in VALUE] == [2, 2, 2, 3] and N_B % 128 == 22 == N_B % 64


@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_every_row_resolves_to_the_names_it_lists(lib, c):
    row = c["row"]
    got = plan_census.run_case(lib, (c["H"], c["L"], tuple(CODE[p] for p in row["triple"]), 4, N, dict(row["env"])))
    assert got[1] == 0, got
    assert tuple(got[5:8]) == row["names"]
    assert got[2] == -(-N // row["tile"]) * row["tile"]
    # the spill the emulation is told is the census row's: what its kernel names admit by csrc/spill.h.  The 24-bit
    # layouts need all three roles in a bf16 mode and neither an 8-wave narrow nor a pipelined sweep.
    opts = _emul_options(tuple(got[5:8]))
    narrow8 = {"fwd_pipe_kernel", "fwd_bf16_kernel", "bwd_pipe_kernel", "bwd_bf16_kernel"}
    assert (opts["spill"] == "f32") == (F32 in row["triple"] or bool(narrow8 & set(row["names"])))


def _value_names(H):
    wide = "_wide" if (H + 31) // 32 * 32 > 256 else ""
    return tuple(k + "_bf16" + wide + "_kernel" for k in ("fwd", "bwd", "dw"))


@pytest.mark.parametrize("L,H,seed", VALUE, ids=["%dx%d" % v[:2] for v in VALUE])
def test_every_value_row_resolves_to_the_names_it_lists(lib, L, H, seed):
    got = plan_census.run_case(lib, (H, L, (2, 2, 2), 1, N_B, {}))
    assert got[1] == 0, got
    tile = value_tile(H, False)
    assert tuple(got[5:8]) == _value_names(H) and got[2] == -(-N_B // tile) * tile


# --------------------------------------------------------------------------------------------------------------------
# CPU: the conditions on the inputs
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _nets(CASES), ids=_ids(_nets(CASES)))
def test_the_viscous_term_carries_its_share(c):
    s = _shares(c)
    assert min(s.values()) >= SHARE_MIN, s


_NOISE_ROWS = _rows_of_nets(CASES)


@pytest.mark.parametrize("c", _NOISE_ROWS, ids=_ids(_NOISE_ROWS))
def test_the_bar_is_four_times_sharper_than_the_format_error(c):
    """A condition on the inputs, not a measurement: a row that does not meet it gets another seed or depth."""
    noise, fmt = _noise(c), _format(c)
    print("[bf16 mode] %s noise %s | format %s | bar / format %s" % (
        c["tag"], " ".join("%s %.1e" % (q, noise[q]) for q in QS), " ".join("%s %.1e" % (q, fmt[q]) for q in QS),
        " ".join("%s %.3f" % (q, FACTOR * noise[q] / fmt[q]) for q in QS)))
    for q in _conditioned(c):
        assert noise[q] > 0.0 and FACTOR * FACTOR * noise[q] <= fmt[q], (q, noise[q], fmt[q])


# --------------------------------------------------------------------------------------------------------------------
# CPU: the sensitivity controls, on the emulation
# --------------------------------------------------------------------------------------------------------------------
def _plain_row_of_net(c):
    """The all-bf16 row of a case's net that the controls run on."""
    return next(k for k in CASES if _key(k) == _key(c) and k["row"]["triple"] == (B16,) * 3)


_CONTROL_NETS = [_plain_row_of_net(c) for c in _nets(CASES)]


@pytest.mark.parametrize("c", _CONTROL_NETS, ids=_ids(_CONTROL_NETS))
def test_controls_a_wrong_term_count_or_rounding_leaves_the_bar(c):
    """What a correct kernel must not do, done to the emulation: a role run with three terms, operands truncated."""
    bar, base = _bars(c), _emul(c)
    L, H = c["L"], c["H"]
    fwd3, _ = _dist(c, _emul(c, (X3, B16, B16)), base)
    bwd3, _ = _dist(c, _emul(c, (B16, X3, B16)), base)
    _, dw3 = _dist(c, _emul(c, (B16, B16, X3)), base)
    trunc, _ = _dist(c, _emul(c, fault="trunc"), base)
    hidden_w = max(dw3[2 * l] for l in range(1, L))          # the weight blocks of layers 1 .. L - 1
    moved = dict(fwd3=max(fwd3["eq"] / bar["eq"], fwd3["sums"] / bar["sums"]), bwd3=bwd3["grad"] / bar["grad"],
                 dw3=hidden_w / bar["gradw"], trunc=trunc["eq"] / bar["eq"])
    print("[bf16 mode] %dx%d controls, distance / bar: %s" % (L, H, " ".join("%s %.1f" % kv for kv in moved.items())))
    assert min(moved.values()) > CONTROL, moved
    # and the dW role's other blocks do not move at all: the control is the dW GEMM's alone
    assert max(dw3[k] for k in range(len(dw3)) if k not in [2 * l for l in range(1, L)]) == 0.0


_IMAGE_ROWS = [c for c in _NOISE_ROWS
               if c["row"]["triple"] == (B16,) * 3 and _emul_options(c["row"]["names"])["out"] == "image"]


@pytest.mark.parametrize("c", _IMAGE_ROWS, ids=_ids(_IMAGE_ROWS))
def test_control_the_bar_sees_what_the_output_layer_reads(c):
    """The 8-wave sweeps' output layer takes the last a-streams from the bf16 operand image; an emulation that feeds it
    the fp32 streams, as the other sweeps do, is outside the planes' bar: the rows tell the two apart."""
    inp, opts = _inputs(c), dict(_emul_options(c["row"]["names"]), out="fp32", **_default(c["row"]["triple"]))
    other = em.residual_loss_and_grad(inp["flat"], inp["x"], inp["y"], c["Re"], c["L"], c["H"], prec=c["row"]["triple"],
                                      **opts)
    d, _ = _dist(c, other, _emul(c))
    assert d["eq"] > CONTROL * _bars(c)["eq"], (d["eq"], _bars(c)["eq"])


def test_control_the_five_percent_bar_passes_both_faults():
    """Why this module exists.  On the inputs of test_bf16_fast_mode_runs_and_is_close (6x256 seed 9, Re 2000, 640
    points, every 16th boundary point, alpha_b 10), a forward role that runs three terms and a Laplacian stream scaled
    by 1 % both stay inside that test's 5 % of fp32, for the loss and for the whole gradient."""
    L, H, n, Re = 6, 256, 640, 2000.0
    flat = _net(L, H, 9)
    rng = np.random.RandomState(1)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())

    def run(prec, fault=None):
        r = em.residual_loss_and_grad(flat, x, y, Re, L, H, prec=prec, spill="p24" if prec != F32 else "f32",
                                      tanh="libm" if prec == F32 else "fast", fault=fault)
        b = em.value_loss_and_grad(flat, xb, yb, ub, vb, L, H, coef=2.0 * ALPHA_B / xb.size,
                                   prec=prec if isinstance(prec, str) else B16)
        return sum(r["sums"]) / n + ALPHA_B * sum(b["sums"]) / xb.size, r["grad"] + b["grad"]

    loss32, grad32 = run(F32)
    for tag, got in (("bf16", run(B16)), ("forward with three terms", run((X3, B16, B16))),
                     ("Laplacian stream * 1.01", run(B16, fault=("stream", 3, 1.01)))):
        dl, dg = abs(got[0] - loss32) / loss32, _rel_l2(got[1], grad32)
        print("[bf16 mode] 6x256 seed 9 Re 2000, %s against fp32: loss %.2e gradient %.2e" % (tag, dl, dg))
        assert dl < 5e-2 and dg < 5e-2, (tag, dl, dg)


# --------------------------------------------------------------------------------------------------------------------
# value mode: the boundary plan
# --------------------------------------------------------------------------------------------------------------------
def _boundary():
    idx = np.round(np.linspace(0, 2051, N_B)).astype(int)
    return tuple(a.reshape(-1)[idx].astype(np.float32) for a in ar.cavity_boundary())


_VALUE = {}


def _value(L, H, seed, what, **variant):
    """'oracle': bc_loss_and_grad in fp64; 'emul': the one-stream emulation in plain bf16, in one variant."""
    k = (L, H, seed, what) + tuple(sorted(variant.items()))
    if k not in _VALUE:
        flat, (xb, yb, ub, vb) = _net(L, H, seed), _boundary()
        if what == "oracle":
            P = fr.unflatten(flat.astype(np.float64), 2, 3, L, H)
            _VALUE[k] = fr.bc_loss_and_grad(P, xb.astype(np.float64), yb.astype(np.float64), ub, vb, alpha_b=ALPHA_B)
        else:
            _VALUE[k] = em.value_loss_and_grad(flat, xb, yb, ub, vb, L, H, coef=2.0 * ALPHA_B / N_B, prec=B16,
                                               **(variant or _default((B16,) * 3)))
    return _VALUE[k]


def _value_dist(L, H, seed, a, b):
    ref = _value(L, H, seed, "oracle")
    return dict(pred=max(float(np.linalg.norm(a["pred"][:, k] - b["pred"][:, k]) / np.linalg.norm(ref["pred"][:, k]))
                         for k in range(3)),
                sums=max(abs(a["sums"][k] - b["sums"][k]) / ref["sums"][k] for k in range(2)),
                grad=max(_block_errs(a["grad"], b["grad"], 3, L, H, ref=ref["grad"])))


def _value_noise(L, H, seed):
    runs = [_value(L, H, seed, "emul", **v) for v in VARIANTS]
    ds = [_value_dist(L, H, seed, a, b) for i, a in enumerate(runs) for b in runs[:i]]
    return {q: max(d[q] for d in ds) for q in VQS}


def _value_format(L, H, seed):
    return _value_dist(L, H, seed, _value(L, H, seed, "emul"), _value(L, H, seed, "oracle"))


@pytest.mark.parametrize("L,H,seed", VALUE, ids=["%dx%d" % v[:2] for v in VALUE])
def test_the_value_bar_is_four_times_sharper_than_the_format_error(L, H, seed):
    noise, fmt = _value_noise(L, H, seed), _value_format(L, H, seed)
    print("[bf16 mode] value %dx%d noise %s | format %s | bar / format %s" % (
        L, H, " ".join("%s %.1e" % (q, noise[q]) for q in VQS), " ".join("%s %.1e" % (q, fmt[q]) for q in VQS),
        " ".join("%s %.3f" % (q, FACTOR * noise[q] / fmt[q]) for q in VQS)))
    for q in VQS:
        assert noise[q] > 0.0 and FACTOR * FACTOR * noise[q] <= fmt[q], (q, noise[q], fmt[q])


# --------------------------------------------------------------------------------------------------------------------
# GPU: one engine and one loss_and_grad per row, against the row's emulation at the row's bar
# --------------------------------------------------------------------------------------------------------------------
def _engine(monkeypatch, L, H, Re, prec, env, flat, x, y, bc, constrain=False, sup=None):
    """constrain: hard wall conditions on; sup: a supervised set (x, y, u, v) at alpha_s = ALPHA_B."""
    from nsfnet_amd import engine as eng
    for k in list(os.environ):
        if k.startswith("PINN_") or k == "NSFNET_CHUNK_POINTS":
            monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    E = eng.PinnEngine(torch.device("cuda:0"), L, H, Re, alpha_b=ALPHA_B, alpha_e=1.0, precision=prec,
                       alpha_s=0.0 if sup is None else ALPHA_B)
    if constrain:
        E.set_hard_boundary(True)
    E.net.set_flat(torch.tensor(flat))
    E.set_collocation(x, y)
    E.set_boundary(*bc)
    if sup is not None:
        E.set_supervised(*sup)
    return eng, E


def _alone(eng, E, plan):
    """The gradient of one plan alone (loss_and_grad's own assembly has added the other's)."""
    g = torch.full((E.net.num_params,), float("nan"), dtype=torch.float32, device=torch.device("cuda:0"))
    eng.grad_reduce(E.net, [plan], g)
    torch.cuda.synchronize()
    g = g.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_plain_bf16_kernels_vs_their_arithmetic(monkeypatch, c):
    row, inp = c["row"], _inputs(c)
    eng, E = _engine(monkeypatch, c["L"], c["H"], c["Re"], row["prec"], row["env"], inp["flat"], inp["x"], inp["y"],
                     _boundary())
    assert E.plan_f.kernel_names() == row["names"]
    assert E.plan_f.npad == -(-N // row["tile"]) * row["tile"]
    E.loss_and_grad()
    got = dict(grad=_alone(eng, E, E.plan_f), sums=list(E.sums.cpu().numpy().astype(np.float64)[:3]),
               eqs=[E.plan_f.field(k).cpu().numpy().astype(np.float64) for k in ("eq1", "eq2", "eq3")])
    del E
    torch.cuda.empty_cache()
    ref, emu, bar, fmt = _oracle(c), _emul(c), _bars(c), _format(c)
    d, blocks = _dist(c, got, emu)
    far, _ = _dist(c, got, ref)
    mx = max(float(np.abs(got["eqs"][k] - emu["eqs"][k]).max() / np.abs(ref["eqs"][k]).max()) for k in range(3))
    print("[bf16 mode] %s: from the emulation %s (planes max-abs %.1e) | bar %s | format %s | from the oracle %s" % (
        c["tag"], " ".join("%s %.2e" % (q, d[q]) for q in QS), mx, " ".join("%.1e" % bar[q] for q in QS),
        " ".join("%.1e" % fmt[q] for q in QS), " ".join("%.1e" % far[q] for q in QS)))
    for q in _judged(c):
        assert d[q] <= bar[q], (q, d[q], bar[q], blocks if q == "grad" else None)
    if F32 == row["triple"][0]:
        # an fp32 forward sweep: its planes and sums keep the fp32 bars against the oracle (test_residual_term's rule)
        for k in range(3):
            assert np.abs(got["eqs"][k] - ref["eqs"][k]).max() <= BARS[F32]["eq"] * np.abs(ref["eqs"][k]).max(), k
        assert far["sums"] <= BARS[F32]["sums"]
    if B16 == row["triple"][0]:
        # the forward role really ran one term: it is as far from the oracle as one term is (triangle inequality)
        for q in ("eq", "sums"):
            assert far[q] >= fmt[q] - bar[q], (q, far[q], fmt[q], bar[q])


@pytest.mark.gpu
@pytest.mark.parametrize("L,H,seed", VALUE, ids=["%dx%d" % v[:2] for v in VALUE])
def test_plain_bf16_value_kernels_vs_their_arithmetic(monkeypatch, L, H, seed):
    rng = np.random.RandomState(5)
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    eng, E = _engine(monkeypatch, L, H, 1.0, B16, (), _net(L, H, seed), x, y, _boundary())
    tile = value_tile(H, False)
    assert E.plan_b.kernel_names() == _value_names(H) and E.plan_b.npad == -(-N_B // tile) * tile
    E.loss_and_grad()
    got = dict(grad=_alone(eng, E, E.plan_b), sums=list(E.sums.cpu().numpy().astype(np.float64)[8:10]),
               pred=E.plan_b.pred.cpu().numpy().astype(np.float64).T[:N_B])
    del E
    torch.cuda.empty_cache()
    noise, fmt = _value_noise(L, H, seed), _value_format(L, H, seed)
    d = _value_dist(L, H, seed, got, _value(L, H, seed, "emul"))
    far = _value_dist(L, H, seed, got, _value(L, H, seed, "oracle"))
    print("[bf16 mode] value %dx%d: from the emulation %s | bar %s | format %s | from the oracle %s" % (
        L, H, " ".join("%s %.2e" % (q, d[q]) for q in VQS), " ".join("%.1e" % (FACTOR * noise[q]) for q in VQS),
        " ".join("%.1e" % fmt[q] for q in VQS), " ".join("%.1e" % far[q] for q in VQS)))
    for q in VQS:
        assert d[q] <= FACTOR * noise[q], (q, d[q], FACTOR * noise[q])
    for q in ("pred", "sums"):
        assert far[q] >= fmt[q] - FACTOR * noise[q], (q, far[q], fmt[q])


# --------------------------------------------------------------------------------------------------------------------
# the constrained twins of the 8-wave rows (hard wall conditions)
# --------------------------------------------------------------------------------------------------------------------
# Every TERMS == 1 instantiation of the constrained point stages (half of fwd_bf16's and fwd_bf16_wide's, and the
# reverse ones), by the method above: the emulation takes the map u = g + D N_u, v = D N_v as a pair of fp32 callables
# (oracle.bf16x3_emul's point_map; the closed forms of tests/hardbc_model.py at float32), the norms are the fp64
# model's (hardbc_model.constrained_fwdmode / constrained_value), bar = FACTOR * noise among the emulation's own
# variants, condition 4 * noise <= format / 4.  A constrained plan runs the 8-wave families whatever the switches say,
# so the rows are the 8-wave ones: 3x50, 3x256 at 128 and 64 columns, 3x400 wide on either spill, and the value rows -
# on interior points through the supervised plan, since the boundary plan's gradient is zero under the constraint.
import hardbc_model as hm  # noqa: E402

HBC = hm.HardBc()
_EIGHT = {("fwd_bf16_kernel", "bwd_bf16_kernel"), ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel")}
# (L, H, net seed, points seed): the next seeds after NARROW's 3x50, NET_256's and NET_400's at which the conditions hold
# constrained (the viscous share, 4 * noise <= format / 4, noise of the planes >= 3e-5 and of the gradient >= 1e-5)
HBC_NETS = {50: (3, 50, 59, 15), 256: (3, 256, 1238, 11), 400: (3, 400, 45, 13)}
CASES_HBC = [_case(*HBC_NETS[c["H"]], c["row"]) for c in CASES
             if c["H"] in HBC_NETS and c["row"]["names"][:2] in _EIGHT and c["row"]["triple"][:2] == (B16, B16)]
# (L, H, net seed): the first seeds from VALUE's on that meet the condition with a noise well above fp32 rounding (pred
# >= 3e-5, sums >= 4e-6, gradient >= 1e-5: where no variant flips a bf16 rounding the bar would collapse to it)
VALUE_HBC = [(3, 50, 55), (3, 128, 53), (3, 256, 53), (3, 400, 55)]


def _residual_map(x, y):
    h = hm.point_factors(HBC, x, y, dtype=np.float32)

    def apply(f, kw):
        def run(q):
            q = np.array(q, dtype=np.float32)
            for ch, lift in ((0, True), (1, False)):
                q[:, ch, :] = np.stack(f(h, *(q[:, ch, k] for k in range(4)), **kw(lift)), axis=1)
            return q
        return run
    return apply(hm.transform_streams, lambda lift: dict(lift=lift)), apply(hm.transpose_streams, lambda lift: {})


def _value_map(x, y):
    h = hm.point_factors(HBC, x, y, dtype=np.float32)

    def forward(pred):
        pred = np.array(pred, dtype=np.float32)
        pred[:, 0], pred[:, 1] = h["g"] + h["D"] * pred[:, 0], h["D"] * pred[:, 1]
        return pred

    def transpose(adj):
        adj = np.array(adj, dtype=np.float32)
        adj[:, 0], adj[:, 1] = adj[:, 0] * h["D"], adj[:, 1] * h["D"]
        return adj
    return forward, transpose


_HBC = {}


def _hbc_model(c, Re=None):
    k = _key(c) + ("model", Re)
    if k not in _HBC:
        inp = _inputs(c)
        P = fr.unflatten(inp["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
        _HBC[k] = hm.constrained_fwdmode(P, HBC, inp["x"], inp["y"], c["Re"] if Re is None else Re)
    return _HBC[k]


def _hbc_emul(c, triple=None, **variant):
    row = c["row"]
    triple = row["triple"] if triple is None else triple
    opts = dict(_emul_options(row["names"]), **(variant or _default(row["triple"])))
    k = _key(c) + (triple,) + tuple(sorted(opts.items()))
    if k not in _HBC:
        inp = _inputs(c)
        _HBC[k] = em.residual_loss_and_grad(inp["flat"], inp["x"], inp["y"], c["Re"], c["L"], c["H"], prec=triple,
                                            point_map=_residual_map(inp["x"], inp["y"]), **opts)
    return _HBC[k]


def _hbc_noise(c):
    runs = [_hbc_emul(c, **v) for v in VARIANTS]
    ds = [_dist(c, a, b, _hbc_model(c))[0] for i, a in enumerate(runs) for b in runs[:i]]
    return {q: max(d[q] for d in ds) for q in QS}


def _hbc_format(c):
    return _dist(c, _hbc_emul(c), _hbc_model(c), _hbc_model(c))[0]


def test_the_constrained_table_is_what_the_module_says():
    assert sorted((c["H"], c["row"]["triple"], c["row"]["env"]) for c in CASES_HBC) == sorted([
        (50, (B16,) * 3, ()), (256, (B16,) * 3, (("PINN_SCHED", "0"),)), (256, (B16,) * 3, (("PINN_TILE_COLS", "64"),)),
        (400, (B16,) * 3, (("PINN_WSPLIT", "0"),)), (400, (B16, B16, F32), ())])
    assert {_emul_options(c["row"]["names"])["spill"] for c in CASES_HBC if c["H"] == 400} == {"p24", "f32"}
    assert all(_emul_options(c["row"]["names"])["out"] == "image" for c in CASES_HBC)


@pytest.mark.parametrize("c", CASES_HBC, ids=_ids(CASES_HBC))
def test_every_constrained_row_resolves_to_the_names_it_lists(lib, c):
    from test_hardbc_terms import _constrained_census
    row = c["row"]
    got = _constrained_census(lib, (c["H"], c["L"], tuple(CODE[p] for p in row["triple"]), 4, N, dict(row["env"])),
                              HBC.struct())
    assert got[1] == 0, got
    assert tuple(got[5:8]) == row["names"] and got[2] == -(-N // row["tile"]) * row["tile"]
    # ... with the workspace, hence the spill, of the unconstrained row
    plain = plan_census.run_case(lib, (c["H"], c["L"], tuple(CODE[p] for p in row["triple"]), 4, N,
                                       dict(row["env"], PINN_SCHED="0", PINN_WSPLIT="0", PINN_FUSE="0")))
    assert got[1:] == plain[1:], (got, plain)


def test_the_emulations_point_map_is_the_fp64_models_map():
    """With fp32 products in every role the mapped emulation is the fp64 constrained model to fp32 rounding."""
    c = CASES_HBC[0]
    inp, ref = _inputs(c), _hbc_model(c)
    got = em.residual_loss_and_grad(inp["flat"], inp["x"], inp["y"], c["Re"], c["L"], c["H"], prec=F32, spill="f32",
                                    point_map=_residual_map(inp["x"], inp["y"]))
    d, _ = _dist(c, got, ref, ref)
    assert max(d.values()) <= 1e-5, d
    plain = em.residual_loss_and_grad(inp["flat"], inp["x"], inp["y"], c["Re"], c["L"], c["H"], prec=F32, spill="f32")
    assert _dist(c, plain, ref, ref)[0]["eq"] > 0.1       # and the map is not a no-op


@pytest.mark.parametrize("c", _nets(CASES_HBC), ids=_ids(_nets(CASES_HBC)))
def test_the_viscous_term_carries_its_share_constrained(c):
    r, r0 = _hbc_model(c), _hbc_model(c, 1.0e30)
    rel_max = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    s = dict(eq1=rel_max(r0["eqs"][0], r["eqs"][0]), eq2=rel_max(r0["eqs"][1], r["eqs"][1]), grad=_rel_l2(r0["grad"], r["grad"]))
    assert min(s.values()) >= SHARE_MIN, s


_NOISE_HBC = _rows_of_nets(CASES_HBC)


@pytest.mark.parametrize("c", _NOISE_HBC, ids=_ids(_NOISE_HBC))
def test_the_constrained_bar_is_four_times_sharper_than_the_format_error(c):
    """A condition on the inputs, not a measurement: a row that does not meet it gets another seed."""
    noise, fmt = _hbc_noise(c), _hbc_format(c)
    print("[bf16 mode] constrained %s noise %s | format %s | bar / format %s" % (
        c["tag"], " ".join("%s %.1e" % (q, noise[q]) for q in QS), " ".join("%s %.1e" % (q, fmt[q]) for q in QS),
        " ".join("%s %.3f" % (q, FACTOR * noise[q] / fmt[q]) for q in QS)))
    for q in _conditioned(c):
        assert noise[q] > 0.0 and FACTOR * FACTOR * noise[q] <= fmt[q], (q, noise[q], fmt[q])


def _supervised():
    """150 interior points with targets that satisfy the wall conditions themselves, as a measured flow field would:
    u = g + D a, v = D b with smooth a, b the net does not match, plus noise (test_value_loops' fields)."""
    rng = np.random.RandomState(23)
    x, y = (0.02 + 0.96 * rng.rand(N_B)).astype(np.float32), (0.02 + 0.96 * rng.rand(N_B)).astype(np.float32)
    h = hm.point_factors(HBC, x.astype(np.float64), y.astype(np.float64))
    a = 0.25 + np.sin(2 * np.pi * x) * np.cos(np.pi * y) + 0.05 * rng.randn(N_B)
    b = -0.2 + np.cos(3.0 * x) * np.sin(2 * np.pi * y) + 0.05 * rng.randn(N_B)
    return x, y, (h["g"] + h["D"] * a).astype(np.float32), (h["D"] * b).astype(np.float32)


def _hbc_value(L, H, seed, what, **variant):
    k = (L, H, seed, "value", what) + tuple(sorted(variant.items()))
    if k not in _HBC:
        flat, (x, y, u, v) = _net(L, H, seed), _supervised()
        if what == "model":
            P = fr.unflatten(flat.astype(np.float64), 2, 3, L, H)
            c = 2.0 * ALPHA_B / N_B
            r = hm.constrained_value(P, HBC, x, y, targets=[u, v, None], coef=(c, c, 0.0))
            _HBC[k] = dict(r, sums=r["sums"][:2])
        else:
            _HBC[k] = em.value_loss_and_grad(flat, x, y, u, v, L, H, coef=2.0 * ALPHA_B / N_B, prec=B16,
                                             point_map=_value_map(x, y), **(variant or _default((B16,) * 3)))
    return _HBC[k]


def _hbc_value_dist(L, H, seed, a, b):
    ref = _hbc_value(L, H, seed, "model")
    return dict(pred=max(float(np.linalg.norm(a["pred"][:, k] - b["pred"][:, k]) / np.linalg.norm(ref["pred"][:, k]))
                         for k in range(3)),
                sums=max(abs(a["sums"][k] - b["sums"][k]) / ref["sums"][k] for k in range(2)),
                grad=max(_block_errs(a["grad"], b["grad"], 3, L, H, ref=ref["grad"])))


def _hbc_value_noise(L, H, seed):
    runs = [_hbc_value(L, H, seed, "emul", **v) for v in VARIANTS]
    ds = [_hbc_value_dist(L, H, seed, a, b) for i, a in enumerate(runs) for b in runs[:i]]
    return {q: max(d[q] for d in ds) for q in VQS}


def _hbc_value_format(L, H, seed):
    return _hbc_value_dist(L, H, seed, _hbc_value(L, H, seed, "emul"), _hbc_value(L, H, seed, "model"))


@pytest.mark.parametrize("L,H,seed", VALUE_HBC, ids=["%dx%d" % v[:2] for v in VALUE_HBC])
def test_the_constrained_value_bar_is_four_times_sharper_than_the_format_error(L, H, seed):
    noise, fmt = _hbc_value_noise(L, H, seed), _hbc_value_format(L, H, seed)
    print("[bf16 mode] constrained value %dx%d noise %s | format %s | bar / format %s" % (
        L, H, " ".join("%s %.1e" % (q, noise[q]) for q in VQS), " ".join("%s %.1e" % (q, fmt[q]) for q in VQS),
        " ".join("%s %.3f" % (q, FACTOR * noise[q] / fmt[q]) for q in VQS)))
    for q in VQS:
        assert noise[q] > 0.0 and FACTOR * FACTOR * noise[q] <= fmt[q], (q, noise[q], fmt[q])


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES_HBC, ids=_ids(CASES_HBC))
def test_constrained_plain_bf16_kernels_vs_their_arithmetic(monkeypatch, c):
    row, inp = c["row"], _inputs(c)
    eng, E = _engine(monkeypatch, c["L"], c["H"], c["Re"], row["prec"], row["env"], inp["flat"], inp["x"], inp["y"],
                     _boundary(), constrain=True)
    assert E.plan_f.kernel_names() == row["names"] and E.plan_f.hard_bc() is not None
    assert E.plan_f.npad == -(-N // row["tile"]) * row["tile"]
    E.loss_and_grad()
    got = dict(grad=_alone(eng, E, E.plan_f), sums=list(E.sums.cpu().numpy().astype(np.float64)[:3]),
               eqs=[E.plan_f.field(k).cpu().numpy().astype(np.float64) for k in ("eq1", "eq2", "eq3")])
    del E
    torch.cuda.empty_cache()
    ref, emu, noise, fmt = _hbc_model(c), _hbc_emul(c), _hbc_noise(c), _hbc_format(c)
    bar = {q: FACTOR * noise[q] for q in QS}
    d, blocks = _dist(c, got, emu, ref)
    far, _ = _dist(c, got, ref, ref)
    print("[bf16 mode] constrained %s: from the emulation %s | bar %s | format %s | from the model %s" % (
        c["tag"], " ".join("%s %.2e" % (q, d[q]) for q in QS), " ".join("%.1e" % bar[q] for q in QS),
        " ".join("%.1e" % fmt[q] for q in QS), " ".join("%.1e" % far[q] for q in QS)))
    for q in QS:
        assert d[q] <= bar[q], (q, d[q], bar[q], blocks if q == "grad" else None)
    for q in ("eq", "sums"):        # the forward role really ran one term (triangle inequality)
        assert far[q] >= fmt[q] - bar[q], (q, far[q], fmt[q], bar[q])


@pytest.mark.gpu
@pytest.mark.parametrize("L,H,seed", VALUE_HBC, ids=["%dx%d" % v[:2] for v in VALUE_HBC])
def test_constrained_plain_bf16_value_kernels_vs_their_arithmetic(monkeypatch, L, H, seed):
    rng = np.random.RandomState(5)
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    eng, E = _engine(monkeypatch, L, H, 1.0, B16, (), _net(L, H, seed), x, y, _boundary(), constrain=True,
                     sup=_supervised())
    tile = value_tile(H, False)
    s = E.plan_s
    assert s.kernel_names() == _value_names(H) and s.npad == -(-N_B // tile) * tile and s.hard_bc() is not None
    E.loss_and_grad()
    got = dict(grad=_alone(eng, E, s), sums=list(E.sums.cpu().numpy().astype(np.float64)[16:18]),
               pred=s.pred.cpu().numpy().astype(np.float64).T[:N_B])
    del E, s
    torch.cuda.empty_cache()
    noise, fmt = _hbc_value_noise(L, H, seed), _hbc_value_format(L, H, seed)
    d = _hbc_value_dist(L, H, seed, got, _hbc_value(L, H, seed, "emul"))
    far = _hbc_value_dist(L, H, seed, got, _hbc_value(L, H, seed, "model"))
    print("[bf16 mode] constrained value %dx%d: from the emulation %s | bar %s | format %s | from the model %s" % (
        L, H, " ".join("%s %.2e" % (q, d[q]) for q in VQS), " ".join("%.1e" % (FACTOR * noise[q]) for q in VQS),
        " ".join("%.1e" % fmt[q] for q in VQS), " ".join("%.1e" % far[q] for q in VQS)))
    for q in VQS:
        assert d[q] <= FACTOR * noise[q], (q, d[q], FACTOR * noise[q])
    for q in ("pred", "sums"):
        assert far[q] >= fmt[q] - FACTOR * noise[q], (q, far[q], fmt[q])
