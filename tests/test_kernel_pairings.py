"""The kernel pairings of a plan, each run where its tile loops repeat, against the fp64 oracle.

pinn_plan_create pairs a forward sweep, a reverse sweep and a dW kernel from the three precisions and the schedule
switches.  The kernels of a plan meet only in the S / Z-bar spill of the workspace, so every pairing is a contract
between kernels of different files: the layout (csrc/spill.h: block size, first stored layer), the format (fp32 planes or
the 24-bit three-plane format) and whether layer 0 is spilled or recomputed by its readers.  tests/test_plan_census.py fingerprints
which kernels a plan names; it cannot tell whether they agree on what lies in the spill.  test_tile_loops.py runs three
pairings of the 6x256 net and two of the 4x400 net at looping point counts; this module runs the others a precision
triple or a switch selects - the pipelined sweeps, fp32 sweeps reading what bf16 sweeps spilled and the reverse, each
dW kernel behind either, the classic (fp32-plane) spill of the wide bf16 kernels, the 64-column bf16 and 128-column fp32
kernels at hidden 256 and the unfused role-split pair - on the same nets, points and oracle runs, with the same
comparison (test_tile_loops._compare: residual planes at every point, sums, loss, every layer block of the gradient).

A case whose three precisions are fp32 is held to BARS["fp32"], every other one to BARS["bf16x3"]: a triple with fp32
members is by construction no less accurate than bf16x3 throughout.  The CPU tests keep the case table honest without
a device: every row resolves to the kernels it names, the table and test_tile_loops.py together cover every name
triple the precision triples of the 6x256 plan resolve to, and every row's geometry loops at the point count used.
"""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import fwdmode_ref as fr

from test_tile_loops import (BARS, CASE_FAMILIES, PAIRED, SPLIT_256, _case, _compare, _cus, _net, _oracle, _points,
                             _rel_max, bpc_max, families_of, loop_violations, pick_n)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import plan_census  # noqa: E402

F32, X3 = "fp32", "bf16x3"
CODE = {F32: 0, X3: 1}                # precision codes of pinn_net_set_precision / the census keys


def _row(prec, names, tile, env=()):
    triple = tuple(prec.split(",")) if "," in prec else (prec,) * 3
    tag = prec + "".join(" %s=%s" % kv for kv in env)
    return dict(prec=prec, triple=triple, env=tuple(env), names=tuple(names), tile=tile, tag=tag,
                bar=F32 if triple == (F32,) * 3 else X3)


# hidden 256, 6 layers: net seed 1234, points seed 11, oracle key "6x256" (shared with test_tile_loops.py)
ROWS_256 = [
    _row("fp32,fp32,bf16x3", ("fwd_kernel", "bwd_kernel", "dw_bf16_kernel"), 32),
    _row("fp32,bf16x3,fp32", ("fwd_kernel", "bwd_pipe_kernel", "dw_kernel"), 32),
    _row("fp32,bf16x3,bf16x3", ("fwd_kernel", "bwd_pipe_kernel", "dw_bf16_kernel"), 32),
    _row("bf16x3,fp32,fp32", ("fwd_pipe_kernel", "bwd_kernel", "dw_kernel"), 32),
    _row("bf16x3,fp32,bf16x3", ("fwd_pipe_kernel", "bwd_kernel", "dw_bf16_kernel"), 32),
    _row("bf16x3,bf16x3,fp32", ("fwd_pipe_kernel", "bwd_pipe_kernel", "dw_kernel"), 32),
    _row(X3, ("fwd_pipe_kernel", "bwd_pipe_kernel", "dw_bf16_kernel"), 32, (("PINN_SCHED", "1"),)),
    _row(X3, ("fwd_pipe_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"), 32, (("PINN_BWD_SCHED", "0"),)),
    # the default pairing of 12x256
    _row(X3, ("fwd_bf16_kernel", "bwd_pipe_kernel", "dw_bf16_kernel"), 32,
         (("PINN_FWD_SCHED", "0"), ("PINN_BWD_SCHED", "1"))),
    # the 64-column bf16 kernels: 16-point tiles, up to two workgroups per CU
    _row(X3, ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"), 16, (("PINN_TILE_COLS", "64"),)),
    # the 128-column fp32 kernels, layer 0 recomputed by its readers (SPILL_SKIP0) and spilled
    _row(F32, ("fwd_kernel", "bwd_kernel", "dw_kernel"), 32, (("PINN_TILE_COLS", "128"),)),
    _row(F32, ("fwd_kernel", "bwd_kernel", "dw_kernel"), 32, (("PINN_TILE_COLS", "128"), ("PINN_S0_SKIP32", "0"))),
    # the unfused role-split pair: the default pairing of 8x256
    _row(X3, ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel"), 32, (("PINN_FUSE", "0"),)),
]
# hidden 400, 4 layers: net seed 31, points seed 13, oracle key "4x400"
ROWS_400 = [
    _row("bf16x3,bf16x3,fp32", ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_wide_kernel"), 16),
    _row("fp32,fp32,bf16x3", ("fwd_wide_kernel", "bwd_wide_kernel", "dw_bf16_wide_kernel"), 16),
    _row("fp32,bf16x3,bf16x3", ("fwd_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel"), 16),
    _row("bf16x3,fp32,fp32", ("fwd_bf16_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel"), 16),
    _row(F32, ("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel"), 16),
]
# config 4's shape (6x256 + 4x40 entropy net): the entropy net's value plan then runs bf16 sweeps with the fp32 dW too
ROW_EV = _row("bf16x3,bf16x3,fp32", ("fwd_pipe_kernel", "bwd_pipe_kernel", "dw_kernel"), 32)
SHAPES = {"6x256": (256, 6, ROWS_256), "4x400": (400, 4, ROWS_400)}
TABLE = [(256, 6, r) for r in ROWS_256] + [(400, 4, r) for r in ROWS_400] + [(256, 6, ROW_EV)]
# what test_tile_loops.py runs at 6x256
TILE_LOOPS_256 = [("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel"),
                  ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"),
                  ("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel")]
_ids = lambda rows: [r["tag"] for r in rows]


# --------------------------------------------------------------------------------------------------------------------
# CPU: the case table against the library's resolution, the golden census and the loop geometry
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("H,L,row", TABLE, ids=["%d %s" % (H, r["tag"]) for H, _, r in TABLE])
def test_case_table_names_what_the_library_resolves(lib, H, L, row):
    got = plan_census.run_case(lib, (H, L, tuple(CODE[p] for p in row["triple"]), 4, 360000, dict(row["env"])))
    assert got[1] == 0, got
    assert tuple(got[5:8]) == row["names"]


def test_table_covers_the_precision_triples_of_the_census(golden_dir):
    """Every name triple the 27 precision triples of the 6x256 plan resolve to (plain bf16 as bf16x3: the same kernels
    with one term) is run at a looping point count, here or in test_tile_loops.py."""
    with open(os.path.join(golden_dir, "plan_census.json")) as f:
        census = json.load(f)
    rows = {}
    for w in census:
        m = re.fullmatch(r"H256 L6 p([012]{3}) s4 n360000", w[0])
        if m:
            assert w[1] == 0, w
            rows[m.group(1)] = tuple(w[5:8])
    assert len(rows) == 27
    for code, names in rows.items():           # plain bf16 resolves as bf16x3 does
        assert names == rows[code.replace("2", "1")], (code, names)
    found = {names for code, names in rows.items() if "2" not in code}
    assert found == set(rows.values())
    run = {r["names"] for r in ROWS_256} | set(TILE_LOOPS_256)
    missing = sorted(found - run)
    assert not missing, "%d of the %d name triples of the census have no looping case: %r" % (
        len(missing), len(found), missing)
    assert len(found) == 8, "%d distinct name triples among the 27 precision triples" % len(found)


def _families(row, H):
    return families_of(row["names"], H, row["bar"] == F32, row["tile"])


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_row_loops_at_the_shared_point_count(cus, shape):
    H, L, rows = SHAPES[shape]
    fams, n_hidden = CASE_FAMILIES[shape]
    assert n_hidden == L
    n = pick_n(cus, fams, L)
    assert bpc_max(256, True) == 2 and bpc_max(256, False) == 1 and bpc_max(400, True) == 1
    for row in rows:
        for fam in _families(row, H):
            assert fam in fams, (row["tag"], fam)
            assert fam == (row["tile"], fam[1], 2 if (H, row["tile"]) == (256, 16) else 1)
            assert loop_violations(n, cus, *fam, L) == [], (row["tag"], fam)
    # the ev case runs at the point count of test_config4_shape_ev_loops_vs_oracle
    n = pick_n(cus, [SPLIT_256], 6)
    assert _families(ROW_EV, 256) == [SPLIT_256, SPLIT_256] and loop_violations(n, cus, *SPLIT_256, 6) == []
    assert all(k in PAIRED for k in ROW_EV["names"][:2])


# --------------------------------------------------------------------------------------------------------------------
# GPU: every pairing of the table iterating, against the chunked fp64 oracle over all points
# --------------------------------------------------------------------------------------------------------------------
INPUTS = {"6x256": dict(net_seed=1234, pt_seed=11, Re=2000.0), "4x400": dict(net_seed=31, pt_seed=13, Re=1500.0)}
_RUNS = {}


def _inputs(shape):
    H, L, _ = SHAPES[shape]
    c = INPUTS[shape]
    n = pick_n(_cus(), *CASE_FAMILIES[shape])
    x, y, _ = _points(n, c["pt_seed"])
    return L, H, c["Re"], _net(L, H, c["net_seed"]), x, y


def _run(monkeypatch, shape, row):
    """One engine and one loss_and_grad of a row, once per process: the bitwise comparisons reuse the oracle cases'."""
    key = (shape, row["tag"])
    if key not in _RUNS:
        L, H, Re, flat, x, y = _inputs(shape)
        _RUNS[key] = _case(monkeypatch, L, H, row["prec"], flat, x, y, Re, row["names"], env=row["env"],
                           tile=row["tile"])
    return _RUNS[key]


def _bitwise(a, b, keys):
    for k in keys:
        p, q = (a[k], b[k]) if k != "eqs" else (np.stack(a[k]), np.stack(b[k]))
        assert torch.equal(torch.from_numpy(np.asarray(p)), torch.from_numpy(np.asarray(q))), k


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS_256, ids=_ids(ROWS_256))
def test_6x256_pairings_loop_vs_oracle(monkeypatch, row):
    L, H, Re, flat, x, y = _inputs("6x256")
    ref = _oracle("6x256", L, H, flat, x, y, Re)
    got = _run(monkeypatch, "6x256", row)
    _compare("6x256 " + row["tag"], got, ref, row["bar"], L, H)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS_400, ids=_ids(ROWS_400))
def test_4x400_pairings_loop_vs_oracle(monkeypatch, row):
    """Mixed triples at hidden > 256: the wide bf16 kernels on the classic fp32-plane spill (their 24-bit format needs
    all three kernels in a bf16 mode), the fp32 wide kernels, and each dW kernel behind either sweep."""
    L, H, Re, flat, x, y = _inputs("4x400")
    ref = _oracle("4x400", L, H, flat, x, y, Re)
    got = _run(monkeypatch, "4x400", row)
    _compare("4x400 " + row["tag"], got, ref, row["bar"], L, H)


@pytest.mark.gpu
def test_unfused_pair_is_bitwise_the_fused_sweep_where_it_loops(monkeypatch):
    """$PINN_FUSE=0 launches fwd_split and bwd_split where the default launches fwdbwd_split: the same phase bodies, so
    the same bits - here with every workgroup taking 3-4 trips."""
    unfused = _run(monkeypatch, "6x256", ROWS_256[-1])
    assert ROWS_256[-1]["env"] == (("PINN_FUSE", "0"),)
    fused = _run(monkeypatch, "6x256", _row(X3, ROWS_256[-1]["names"], 32))
    _bitwise(unfused, fused, ("sums", "eqs", "grads"))


@pytest.mark.gpu
def test_fp32_layer0_recompute_is_bitwise_the_spilled_forward_where_it_loops(monkeypatch):
    """The 128-column fp32 kernels with layer 0 recomputed by its readers and with layer 0 spilled: one forward sweep,
    so field planes and sums agree to the bit."""
    skip, spilled = ROWS_256[-3], ROWS_256[-2]
    assert skip["env"] == (("PINN_TILE_COLS", "128"),) and spilled["env"] == skip["env"] + (("PINN_S0_SKIP32", "0"),)
    _bitwise(_run(monkeypatch, "6x256", skip), _run(monkeypatch, "6x256", spilled), ("eqs", "sums"))


@pytest.mark.gpu
def test_config4_shape_ev_mixed_triple_loops_vs_oracle(monkeypatch):
    """The inputs of test_config4_shape_ev_loops_vs_oracle with the fp32 dW kernel behind the pipelined bf16x3 sweeps;
    the entropy net's value plan runs the same triple.  vis_t is the run's own, so the oracle run is this case's."""
    L, H, Re = 6, 256, 4000.0
    n = pick_n(_cus(), [SPLIT_256], L)
    flat, flat_e = _net(L, H, 21), _net(4, 40, 22, n_out=1)
    x, y, rng = _points(n, 12, -1.0, 1.0)
    w = (0.3 + rng.rand(n)).astype(np.float32)
    got = _case(monkeypatch, L, H, ROW_EV["prec"], flat, x, y, Re, ROW_EV["names"], flat_e=flat_e, w=w, scale=2.0,
                tile=ROW_EV["tile"])
    Pe = fr.unflatten(flat_e.astype(np.float64), 2, 1, 4, 40)
    e, _ = fr.forward1(Pe, x.astype(np.float64), y.astype(np.float64))
    assert _rel_max(got["vtm0"], 0.05 * np.abs(e[:, 0])) <= BARS[X3]["eq"]
    vis_t = np.minimum(np.float32(20.0 / Re), got["vtm0"])
    np.testing.assert_allclose(got["vis_t"], vis_t, rtol=1e-6)
    ref = _oracle("config4 " + ROW_EV["prec"], L, H, flat, x, y, Re, vis_t=vis_t, w=w.astype(np.float64), scale=2.0,
                  params_e=Pe)
    _compare("6x256+4x40 ev " + ROW_EV["prec"], got, ref, ROW_EV["bar"], L, H)
