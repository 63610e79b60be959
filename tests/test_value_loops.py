"""The value-mode (1-stream) kernels where their tile loops repeat, against the fp64 oracle over all N points.

Every 8-wave kernel family has a 4-stream instantiation (the PDE residual; tests/test_tile_loops.py) and a 1-stream one
that computes plain network values: the boundary term, the supervised term with NaN-masked pressure targets, the
entropy net of the ev flavour (forward and reverse over every collocation point, every step) and predict().  A value
tile is 128 points (64 on the 64-column kernels), so the oracle tests elsewhere stop at ~17 value tiles: no workgroup
takes a second trip and no dW group sums two tiles.  Here N comes from the device's CU count (pick_n of
test_tile_loops.py on the value families) so that every workgroup takes 3-4 trips and every dW group sums >= 4 tiles
over a range that does not divide evenly, and the plans are driven directly (ValuePlan + grad_reduce): the value-mode
gradient is seen alone, per layer block, not diluted in a residual gradient's norm.

What a trip carries to the next, and a fault in which these cases are sized to show: the per-workgroup loss partials,
the layer-0 / output-layer / bias accumulators of the reverse sweep, the output-adjoint plane the forward writes at
c * npad + point and the reverse sweep reads back, the S / Z-bar spill addressing at one stream, a dW group's slab
accumulator.  The CPU tests pin the chunked value oracle, the geometry, and that the bars would catch a fault in ONE
tile (dropped, doubled or shifted adjoints move every layer block by more than twice the gradient bar).

Inputs.  A gradient is a sum over points; with incoherent adjoints (random signs) it is a random walk whose norm grows
as sqrt(N) while fp32 rounding grows with the sum of magnitudes, and a block's relative error would measure the
cancellation, not the kernel.  So the adjoints here have spatial structure, like the real ones (u - u_b on the lid,
-g4 of a smooth residual): targets are smooth fields the net does not match plus noise, explicit seeds are a smooth
field times magnitudes spread log-uniformly over three decades.
"""
import numpy as np
import pytest
import torch

from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr
from test_tile_loops import BARS, bpc_max, geometry, loop_violations, padded_hidden, pick_n

# bars of the small-N oracle tests: pred absolute in fp32 (test_predict_matches_forward1) and relative to
# max(1, max|ref|) in bf16x3 (test_wide_net_predict_and_fast_mode); sums and per-block gradient: BARS of test_tile_loops
PRED_BAR = {"fp32": 3e-6, "bf16x3": 2e-5}


# --------------------------------------------------------------------------------------------------------------------
# launch geometry of a value plan (nsfnet_amd/csrc/capi.hip, pinn_plan_create at streams == 1)
# --------------------------------------------------------------------------------------------------------------------
def value_tile(hidden, fp32):
    """Points per value tile: 64 on the 64-column kernels (padded hidden > 256, or 256 in all-fp32 mode), else 128."""
    hp = padded_hidden(hidden)
    return 64 if hp > 256 or (hp == 256 and fp32) else 128


def value_family(hidden, fp32):
    return (value_tile(hidden, fp32), False, bpc_max(hidden, fp32))


def loop_only_violations(n, cus, tile, paired, bpc):
    """loop_violations without the dW-group conditions, for one hidden layer (no hidden-to-hidden dW: groups == 0)."""
    return [v for v in loop_violations(n, cus, tile, paired, bpc, 2) if not v.endswith("dW groups")]


def pick_n_one_layer(cus, fam):
    """pick_n's rule on the loop conditions alone: the smallest tile count that satisfies them, its fullest n."""
    tile, paired, bpc = fam
    n = 3 * cus * tile * bpc
    while loop_only_violations(n, cus, *fam):
        n += 1
    while not loop_only_violations(n + 1, cus, *fam) and -(-(n + 1) // tile) == -(-n // tile):
        n += 1
    return n


# name: (L, H, n_out, kind of seeds); the precision decides the family at 6x256 only
CASES = {
    "4x40": (4, 40, 1, "seeds"),
    "4x50": (4, 50, 3, "boundary"),
    "6x128": (6, 128, 3, "supervised"),
    "6x256": (6, 256, 3, "supervised"),
    "8x400": (8, 400, 3, "boundary"),
    "2x512": (2, 512, 3, "boundary"),
    "1x8": (1, 8, 3, "boundary"),
}


def case_n(case, cus, fp32):
    L, H = CASES[case][:2]
    fam = value_family(H, fp32)
    return pick_n_one_layer(cus, fam) if L == 1 else pick_n(cus, [fam], L)


# --------------------------------------------------------------------------------------------------------------------
# seeded inputs
# --------------------------------------------------------------------------------------------------------------------
def _net(L, H, n_out, seed):
    return ar.flat_params(ar.seeded_net(n_out, L, H, seed=seed)).numpy().copy()


def _inputs(case, n, cus, fp32):
    """Points, and targets + coef or explicit seeds, of a case at n points (float32, as the plans hold them)."""
    L, H, n_out, kind = CASES[case]
    tile, _, bpc = value_family(H, fp32)
    rng = np.random.RandomState(1000 + 7 * L + H)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    out = dict(x=x, y=y, flat=_net(L, H, n_out, 300 + H + L), targets=None, coef=None, out_adj=None)
    noise = lambda: 0.05 * rng.randn(n)
    if kind == "seeds":
        # d loss / d e of the entropy net, as ResidualPlan.ebar: length padded to 128, the padding never read
        npad = -(-n // 128) * 128
        adj = np.zeros(npad, np.float32)
        adj[:n] = (0.3 + np.sin(2 * np.pi * x) * np.cos(np.pi * y)) * 10.0 ** rng.uniform(-3.0, 0.0, n) / n
        adj[n:] = 1.0e3      # a read past n would show
        out["out_adj"] = adj
        return out
    u = (0.25 + np.sin(2 * np.pi * x) * np.cos(np.pi * y) + noise()).astype(np.float32)
    v = (-0.2 + np.cos(3.0 * x) * np.sin(2 * np.pi * y) + noise()).astype(np.float32)
    if kind == "boundary":
        c = 2.0 * 10.0 / n
        out.update(targets=[u, v, None], coef=(c, c, 0.0))
        return out
    # supervised: NaN pressure targets - ~30 % anywhere, every other one in the ragged last tile, one tile of the
    # third trip with no finite p at all, one tile of the second trip with a single finite p
    p = (0.3 + np.sin(np.pi * (x - y)) + noise()).astype(np.float32)
    ntiles, grid = -(-n // tile), cus * bpc
    assert ntiles > 3 * grid
    p[rng.rand(n) < 0.3] = np.nan
    last = (ntiles - 1) * tile
    p[last:n:2] = np.nan
    t_all, t_one = 2 * grid + 5, grid + 7
    p[t_all * tile:(t_all + 1) * tile] = np.nan
    keep = p[t_one * tile + 37]
    p[t_one * tile:(t_one + 1) * tile] = np.nan
    p[t_one * tile + 37] = keep if np.isfinite(keep) else np.float32(0.25)
    n_p = int(np.isfinite(p).sum())
    out.update(targets=[u, v, p], coef=(2.0 / n, 2.0 / n, 2.0 / n_p), n_p=n_p, t_all=t_all, t_one=t_one)
    return out


def _params(inp, case):
    L, H, n_out, _ = CASES[case]
    return fr.unflatten(inp["flat"].astype(np.float64), 2, n_out, L, H)


def _seed_of(inp, n, n_out):
    return None if inp["out_adj"] is None else inp["out_adj"][:n].astype(np.float64).reshape(n, n_out)


_ORACLE = {}


def _oracle(case, n, cus, fp32):
    """Inputs and the chunked fp64 oracle of a case, once per (case, n, tile): the precision variants share it."""
    key = (case, n, cus, value_tile(CASES[case][1], fp32))
    if key not in _ORACLE:
        inp = _inputs(case, n, cus, fp32)
        ref = fr.value_loss_and_grad_chunked(_params(inp, case), inp["x"], inp["y"], targets=inp["targets"],
                                             coef=inp["coef"], out_adj=_seed_of(inp, n, CASES[case][2]))
        _ORACLE[key] = (inp, ref)
    return _ORACLE[key]


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def _block_errs(a, b, n_out, L, H):
    """rel-L2 error of every layer's weight and bias block."""
    blocks = lambda g: [q for wb in fr.unflatten(np.asarray(g, np.float64), 2, n_out, L, H) for q in wb]
    return [_rel_l2(p, q) for p, q in zip(blocks(a), blocks(b))]


# --------------------------------------------------------------------------------------------------------------------
# CPU: the chunked value oracle
# --------------------------------------------------------------------------------------------------------------------
def _small(n_out, n=23, L=2, H=12, seed=3):
    rng = np.random.RandomState(seed)
    P = fr.unflatten(_net(L, H, n_out, seed + 1).astype(np.float64), 2, n_out, L, H)
    x, y = rng.rand(n) * 2 - 1, rng.rand(n) * 2 - 1
    tg = [rng.randn(n) for _ in range(n_out)]
    tg[-1][rng.rand(n) < 0.4] = np.nan
    tg[-1][n - 1] = np.inf
    if n_out == 3:
        tg[1] = None
    return P, x, y, tg, [0.7, 1.9, 0.3][:n_out]


@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("chunk", [1, 7, 23])
def test_chunked_value_oracle_equals_one_pass(n_out, chunk):
    P, x, y, tg, coef = _small(n_out)
    pred, saved = fr.forward1(P, x, y)
    adj, sums = np.zeros_like(pred), np.zeros(4)
    for c in range(n_out):
        if tg[c] is None:
            continue
        for i in range(x.size):
            if np.isfinite(tg[c][i]):
                d = pred[i, c] - tg[c][i]
                sums[c] += d * d
                sums[3] += c == 2
                adj[i, c] = coef[c] * d
    grad = fr.backward1(P, x, y, saved, adj)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
    got = fr.value_loss_and_grad_chunked(P, x, y, targets=tg, coef=coef, chunk=chunk)
    assert rel(got["pred"], pred) <= 1e-12 and got["pred"].shape == (x.size, n_out)
    assert rel(got["sums"], sums) <= 1e-12 and got["sums"][3] == sums[3]
    assert rel(got["grad"], grad) <= 1e-12
    # NaN-masked targets against the same adjoints given explicitly; an explicit seed takes precedence over targets
    for kw in (dict(), dict(targets=tg, coef=[5.0] * n_out)):
        got2 = fr.value_loss_and_grad_chunked(P, x, y, out_adj=adj if n_out > 1 else adj[:, 0], chunk=chunk, **kw)
        assert rel(got2["grad"], grad) <= 1e-12
    assert got2["sums"][3] == sums[3]
    assert fr.value_loss_and_grad_chunked(P, x, y, chunk=chunk)["sums"] == [0.0] * 4


@pytest.mark.parametrize("chunk", [1, 100, 8192])
def test_chunked_value_oracle_equals_bc_loss_and_grad(chunk):
    L, H = 3, 20
    P = fr.unflatten(_net(L, H, 3, 8).astype(np.float64), 2, 3, L, H)
    xb, yb, ub, vb = (a.reshape(-1)[::16] for a in ar.cavity_boundary())
    b = fr.bc_loss_and_grad(P, xb, yb, ub, vb, alpha_b=10.0)
    c = 2.0 * 10.0 / xb.size
    got = fr.value_loss_and_grad_chunked(P, xb, yb, targets=[ub, vb, None], coef=(c, c, 0.0), chunk=chunk)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
    assert rel(got["grad"], b["grad"]) <= 1e-12
    assert rel(got["sums"][:2], b["sums"]) <= 1e-12 and got["sums"][2:] == [0.0, 0.0]
    assert rel(got["pred"], b["pred"]) <= 1e-12


# --------------------------------------------------------------------------------------------------------------------
# CPU: the geometry
# --------------------------------------------------------------------------------------------------------------------
def test_value_families():
    assert value_family(40, False) == value_family(50, True) == (128, False, 4)
    assert value_family(128, True) == value_family(128, False) == (128, False, 2)
    assert value_family(256, False) == (128, False, 1) and value_family(256, True) == (64, False, 2)
    assert value_family(400, False) == value_family(512, False) == (64, False, 1)
    assert value_family(8, True) == (128, False, 8)


def test_value_pick_n_known_values():
    # 256 CUs: 3 * grid + 1 tiles of 128 (64) points, the last one a point short
    for case in ("4x40", "4x50"):
        n = case_n(case, 256, False)
        assert n == 393343 == case_n(case, 256, True)
        g = geometry(n, 256, *value_family(CASES[case][1], False), 4)
        assert (g["ntiles"], g["grid"], g["groups"]) == (3073, 1024, [85, 170, 256, 341])
    assert case_n("6x128", 256, True) == case_n("6x128", 256, False) == 196735
    assert case_n("6x256", 256, False) == 98431
    g = geometry(98431, 256, *value_family(256, False), 6)
    assert (g["ntiles"], g["groups"]) == (769, [51])
    assert case_n("6x256", 256, True) == 98367
    assert geometry(98367, 256, *value_family(256, True), 6)["ntiles"] == 1537
    assert case_n("8x400", 256, False) == 49215
    g = geometry(49215, 256, *value_family(400, False), 8)
    assert (g["ntiles"], g["groups"]) == (769, [36])
    assert case_n("2x512", 256, False) == 65599
    # one hidden layer: 8 workgroups per CU, 3 * 2048 + 1 tiles
    assert case_n("1x8", 256, True) == 128 * (3 * 2048 + 1) - 1


@pytest.mark.parametrize("cus", [256, 80, 32])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("fp32", [False, True])
def test_value_pick_n_makes_every_loop_repeat(cus, case, fp32):
    L, H = CASES[case][:2]
    fam = value_family(H, fp32)
    n = case_n(case, cus, fp32)
    if L == 1:
        assert loop_only_violations(n, cus, *fam) == []
    else:
        assert loop_violations(n, cus, *fam, L) == []
    g = geometry(n, cus, *fam, max(L, 2))
    assert g["grid"] == cus * fam[2] and g["loop"] > 3 * g["grid"] and g["loop"] % g["grid"]
    if L > 1:
        assert all(4 <= g["ntiles"] // gr and g["ntiles"] % gr for gr in g["groups"])
    assert loop_only_violations(fam[0] * 3 * g["grid"], cus, *fam) != []      # the wrapper keeps the loop conditions


# --------------------------------------------------------------------------------------------------------------------
# CPU: the gradient bar sees a fault in one tile
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["4x40", "4x50", "6x128", "6x256", "8x400"])
def test_block_bar_catches_a_one_tile_fault(case):
    """One tile's adjoints dropped (a late tile), doubled (a mid-range tile of the second trip) or taken from the tile
    before (third trip), in the fp64 oracle at pick_n(32 CUs): every layer block moves by more than twice the GPU
    gradient bar.  (At 256 CUs a tile's share is 8x smaller.  Measured on the oracle with these inputs, dropping tile
    ntiles - 3 there moves every block by >= 2.9e-4 at 4x40 and 4x50 / 393343 points, the weakest cases, 6.0e-4 at
    6x128, 9.5e-4 at 2x512, >= 1.3e-3 at 6x256 and 8x400 - three times the bar or more - while an fp32 restatement
    of the oracle sits <= 6e-7 per block from it.)"""
    cus, fp32 = 32, False
    L, H, n_out, _ = CASES[case]
    n = case_n(case, cus, fp32)
    tile, _, bpc = value_family(H, fp32)
    inp, ref = _oracle(case, n, cus, fp32)
    P, x, y = _params(inp, case), inp["x"], inp["y"]
    if inp["out_adj"] is not None:
        adj = _seed_of(inp, n, n_out)
    else:
        adj = np.zeros((n, n_out))
        for c, t in enumerate(inp["targets"]):
            if t is not None:
                ok = np.isfinite(t)
                adj[ok, c] = inp["coef"][c] * (ref["pred"][ok, c] - t[ok].astype(np.float64))
    grad = lambda a: fr.value_loss_and_grad_chunked(P, x, y, out_adj=a)["grad"]
    assert max(_block_errs(grad(adj), ref["grad"], n_out, L, H)) <= 1e-12
    ntiles, grid = -(-n // tile), cus * bpc
    sl = lambda t: slice(t * tile, (t + 1) * tile)
    drop, dbl, shift = adj.copy(), adj.copy(), adj.copy()
    drop[sl(ntiles - 3)] = 0.0
    dbl[sl(grid + grid // 2)] *= 2.0
    shift[sl(2 * grid + 1)] = adj[sl(2 * grid)]
    for tag, a in (("drop", drop), ("double", dbl), ("shift", shift)):
        moved = _block_errs(grad(a), ref["grad"], n_out, L, H)
        print("[value loops] %s %s one tile of %d: blocks move %.2e .. %.2e" % (case, tag, ntiles, min(moved), max(moved)))
        assert min(moved) > 2.0 * max(BARS["bf16x3"]["grad"], BARS["fp32"]["grad"]), (tag, moved)


# --------------------------------------------------------------------------------------------------------------------
# GPU: ValuePlan + grad_reduce alone, every loop repeating
# --------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _clear_env(monkeypatch):
    import os
    for k in list(os.environ):
        if k.startswith("PINN_") or k.startswith("NSFNET_"):
            monkeypatch.delenv(k, raising=False)


def _names(H, prec):
    wide = "_wide" if value_tile(H, prec == "fp32") == 64 else ""
    if prec == "fp32":
        return tuple(k + wide + "_kernel" for k in ("fwd", "bwd", "dw"))
    wide = "_wide" if padded_hidden(H) > 256 else ""
    return tuple(k + "_bf16" + wide + "_kernel" for k in ("fwd", "bwd", "dw"))


def _run(monkeypatch, case, prec, with_backward=True):
    """The case's plan on the device, its geometry asserted; returns inputs, oracle and what the plan computed."""
    from nsfnet_amd import engine as eng
    _clear_env(monkeypatch)
    L, H, n_out, kind = CASES[case]
    cus, fp32 = _cus(), prec == "fp32"
    n = case_n(case, cus, fp32)
    fam = value_family(H, fp32)
    inp, ref = _oracle(case, n, cus, fp32)
    dev = torch.device("cuda:0")
    net = eng.DeviceNet(n_out, L, H, dev, precision=prec)
    net.set_flat(torch.tensor(inp["flat"]))
    plan = eng.ValuePlan(net, inp["x"], inp["y"], targets=inp["targets"] if with_backward else None,
                         with_backward=with_backward)
    # the geometry this case is for
    assert plan.kernel_names() == _names(H, prec)
    assert plan.npad == -(-n // fam[0]) * fam[0]
    bad = loop_only_violations(n, cus, *fam) if L == 1 else loop_violations(n, cus, *fam, L)
    assert bad == [], (fam, bad)
    g = geometry(n, cus, *fam, max(L, 2))
    geo = "tiles %d grid <= %d (>= %d trips) dW groups %s (>= %d tiles)" % (
        g["ntiles"], g["grid"], g["ntiles"] // g["grid"], g["groups"] if L > 1 else 0,
        min(g["ntiles"] // gr for gr in g["groups"]) if L > 1 else 0)
    got = dict(geo=geo, n=n)
    if with_backward:
        plan.forward(coef=inp["coef"] or (0.0, 0.0, 0.0), save=True)
        seeds = None
        if inp["out_adj"] is not None:
            seeds = torch.tensor(inp["out_adj"]).to(dev)
            assert seeds.numel() == -(-n // 128) * 128
        plan.backward(out_adj=seeds)
        grads = torch.full((net.num_params,), float("nan"), dtype=torch.float32, device=dev)
        eng.grad_reduce(net, [plan], grads)
        torch.cuda.synchronize()
        got.update(sums=plan.sums.cpu().numpy().astype(np.float64), grad=grads.cpu().numpy().astype(np.float64))
        if seeds is not None:
            # the same reverse sweep from seeds with one late tile blanked: what the comparison must not let pass
            seeds[(g["ntiles"] - 3) * fam[0]:(g["ntiles"] - 2) * fam[0]] = 0.0
            plan.backward(out_adj=seeds)
            eng.grad_reduce(net, [plan], grads)
            torch.cuda.synchronize()
            got["grad_one_tile_blank"] = grads.cpu().numpy().astype(np.float64)
    else:
        plan.forward(save=False)
        torch.cuda.synchronize()
    got["pred"] = plan.pred.cpu().numpy().astype(np.float64).T
    del plan, net
    torch.cuda.empty_cache()
    return inp, ref, got


def _compare(tag, case, prec, inp, ref, got):
    """pred at every point and channel, the sums of the channels that have targets (and the exact finite-p count),
    every layer block of the gradient."""
    L, H, n_out, _ = CASES[case]
    errs = {}
    d = np.abs(got["pred"] - ref["pred"])
    errs["pred"] = float(d.max())
    pred_bar = PRED_BAR[prec] * (1.0 if prec == "fp32" else max(1.0, float(np.abs(ref["pred"]).max())))
    first = int(np.argmax(d.max(axis=1) > pred_bar)) if errs["pred"] > pred_bar else -1
    if "grad" in got:
        with_t = [c for c in range(n_out) if inp["targets"] is not None and inp["targets"][c] is not None]
        for c in with_t:
            errs["sum%d" % c] = abs(got["sums"][c] - ref["sums"][c]) / ref["sums"][c]
        blocks = _block_errs(got["grad"], ref["grad"], n_out, L, H)
        errs["grad"] = max(blocks)
    print("[value loops] %s N=%d %s: %s" % (tag, got["n"], got["geo"], " ".join("%s %.2e" % kv for kv in errs.items())))
    assert errs["pred"] <= pred_bar, ("pred", errs["pred"], "first point over the bar", first)
    if "grad" in got:
        for c in with_t:
            assert errs["sum%d" % c] <= BARS[prec]["sums"], (c, errs["sum%d" % c])
        assert got["sums"][3] == ref["sums"][3] == inp.get("n_p", 0)
        assert np.isfinite(got["grad"]).all()
        assert errs["grad"] <= BARS[prec]["grad"], ("grad blocks", blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_entropy_net_value_loops_vs_oracle(monkeypatch, prec):
    """4x40, one output: the entropy net's reverse sweep from explicit seeds laid out as ResidualPlan.ebar."""
    inp, ref, got = _run(monkeypatch, "4x40", prec)
    _compare("4x40 n_out 1 seeds %s" % prec, "4x40", prec, inp, ref, got)
    # the control: with one of the ~3 * CUs * 4 tiles' seeds blanked on the device, every block leaves the bar
    moved = _block_errs(got["grad_one_tile_blank"], ref["grad"], 1, 4, 40)
    print("[value loops] 4x40 %s, one tile's seeds blanked: blocks %.2e .. %.2e from the oracle" % (prec, min(moved), max(moved)))
    assert min(moved) > BARS[prec]["grad"], moved


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_boundary_like_value_loops_vs_oracle(monkeypatch, prec):
    """4x50, targets on u and v only, coef (c, c, 0): the boundary term's shape, 4 workgroups per CU."""
    inp, ref, got = _run(monkeypatch, "4x50", prec)
    _compare("4x50 boundary %s" % prec, "4x50", prec, inp, ref, got)


@pytest.mark.gpu
@pytest.mark.parametrize("case,prec", [("6x128", "fp32"), ("6x256", "bf16x3"), ("6x256", "fp32")])
def test_supervised_value_loops_vs_oracle(monkeypatch, case, prec):
    """u, v, p targets with NaN p: narrow fp32 (2 workgroups per CU), the headline width on the 128-column bf16
    kernels, and fp32's 64-column kernels."""
    inp, ref, got = _run(monkeypatch, case, prec)
    _compare("%s supervised %s" % (case, prec), case, prec, inp, ref, got)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["8x400", "2x512"])
def test_wide_value_loops_vs_oracle(monkeypatch, case):
    inp, ref, got = _run(monkeypatch, case, "bf16x3")
    _compare("%s boundary bf16x3" % case, case, "bf16x3", inp, ref, got)


@pytest.mark.gpu
def test_one_hidden_layer_value_loops_vs_oracle(monkeypatch):
    """1x8: no hidden-to-hidden dW (groups == 0); layer 0, the output layer and the biases all come from the reverse
    sweep's accumulators, 8 workgroups per CU."""
    inp, ref, got = _run(monkeypatch, "1x8", "fp32")
    _compare("1x8 boundary fp32", "1x8", "fp32", inp, ref, got)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["6x256", "8x400"])
def test_predict_value_loops_vs_oracle(monkeypatch, case):
    """predict()'s plan (no backward workspace, no targets) at the same N."""
    inp, ref, got = _run(monkeypatch, case, "bf16x3", with_backward=False)
    _compare("%s predict bf16x3" % case, case, "bf16x3", inp, ref, got)


@pytest.mark.gpu
def test_ev_hand_over_value_loops_vs_oracle(monkeypatch):
    """residual reverse sweep -> ebar -> value reverse sweep -> dW with the value side iterating: 2x16 main net, 4x40
    entropy net (trainable), bf16x3, N = pick_n of the entropy net's value family (the 32-point residual tiles loop
    there too)."""
    from nsfnet_amd import engine as eng
    _clear_env(monkeypatch)
    L, H, Re, prec = 2, 16, 1000.0, "bf16x3"
    cus = _cus()
    fam = value_family(40, False)
    n = pick_n(cus, [fam], 4)
    flat, flat_e = _net(L, H, 3, 61), _net(4, 40, 1, 62)
    rng = np.random.RandomState(16)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    E = eng.PinnEngine(torch.device("cuda:0"), L, H, Re, alpha_b=10.0, alpha_e=1.0, precision=prec, flavour="ev",
                       n_hidden_e=4, hidden_e=40, alpha_evm=0.05)
    E.net.set_flat(torch.tensor(flat))
    E.net_e.set_flat(torch.tensor(flat_e))
    E.e_trainable = True
    E.set_collocation(x, y)
    E.set_boundary(*(a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary()))
    plan_e = E.plan_e
    assert plan_e.kernel_names() == _names(40, prec) and plan_e.npad == -(-n // 128) * 128
    assert loop_violations(n, cus, *fam, 4) == []
    g = geometry(n, cus, 32, False, bpc_max(H, False), L)
    assert E.plan_f.npad == g["ntiles"] * 32 and g["loop"] >= 3 * g["grid"] + 1
    vtm0 = E.plan_f.vis_t_minus.cpu().numpy().astype(np.float64)
    E.loss_and_grad()
    torch.cuda.synchronize()
    grads_e = E.grads_e.cpu().numpy().astype(np.float64)
    vtm1 = E.plan_f.vis_t_minus.cpu().numpy().astype(np.float64)
    vis_t_dev = E.plan_f.vis_t.cpu().numpy().astype(np.float64)
    del E, plan_e
    torch.cuda.empty_cache()
    Pe = fr.unflatten(flat_e.astype(np.float64), 2, 1, 4, 40)
    e, _ = fr.forward1(Pe, x.astype(np.float64), y.astype(np.float64))
    vtm_ref = 0.05 * np.abs(e[:, 0])
    vis_t = np.minimum(np.float32(20.0 / Re), vtm0)
    np.testing.assert_allclose(vis_t_dev, vis_t, rtol=1e-6)
    ref = fr.pde_loss_and_grad_chunked(fr.unflatten(flat.astype(np.float64), 2, 3, L, H), x, y, Re, vis_t=vis_t,
                                       params_e=Pe)
    blocks = _block_errs(grads_e, ref["grad_e"], 1, 4, 40)
    errs = dict(vtm0=float(np.abs(vtm0 - vtm_ref).max() / vtm_ref.max()),
                vtm1=float(np.abs(vtm1 - vtm_ref).max() / vtm_ref.max()), grad_e=max(blocks))
    vg = geometry(n, cus, *fam, 4)
    print("[value loops] 2x16+4x40 ev bf16x3 N=%d tiles %d grid <= %d dW groups %s; residual tiles %d grid <= %d: %s" % (
        n, vg["ntiles"], vg["grid"], vg["groups"], g["ntiles"], g["grid"], " ".join("%s %.2e" % kv for kv in errs.items())))
    # (the entropy net runs in bf16x3: its output carries that mode's field error)
    assert errs["vtm0"] <= BARS[prec]["eq"] and errs["vtm1"] <= BARS[prec]["eq"]
    assert errs["grad_e"] <= BARS[prec]["grad"], ("grad_e blocks", blocks)
