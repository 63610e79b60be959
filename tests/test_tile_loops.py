"""The kernels' tile loops, run for real: every workgroup of every sweep takes 3 or 4 trips round its loop, against the
fp64 oracle over all N points.

Each HIP kernel takes tiles (the role-split / pipelined sweeps: pairs of tiles) at a stride of its grid, and dW gives
each group a contiguous range of tiles.  The oracle tests elsewhere stop at a few hundred tiles, where no workgroup
repeats and no dW group sums more than two tiles; the state a loop carries from one trip to the next (next-tile
seeds, the staged point of the previous tile, an odd count's dummy partner, a group's accumulator) is then never
exercised.  Here N is chosen from the device's CU count (pick_n) so that, for every kernel family a case launches:
  * loop count >= 3 * grid + 1 and not a multiple of the grid (pairs for the paired sweeps, tiles for the 8-wave ones, whose grid is taken at its
    upper bound CUs * bpc_max so that the statement holds whatever the LDS allows);
  * the tile count is odd (the paired sweeps' dummy partner falls on a later pair) and N is not a tile multiple, with
    the last tiles as full as that allows;
  * every dW group sums >= 4 tiles and the groups do not divide the tiles evenly, for every group count the plan
    could pick.
The CPU tests pin the chunked oracle and the geometry helper; the GPU cases assert the geometry from the plan's padded
point count and kernel names before they compare anything.
"""
import numpy as np
import pytest
import torch

from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr

PAIRED = ("fwd_split_kernel", "bwd_split_kernel", "fwd_pipe_kernel", "bwd_pipe_kernel", "fwd_wsplit_kernel",
          "bwd_wsplit_kernel")

# bars of the small-N oracle tests (test_hip_kernels.py, test_pipelined_kernels.py): fields max-abs / max|ref|, loss
# sums relative, loss relative, gradients relative L2
BARS = {"fp32": dict(eq=2e-5, sums=1e-5, loss=1e-5, grad=1e-4),
        "bf16x3": dict(eq=5e-4, sums=2e-4, loss=1e-4, grad=1e-4)}


# --------------------------------------------------------------------------------------------------------------------
# launch geometry (nsfnet_amd/csrc/capi.hip, pinn_plan_create)
# --------------------------------------------------------------------------------------------------------------------
def padded_hidden(hidden):
    return (hidden + 31) // 32 * 32


def tile_points(hidden, fp32):
    """Points per tile of a residual plan: 16 for the 64-column kernels (hidden > 256, and fp32 at 256), else 32."""
    hp = padded_hidden(hidden)
    return 16 if hp > 256 or (hp == 256 and fp32) else 32


def bpc_max(hidden, fp32):
    """Upper bound of the workgroups per CU of the 8-wave sweeps and of dW (the cap of pinn_plan_create's bpc)."""
    hp = padded_hidden(hidden)
    nw = hp // 32
    if nw >= 8:
        return 2 if tile_points(hidden, fp32) == 16 and nw == 8 else 1
    return 8 // nw


def geometry(n, cus, tile, paired, bpc, n_hidden):
    """Loop count, grid (bound), tile count and the possible dW group counts of one kernel family at n points."""
    ntiles = -(-n // tile)
    loop = (ntiles + 1) // 2 if paired else ntiles
    grid = min(cus, loop) if paired else min(cus * bpc, ntiles)
    groups = sorted({max(1, min(ntiles, cus * b // (n_hidden - 1))) for b in range(1, bpc + 1)})
    return dict(ntiles=ntiles, loop=loop, grid=grid, groups=groups)


def loop_violations(n, cus, tile, paired, bpc, n_hidden):
    g = geometry(n, cus, tile, paired, bpc, n_hidden)
    bad = []
    if g["loop"] < 3 * g["grid"] + 1:
        bad.append("loop %d < 3 * grid %d + 1" % (g["loop"], g["grid"]))
    if g["loop"] % g["grid"] == 0:
        bad.append("every workgroup takes %d trips" % (g["loop"] // g["grid"]))
    if g["ntiles"] % 2 == 0:
        bad.append("even tile count %d" % g["ntiles"])
    if n % tile == 0:
        bad.append("n a multiple of %d" % tile)
    for gr in g["groups"]:
        if g["ntiles"] // gr < 4 or g["ntiles"] % gr == 0:
            bad.append("%d tiles over %d dW groups" % (g["ntiles"], gr))
    return bad


def pick_n(cus, families, n_hidden):
    """A point count at which every (tile, paired, bpc) family of a case repeats its loops as the module docstring
    requires: the smallest tile counts that do, and within them the largest n."""
    lo = max(3 * cus * (2 * tile if paired else tile * bpc) for tile, paired, bpc in families)
    ok = lambda n: not any(loop_violations(n, cus, t, p, b, n_hidden) for t, p, b in families)
    tiles = lambda n: [-(-n // t) for t, _, _ in families]
    for n in range(lo, 64 * lo):
        if ok(n):
            # the same tile counts, with the last tiles as full as the conditions allow: a ragged tile of one point
            # would hide a fault in the odd count's last pair under the bars
            while ok(n + 1) and tiles(n + 1) == tiles(n):
                n += 1
            return n
    raise AssertionError("no point count found")


def families_of(names, hidden, fp32, tile=None):
    """(tile, paired, bpc) of the forward and reverse sweeps a plan launches, from its kernel names.  tile: the points
    per tile where precision alone does not tell them (a precision triple, $PINN_TILE_COLS)."""
    if tile is None:
        tile = tile_points(hidden, fp32)
    b = bpc_max(hidden, tile == 16)
    return [(tile, k in PAIRED, b) for k in names[:2]]


SPLIT_256 = (32, True, 1)       # role-split sweeps, hidden 256, bf16 modes
EIGHT_256 = (32, False, 1)      # 8-wave bf16 sweeps, hidden 256 ($PINN_SCHED=0)
FP32_256 = (16, False, 2)       # 8-wave fp32 sweeps, hidden 256 (64-column tiles)
WSPLIT = (16, True, 1)          # wide role-split sweeps, hidden 288..448
WIDE = (16, False, 1)           # 8-wave wide bf16 sweeps ($PINN_WSPLIT=0)
CASE_FAMILIES = {
    "6x256": ([SPLIT_256, EIGHT_256, FP32_256], 6),
    "4x400": ([WSPLIT, WIDE], 4),
    "8x400": ([WSPLIT], 8),
    "4x50": ([(32, False, 4)], 4),
    "6x128": ([(32, False, 2)], 6),
}


# --------------------------------------------------------------------------------------------------------------------
# CPU: the chunked oracle and the geometry
# --------------------------------------------------------------------------------------------------------------------
def _small_case(ev, n=23, L=2, H=12, seed=0):
    rng = np.random.RandomState(seed)
    P = fr.unflatten(ar.flat_params(ar.seeded_net(3, L, H, seed=seed + 1)).numpy().astype(np.float64), 2, 3, L, H)
    x, y = rng.rand(n) * 2 - 1, rng.rand(n) * 2 - 1
    kw = {}
    if ev:
        kw = dict(vis_t=0.01 * rng.rand(n), w=0.5 + rng.rand(n), scale=2.0)
    return P, x, y, kw


@pytest.mark.parametrize("ev", [False, True])
@pytest.mark.parametrize("chunk", [1, 7, 23])
def test_chunked_oracle_equals_one_pass(ev, chunk):
    P, x, y, kw = _small_case(ev)
    Pe = fr.unflatten(ar.flat_params(ar.seeded_net(1, 2, 8, seed=9)).numpy().astype(np.float64), 2, 1, 2, 8) if ev else None
    e = saved_e = None
    if ev:
        ev_out, saved_e = fr.forward1(Pe, x, y)
        e = ev_out[:, 0]
    ref = fr.pde_loss_and_grad(P, x, y, 1000.0, alpha_e=1.3, e=e, **kw)
    got = fr.pde_loss_and_grad_chunked(P, x, y, 1000.0, alpha_e=1.3, params_e=Pe, chunk=chunk, **kw)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
    assert len(got["eqs"]) == len(ref["eqs"]) == (4 if ev else 3)
    assert rel(got["sums"], ref["sums"]) <= 1e-12
    assert rel(got["grad"], ref["grad"]) <= 1e-12
    assert rel(got["out"], ref["out"]) <= 1e-12
    for a, b in zip(got["eqs"], ref["eqs"]):
        assert rel(a, b) <= 1e-12
    if ev:
        ge = fr.backward1(Pe, x, y, saved_e, ref["e_adj"].reshape(-1, 1))
        assert rel(got["grad_e"], ge) <= 1e-12
        # an explicit e takes precedence over the entropy net's output and gives the same result here
        got2 = fr.pde_loss_and_grad_chunked(P, x, y, 1000.0, alpha_e=1.3, e=e, params_e=Pe, chunk=chunk, **kw)
        assert rel(got2["grad_e"], ge) <= 1e-12
    else:
        assert "grad_e" not in got


@pytest.mark.parametrize("cus", [256, 80, 32])
@pytest.mark.parametrize("case", sorted(CASE_FAMILIES))
def test_pick_n_makes_every_loop_repeat(cus, case):
    fams, L = CASE_FAMILIES[case]
    n = pick_n(cus, fams, L)
    for tile, paired, bpc in fams:
        assert loop_violations(n, cus, tile, paired, bpc, L) == []
        g = geometry(n, cus, tile, paired, bpc, L)
        assert g["grid"] == (cus if paired else cus * bpc)     # the whole device is busy: no loop is cut short
        assert g["loop"] > 3 * g["grid"] and g["loop"] % g["grid"]    # >= 3 trips, not all workgroups the same
        assert all(4 <= g["ntiles"] // gr and g["ntiles"] % gr for gr in g["groups"])


def test_pick_n_known_values():
    # 6x256 at 256 CUs: 6 * 256 + 1 = 1537 tiles of 32 points (769 pairs; 3073 tiles of 16 for fp32), 51 dW groups
    assert pick_n(256, *CASE_FAMILIES["6x256"]) == 32 * 6 * 256 + 15
    # the wide role-split sweeps at 256 CUs: 1537 tiles of 16 points
    assert pick_n(256, *CASE_FAMILIES["8x400"]) == 16 * 6 * 256 + 15
    assert geometry(16 * 6 * 256 + 15, 256, *WSPLIT, 8)["groups"] == [36]
    # the geometry restates capi.hip: even / multiple counts are rejected
    assert loop_violations(32 * (6 * 256 + 3), 256, *SPLIT_256, 6) == ["n a multiple of 32"]
    assert "even tile count 1538" in loop_violations(32 * 6 * 256 + 33, 256, *SPLIT_256, 6)
    assert bpc_max(256, True) == 2 and bpc_max(256, False) == 1 and bpc_max(50, False) == 4 and bpc_max(400, False) == 1
    assert tile_points(128, True) == 32 and tile_points(256, True) == 16 and tile_points(400, False) == 16


# --------------------------------------------------------------------------------------------------------------------
# GPU: every sweep and dW iterating, against the chunked fp64 oracle over all points
# --------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rel_max(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def _block_rel_l2(a, b, n_out, L, H):
    """Largest rel-L2 error over the weight and bias blocks of each layer: a fault in one layer's dW (or in one tile's
    share of it) is diluted in the norm of the whole gradient, which the output layer's blocks dominate."""
    blocks = lambda g: [q for wb in fr.unflatten(np.asarray(g, np.float64), 2, n_out, L, H) for q in wb]
    return max(_rel_l2(p, q) for p, q in zip(blocks(a), blocks(b)))


def _bc():
    return tuple(a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())


_ORACLE = {}


def _oracle(key, L, H, flat, x, y, Re, **kw):
    """The chunked oracle, once per key: the cases that differ only in schedule or precision share it."""
    if key not in _ORACLE:
        P = fr.unflatten(flat.astype(np.float64), 2, 3, L, H)
        r = fr.pde_loss_and_grad_chunked(P, x.astype(np.float64), y.astype(np.float64), Re, **kw)
        xb, yb, ub, vb = _bc()
        b = fr.bc_loss_and_grad(P, xb.astype(np.float64), yb.astype(np.float64), ub, vb, alpha_b=10.0)
        _ORACLE[key] = (r, b)
    return _ORACLE[key]


def _case(monkeypatch, L, H, prec, flat, x, y, Re, names, env=(), flat_e=None, w=None, scale=1.0, tile=None):
    from nsfnet_amd import engine as eng
    for k in ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_TILE_COLS", "PINN_STAGGER",
              "PINN_FUSE", "PINN_S0_SKIP32", "NSFNET_CHUNK_POINTS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    ev = flat_e is not None
    kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05, coord_scale=scale) if ev else {}
    E = eng.PinnEngine(torch.device("cuda:0"), L, H, Re, alpha_b=10.0, alpha_e=1.0, precision=prec, **kw)
    E.net.set_flat(torch.tensor(flat))
    if ev:
        E.net_e.set_flat(torch.tensor(flat_e))
        E.e_trainable = True
    E.set_collocation(x, y, weights=w)
    E.set_boundary(*_bc())
    # the geometry this case is for: the intended kernel families, each of them looping
    n, cus, fp32 = x.size, _cus(), prec == "fp32"
    assert E.plan_f.kernel_names() == names
    if tile is None:
        tile = tile_points(H, fp32)
    assert E.plan_f.npad == -(-n // tile) * tile
    for fam in families_of(names, H, fp32, tile):
        assert loop_violations(n, cus, *fam, L) == [], (fam, loop_violations(n, cus, *fam, L))
    out = dict(vtm0=E.plan_f.vis_t_minus.cpu().numpy().astype(np.float64) if ev else None)
    E.loss_and_grad()
    torch.cuda.synchronize()
    fields = ("eq1", "eq2", "eq3", "eq4") if ev else ("eq1", "eq2", "eq3")
    out.update(eqs=[E.plan_f.field(k).cpu().numpy().astype(np.float64) for k in fields],
               sums=E.sums.cpu().numpy().astype(np.float64), loss=float(E.loss_terms()["loss"]),
               grads=E.grads.cpu().numpy().astype(np.float64), n_b=E.n_b_global)
    if ev:
        out["grads_e"] = E.grads_e.cpu().numpy().astype(np.float64)
        out["vis_t"] = E.plan_f.vis_t.cpu().numpy().astype(np.float64)
    del E
    torch.cuda.empty_cache()
    return out


def _compare(tag, got, ref, prec, L, H):
    """Residual planes at every point, sums[0:4], the loss, the gradient (and the entropy net's) at the small-N bars -
    the gradient's bar on every layer's weight and bias block."""
    r, b = ref
    bar = BARS[prec]
    n = r["eqs"][0].size
    errs = {}
    for k, q in enumerate(got["eqs"]):
        errs["eq%d" % (k + 1)] = _rel_max(q, r["eqs"][k])
    nq = len(got["eqs"])
    errs["sums"] = _rel_max(got["sums"][:nq], np.asarray(r["sums"]))
    ref_loss = 10.0 * sum(b["sums"]) / got["n_b"] + (sum(r["sums"][:3]) + (0.1 * r["sums"][3] if nq == 4 else 0.0)) / n
    errs["loss"] = abs(got["loss"] - ref_loss) / ref_loss
    errs["grad"] = _block_rel_l2(got["grads"], r["grad"] + b["grad"], 3, L, H)
    if "grad_e" in r:
        errs["grad_e"] = _block_rel_l2(got["grads_e"], r["grad_e"], 1, 4, 40)
    print("[tile loops] %s N=%d: %s" % (tag, n, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k in [k for k in errs if k.startswith("eq")]:
        assert errs[k] <= bar["eq"], (k, errs[k])
    for k in ("sums", "loss", "grad"):
        assert errs[k] <= bar[k], (k, errs[k])
    if "grad_e" in errs:
        assert errs["grad_e"] <= bar["grad"], ("grad_e", errs["grad_e"])


def _net(L, H, seed, n_out=3):
    return ar.flat_params(ar.seeded_net(n_out, L, H, seed=seed)).numpy().copy()


def _points(n, seed, lo=0.0, hi=1.0):
    rng = np.random.RandomState(seed)
    return ((lo + (hi - lo) * rng.rand(n)).astype(np.float32), (lo + (hi - lo) * rng.rand(n)).astype(np.float32), rng)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,sched,names", [
    ("bf16x3", "2", ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")),
    ("bf16x3", "0", ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")),
    ("fp32", "2", ("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel")),
])
def test_6x256_loops_vs_oracle(monkeypatch, prec, sched, names):
    """The headline shape: role-split sweeps with layer 0 recomputed by dw_bf16 and the 24-bit spill (default), the
    8-wave bf16 kernels ($PINN_SCHED=0), and fp32's 64-column 8-wave kernels - the same points and one oracle run."""
    L, H, Re = 6, 256, 2000.0
    n = pick_n(_cus(), *CASE_FAMILIES["6x256"])
    flat = _net(L, H, 1234)
    x, y, _ = _points(n, 11)
    ref = _oracle("6x256", L, H, flat, x, y, Re)
    got = _case(monkeypatch, L, H, prec, flat, x, y, Re, names, env=(("PINN_SCHED", sched),))
    _compare("6x256 %s sched %s" % (prec, sched), got, ref, prec, L, H)


@pytest.mark.gpu
def test_config4_shape_ev_loops_vs_oracle(monkeypatch):
    """Config 4's shape: 6x256 main net + 4x40 entropy net (trainable), per-point weights, coord_scale 2, bf16x3."""
    L, H, Re = 6, 256, 4000.0
    n = pick_n(_cus(), [SPLIT_256], L)
    flat, flat_e = _net(L, H, 21), _net(4, 40, 22, n_out=1)
    x, y, rng = _points(n, 12, -1.0, 1.0)
    w = (0.3 + rng.rand(n)).astype(np.float32)
    got = _case(monkeypatch, L, H, "bf16x3", flat, x, y, Re, ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel"),
                flat_e=flat_e, w=w, scale=2.0)
    Pe = fr.unflatten(flat_e.astype(np.float64), 2, 1, 4, 40)
    e, _ = fr.forward1(Pe, x.astype(np.float64), y.astype(np.float64))
    # (the entropy net runs in bf16x3 too: its output carries that mode's field error)
    assert _rel_max(got["vtm0"], 0.05 * np.abs(e[:, 0])) <= BARS["bf16x3"]["eq"]
    vis_t = np.minimum(np.float32(20.0 / Re), got["vtm0"])
    np.testing.assert_allclose(got["vis_t"], vis_t, rtol=1e-6)
    ref = _oracle("config4", L, H, flat, x, y, Re, vis_t=vis_t, w=w.astype(np.float64), scale=2.0, params_e=Pe)
    _compare("6x256+4x40 ev", got, ref, "bf16x3", L, H)


@pytest.mark.gpu
@pytest.mark.parametrize("wsplit,names", [
    ("1", ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")),
    ("0", ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel")),
])
def test_wide_4x400_loops_vs_oracle(monkeypatch, wsplit, names):
    """The wide role-split sweeps (16-point tiles, pairs) and the 8-wave wide kernels they replace, same points."""
    L, H, Re = 4, 400, 1500.0
    n = pick_n(_cus(), *CASE_FAMILIES["4x400"])
    flat = _net(L, H, 31)
    x, y, _ = _points(n, 13)
    ref = _oracle("4x400", L, H, flat, x, y, Re)
    got = _case(monkeypatch, L, H, "bf16x3", flat, x, y, Re, names, env=(("PINN_WSPLIT", wsplit),))
    _compare("4x400 wsplit %s" % wsplit, got, ref, "bf16x3", L, H)


@pytest.mark.gpu
def test_config5_shape_ev_loops_vs_oracle(monkeypatch):
    """Config 5's shape: 8x400 main net (wide role-split sweeps, dw_bf16_wide) + 4x40 entropy net, bf16x3."""
    L, H, Re = 8, 400, 10000.0
    n = pick_n(_cus(), *CASE_FAMILIES["8x400"])
    flat, flat_e = _net(L, H, 41), _net(4, 40, 42, n_out=1)
    x, y, _ = _points(n, 14)
    got = _case(monkeypatch, L, H, "bf16x3", flat, x, y, Re,
                ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel"), flat_e=flat_e)
    Pe = fr.unflatten(flat_e.astype(np.float64), 2, 1, 4, 40)
    vis_t = np.minimum(np.float32(20.0 / Re), got["vtm0"])
    np.testing.assert_allclose(got["vis_t"], vis_t, rtol=1e-6)
    ref = _oracle("config5", L, H, flat, x, y, Re, vis_t=vis_t, params_e=Pe)
    _compare("8x400+4x40 ev", got, ref, "bf16x3", L, H)


@pytest.mark.gpu
@pytest.mark.parametrize("case,prec,names", [
    ("4x50", "bf16x3", ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")),
    ("6x128", "fp32", ("fwd_kernel", "bwd_kernel", "dw_kernel")),
])
def test_narrow_nets_loops_vs_oracle(monkeypatch, case, prec, names):
    """Configs 1 and 2: several workgroups per CU, so the 8-wave grid is a multiple of the CU count."""
    L, H = (int(v) for v in case.split("x"))
    Re = 100.0
    n = pick_n(_cus(), *CASE_FAMILIES[case])
    flat = _net(L, H, 50 + L)
    x, y, _ = _points(n, 15)
    ref = _oracle(case, L, H, flat, x, y, Re)
    got = _case(monkeypatch, L, H, prec, flat, x, y, Re, names)
    _compare("%s %s" % (case, prec), got, ref, prec, L, H)
