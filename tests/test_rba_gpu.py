"""GPU tests of the residual-based attention weights on the collocation points: pinn_rba_stats,
pinn_rba_apply and pinn_rba_fill against the fp64 model of tests/rba_model.py, the engine with the feature against an
engine without it that is handed the effective weights (bitwise: the feature changes nothing but w), graph replay
against eager (bitwise: the weights keep evolving inside the graph) and mini-batching of the ev flavour."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import batch_model as bm  # noqa: E402
import fold_model as fm  # noqa: E402
import rba_model as rm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# 1; not a multiple of 4; not a multiple of the block (256 threads x 4 points) nor of 4 x 64 lanes; one block exactly;
# and more than 512 blocks' worth of points: the grid-stride loop repeats and the fold has two partials per thread
SIZES = [1, 7, 1003, 1024, 70001, 600013]


def _planes(n, seed, scale=1.0):
    """A stand-in for an evaluated ResidualPlan: random field planes [FLD_COUNT, npad], the padding poisoned."""
    from nsfnet_amd import engine as eng
    npad = (n + 31) // 32 * 32
    rng = np.random.RandomState(seed)
    f = (rng.randn(eng.FLD_COUNT, npad) * scale * 10.0 ** rng.uniform(-3, 1, size=(1, npad))).astype(np.float32)
    f[:, n:] = np.nan                                   # nothing past n may be read into a result
    plan = SimpleNamespace(n=n, npad=npad, fields=torch.tensor(f, device=DEV))
    return plan, f[eng.FLD["eq1"]:eng.FLD["eq4"] + 1, :n]


def _ulps(a, b):
    """Distance in fp32 ulps between two arrays of non-negative floats."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _indices(kind, n, n_store):
    if kind == "ascending":                             # what pinn_batch_draw writes
        return bm.draw(n_store, n, 3, 5, 0)
    j = np.arange(n, dtype=np.int64)                    # strided, descending
    return n_store - 1 - 2 * j


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("w4", [0.0, 0.1])
def test_stats_match_the_model(n, w4):
    from nsfnet_amd import engine as eng
    plan, eq = _planes(n, seed=n)
    scratch = eng.rba_scratch(n, DEV)
    runs = []
    for _ in range(2):
        eng.rba_stats(plan, w4, scratch)
        torch.cuda.synchronize()
        runs.append(scratch[:8].cpu().numpy().copy())
    np.testing.assert_array_equal(runs[0].view(np.int64), runs[1].view(np.int64))      # the tickets are 0 again, same bits
    rmax, sums = rm.stats(eq, w4)
    got = runs[0]
    assert got[0] == rmax, (got[0], rmax)               # the max is exact
    for k in range(4):
        print("n=%d w4=%s sum%d rel err %.3e" % (n, w4, k + 1, abs(got[1 + k] - sums[k]) / max(sums[k], 1e-300)))
        assert abs(got[1 + k] - sums[k]) <= 1e-12 * sums[k], (k, got[1 + k], sums[k])
    assert got[5] == 0.0 and got[6] == 0.0
    if w4 == 0.0:
        assert got[4] == 0.0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("w4", [0.0, 0.1])
def test_stats_equal_the_fold_model_bit_for_bit(n, w4):
    """rmax and the four sums are the folds of csrc/fixed_fold.h in their fixed order (256 threads x 4 points per block,
    at most 512 blocks): equal to tests/fold_model.py bit for bit, not merely close."""
    from nsfnet_amd import engine as eng
    plan, eq = _planes(n, seed=n)
    scratch = eng.rba_scratch(n, DEV)
    eng.rba_stats(plan, w4, scratch)
    torch.cuda.synchronize()
    got = scratch[:5].cpu().numpy()
    nblk = min(-(-n // 1024), 512)
    q = eq.astype(np.float64)
    want = [fm.grid_fold(rm.norms(eq, w4), nblk, fm.NANMAX)]
    want += [fm.grid_fold(q[k] * q[k], nblk) if k < 3 or w4 != 0.0 else 0.0 for k in range(4)]
    print("n=%d w4=%s device %r model %r" % (n, w4, got.tolist(), want))
    assert fm.same_bits(got, want), (got, want)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", [None, "ascending", "strided"])
@pytest.mark.parametrize("with_s,w4", [(False, 0.0), (True, 0.1), (True, 0.0), (False, 0.1)])
def test_apply_matches_the_model(n, kind, with_s, w4):
    from nsfnet_amd import engine as eng
    gamma, eta = 0.999, 0.01
    plan, eq = _planes(n, seed=n + 1)
    n_store = n if kind is None else 2 * n + 3
    rng = np.random.RandomState(n + 2)
    s = (0.2 + rng.rand(n_store)).astype(np.float32) if with_s else None
    lam0 = (rng.rand(n_store) * 10).astype(np.float32)
    w0 = rm.weights(s, lam0)
    idx = None if kind is None else _indices(kind, n, n_store)
    if kind == "strided" and n > 4:
        idx[1], idx[-1] = -5, n_store                   # outside [0, n_store): skipped
    rec0 = np.zeros(rm.RECORD); rec0[rm.R_UPDATES], rec0[rm.R_SKIPPED] = 3, 2
    dev = lambda a, dt=None: None if a is None else torch.tensor(a, dtype=dt, device=DEV)
    outs = []
    for _ in range(2):
        lam, w, rec = dev(lam0), dev(w0), dev(rec0)
        scratch = eng.rba_scratch(n, DEV)
        eng.rba_stats(plan, w4, scratch)
        eng.rba_apply(plan, w4, gamma, eta, dev(idx), dev(s), lam, w, scratch, rec)
        torch.cuda.synchronize()
        outs.append((lam.cpu().numpy(), w.cpu().numpy(), rec.cpu().numpy(), scratch[:8].cpu().numpy()))
    for a, b in zip(*outs):                             # two identical calls: identical bits
        np.testing.assert_array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                      b.view(np.int32 if b.dtype == np.float32 else np.int64))
    lam, w, rec, scratch = outs[0]
    mlam, mw, mrec = rm.apply(eq, w4, gamma, eta, lam0, s, idx, w=w0, record=rec0)
    touched = np.flatnonzero(mlam.view(np.int32) != lam0.view(np.int32))
    rest = np.setdiff1d(np.arange(n_store), touched)
    np.testing.assert_array_equal(lam[rest], lam0[rest])            # nothing else of the store is written
    np.testing.assert_array_equal(w[rest], w0[rest])
    print("n=%d idx=%s s=%s w4=%s max ulps lam %d w %d" % (n, kind, with_s, w4, _ulps(lam, mlam).max(),
                                                          _ulps(w, mw).max()))
    assert _ulps(lam, mlam).max() <= 1 and _ulps(w, mw).max() <= 1
    assert rec[rm.R_RMAX] == mrec[rm.R_RMAX] == scratch[0]
    np.testing.assert_allclose(rec[rm.R_SUMS:rm.R_SUMS + 4], mrec[rm.R_SUMS:rm.R_SUMS + 4], rtol=1e-12)
    assert rec[rm.R_COUNT] == mrec[rm.R_COUNT] and rec[rm.R_UPDATES] == 4 and rec[rm.R_SKIPPED] == 2
    if _ulps(lam, mlam).max() == 0:
        assert rec[rm.R_MIN] == mrec[rm.R_MIN] and rec[rm.R_MAX] == mrec[rm.R_MAX]
    np.testing.assert_allclose(rec[rm.R_SUM], mrec[rm.R_SUM], rtol=1e-12)
    assert scratch[5] == 0.0 and scratch[6] == 0.0


@pytest.mark.parametrize("n", [1, 1003, 70001])
@pytest.mark.parametrize("with_s", [False, True])
def test_fill_matches_the_model(n, with_s):
    from nsfnet_amd import engine as eng
    s = (0.2 + np.random.RandomState(n).rand(n)).astype(np.float32) if with_s else None
    lam = torch.full((n,), -1.0, device=DEV)
    w = torch.full((n,), -1.0, device=DEV)
    eng.rba_fill(1.7, None if s is None else torch.tensor(s, device=DEV), lam, w)
    torch.cuda.synchronize()
    mlam, mw = rm.fill(n, 1.7, s)
    np.testing.assert_array_equal(lam.cpu().numpy(), mlam)
    np.testing.assert_array_equal(w.cpu().numpy(), mw)


@pytest.mark.parametrize("n", [1003, 600013])
@pytest.mark.parametrize("bad", ["nan", "zero", "inf"])
def test_a_nan_or_all_zero_residual_leaves_lam_and_w_bitwise_unchanged(n, bad):
    from nsfnet_amd import engine as eng
    plan, eq = _planes(n, seed=9)
    E1 = eng.FLD["eq1"]
    if bad == "zero":
        plan.fields[E1:E1 + 4, :n] = 0.0
    else:
        plan.fields[E1 + 1, n // 2] = float(bad)                    # one planted value
    rng = np.random.RandomState(1)
    s = torch.tensor((0.2 + rng.rand(n)).astype(np.float32), device=DEV)
    lam = torch.tensor((rng.rand(n) * 3).astype(np.float32), device=DEV)
    w = torch.tensor(rng.rand(n).astype(np.float32), device=DEV)
    lam0, w0 = lam.clone(), w.clone()
    rec = torch.zeros(rm.RECORD, dtype=torch.float64, device=DEV)
    scratch = eng.rba_scratch(n, DEV)
    for k in range(2):
        eng.rba_stats(plan, 0.1, scratch)
        eng.rba_apply(plan, 0.1, 0.9, 0.1, None, s, lam, w, scratch, rec)
        torch.cuda.synchronize()
        assert torch.equal(lam.view(torch.int32), lam0.view(torch.int32))
        assert torch.equal(w.view(torch.int32), w0.view(torch.int32))
        r = rec.cpu().numpy()
        assert r[rm.R_SKIPPED] == k + 1 and r[rm.R_UPDATES] == 0
        assert {"nan": np.isnan(r[0]), "zero": r[0] == 0.0, "inf": np.isinf(r[0])}[bad]
    if bad == "nan":        # the positive quiet NaN: the multi-rank MAX of the int64 bytes propagates it
        assert int(scratch[:1].view(torch.int64).item()) == 0x7FF8000000000000


def test_c_abi_refuses_bad_arguments():
    from nsfnet_amd import _lib
    lib = _lib.load()
    assert lib.pinn_abi_version() == 3
    plan, _ = _planes(10, 0)
    lam = torch.ones(16, device=DEV)
    w = torch.ones(16, device=DEV)
    scratch = torch.zeros(lib.pinn_rba_scratch_bytes(10) // 8, dtype=torch.float64, device=DEV)
    rec = torch.zeros(rm.RECORD, dtype=torch.float64, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    base = dict(n=10, npad=plan.npad, gamma=0.9, eta=0.1, n_store=10, lam=p(lam), w=p(w))

    def call(**kw):
        a = dict(base, **kw)
        return lib.pinn_rba_apply(a["n"], p(plan.fields), a["npad"], 0.1, a["gamma"], a["eta"], None, a["n_store"], None,
                                  a["lam"], a["w"], p(scratch), p(rec), None)

    assert call(n_store=9) != 0                         # identity needs n <= n_store
    assert call(gamma=0.0) != 0 and call(gamma=1.5) != 0 and call(eta=-1.0) != 0
    assert call(npad=10) != 0 and call(npad=8) != 0
    assert call(lam=p(lam) + 4) != 0 and call(w=p(lam)) != 0
    assert lib.pinn_rba_stats(10, p(plan.fields) + 4, plan.npad, 0.1, p(scratch), None) != 0
    torch.cuda.synchronize()
    assert torch.equal(lam, torch.ones_like(lam)) and float(rec.abs().sum()) == 0.0
    assert call() == 0                                  # scratch is still zero: rmax = 0, a skipped update
    assert lib.pinn_rba_stats(10, p(plan.fields), plan.npad, 0.1, p(scratch), None) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert float(rec[rm.R_SKIPPED]) == 1.0 and float(rec[rm.R_UPDATES]) == 1.0


# ---------------------------------------------------------------- engines
def _bc(every=16):
    return tuple(a.reshape(-1)[::every].astype(np.float32) for a in ar.cavity_boundary())


def _points(n, seed=5):
    rng = np.random.RandomState(seed)
    return (rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32), (0.5 + rng.rand(n)).astype(np.float32))


def _engine(flavour, L, H, prec, x, y, w, seed=5):
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=2, hidden_e=24, alpha_evm=0.05) if flavour == "ev" else {}
    E = eng.PinnEngine(DEV, L, H, 2000.0, alpha_b=10.0, alpha_e=1.0, precision=prec, **ev)
    E.net.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().copy()))
    if flavour == "ev":
        E.net_e.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(1, 2, 24, seed=seed + 1)).numpy().copy()))
    E.set_collocation(x, y, weights=w)
    E.set_boundary(*_bc())
    return E


def _state(E):
    torch.cuda.synchronize()
    out = [E.net.params, E.net.m, E.net.v]
    if E.net_e is not None:
        out += [E.net_e.params, E.net_e.m, E.net_e.v, E.plan_f.vis_t_minus]
    return [t.cpu().numpy().copy() for t in out]


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
@pytest.mark.parametrize("L,H,prec", [(3, 24, "fp32"), (3, 24, "bf16x3"), (6, 256, "fp32"), (6, 256, "bf16x3")])
def test_the_feature_changes_nothing_but_w_bitwise(flavour, L, H, prec, monkeypatch):
    """Step k of an engine with the feature against an engine without it that was handed the effective weights
    s lam_{k-1}^2 (read back from the device): gradient, loss sums and post-Adam state agree bit for bit; lam and w
    follow the model applied to the residual planes each step published."""
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    N, eta, gamma = 2000, 0.3, 0.9
    x, y, w = _points(N)
    s = w if flavour == "ev" else None                   # SDF weights: the ev flavour
    E = _engine(flavour, L, H, prec, x, y, s)
    R = _engine(flavour, L, H, prec, x, y, np.ones(N, np.float32))
    if (H, prec) == (256, "bf16x3"):
        assert E.plan_f.kernel_names()[0] == "fwd_split_kernel"       # the default role-split fused path
    E.set_residual_attention(eta, gamma)
    lam, mw = rm.fill(N, 1.0, s)
    w4 = E.eq4_weight if flavour == "ev" else 0.0
    from nsfnet_amd import engine as eng
    for k in range(5):
        E.e_trainable = R.e_trainable = flavour == "ev" and k == 2
        torch.cuda.synchronize()
        np.testing.assert_array_equal(E.attention().cpu().numpy(), lam)
        assert _ulps(E.plan_f.w.cpu().numpy(), rm.weights(s, lam)).max() <= 1
        R.plan_f.w.copy_(E.plan_f.w)                    # s lam_{k-1}^2, read back
        E.loss_and_grad(); R.loss_and_grad()
        torch.cuda.synchronize()
        assert torch.equal(E.grads, R.grads) and torch.equal(E.grads_e, R.grads_e) and torch.equal(E.sums, R.sums)
        eq = E.plan_f.fields[eng.FLD["eq1"]:eng.FLD["eq4"] + 1, :N].cpu().numpy()
        assert torch.equal(E.plan_f.fields[:, :N], R.plan_f.fields[:, :N])
        new, mw, _ = rm.apply(eq, w4, gamma, eta, lam, s)
        got = E.attention().cpu().numpy()
        assert _ulps(got, new).max() <= 1
        lam = got                                        # carry the device's lam: the bound is per update
        E.adam_step(1e-3); R.adam_step(1e-3)
        for a, b in zip(_state(E), _state(R)):
            np.testing.assert_array_equal(a, b)
    info = E.attention_info()
    assert info["updates"] == 5 and info["skipped"] == 0
    assert info["lam_min"] == float(lam.min()) and info["lam_max"] == float(lam.max())
    assert 0.0 < info["lam_min"] < info["lam_max"] <= rm.bound(1.0, gamma, eta) * (1 + 1e-6)
    q = eq.astype(np.float64)
    np.testing.assert_allclose(info["loss_eq1"], np.sum(q[0] ** 2) / N, rtol=1e-12)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
@pytest.mark.parametrize("L,H,prec", [(3, 24, "fp32"), (6, 256, "bf16x3")])
def test_graph_replay_is_bit_identical_to_eager(flavour, L, H, prec, monkeypatch):
    """One eager step (the capture) and five replayed ones against six eager steps: the weights keep evolving inside
    the graph, all state being device memory."""
    N = 2000
    x, y, w = _points(N)

    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E = _engine(flavour, L, H, prec, x, y, w if flavour == "ev" else None)
        E.set_residual_attention(0.3, 0.9)
        lams = []
        for _ in range(6):
            E.step(1e-3)
            torch.cuda.synchronize()
            lams.append(E.attention().cpu().numpy().copy())
        assert len(E._graphs) == (1 if graph else 0)
        assert E.attention_info()["updates"] == 6
        return _state(E) + lams + [E.plan_f.w.cpu().numpy().copy()]

    eager, graph = run(False), run(True)
    for a, b in zip(eager, graph):
        np.testing.assert_array_equal(a, b)
    lams = eager[-7:-1]
    assert all((lams[k] != lams[k + 1]).any() for k in range(5))


def test_batching_ev_updates_exactly_the_drawn_points(monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    N, B, eta, gamma = 2000, 384, 0.3, 0.9
    x, y, w = _points(N)
    E = _engine("ev", 3, 24, "fp32", x, y, w)
    E.set_batching(B, seed=11)
    E.set_residual_attention(eta, gamma)
    from nsfnet_amd import engine as eng
    for t in range(3):
        torch.cuda.synchronize()
        lam0, w0, vtm0 = E.attention().clone(), E.plan_f.w.clone(), E.plan_f.vis_t_minus.clone()
        E.step(1e-3)
        torch.cuda.synchronize()
        idx = E.batch_indices()
        np.testing.assert_array_equal(idx.cpu().numpy(), bm.draw(N, B, t, 11, 0))
        changed = torch.nonzero(E.attention() != lam0).reshape(-1)
        assert torch.equal(changed, idx)                 # exactly the drawn points
        f, _ = E.eval_plans()
        assert torch.equal(f.w, w0[idx])                 # the batch ran on the weights from before its update
        eq = f.fields[eng.FLD["eq1"]:eng.FLD["eq4"] + 1, :B].cpu().numpy()
        new, mw, _ = rm.apply(eq, E.eq4_weight, gamma, eta, lam0.cpu().numpy(), w, idx.cpu().numpy())
        assert _ulps(E.attention().cpu().numpy(), new).max() <= 1
        assert E.attention_info()["rmax"] == rm.stats(eq, E.eq4_weight)[0]       # the batch's
        rest = torch.ones(N, dtype=torch.bool, device=DEV)
        rest[idx] = False
        assert torch.equal(E.plan_f.vis_t_minus[rest], vtm0[rest])              # the scatter still works
        assert torch.equal(E.plan_f.vis_t_minus[idx], f.vis_t_minus)
        assert torch.equal(E.plan_f.w[rest], w0[rest])
