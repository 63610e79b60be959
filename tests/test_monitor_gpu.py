"""GPU tests of the convergence monitor: pinn_monitor_vis_stats and pinn_monitor_observe against
the fp64 model of tests/monitor_model.py bit for bit, the engine's ring against the model evaluated on the sums and
vis_t bits read after each step and against loss_terms(), the engine with the monitor against a twin without it
(observe-only, bitwise), graph replay in a fresh child process against eager (bitwise), the end-to-end stop of a stage
whose loss is constant, a NaN weight, the checkpoint continuation on the device and the refusals."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fold_model as fm  # noqa: E402
import monitor_model as mm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LR = 1e-3


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


# ---------------------------------------------------------------- the kernels through the C ABI
# monitor.hip has ptime.hip's geometry (256 threads x 4 entries per block, at most 512 blocks): 1; less than a quad; one
# short of a block and one past it (a second block with a ragged quad); and more than 512 blocks' worth, so that the
# grid-stride loop repeats and ends in a ragged quad
VIS_SIZES = [1, 3, 1023, 1025, 512 * 1024 + 1029]
VIS_T0 = np.float32(20.0 / 3000.0)


def _vis_plane(n, seed, special=False):
    rng = np.random.RandomState(seed)
    v = (rng.rand(n) * 1.5 * VIS_T0).astype(np.float32)
    v = np.minimum(v, VIS_T0)                           # about a third of the entries sit on the cap, as in training
    if special:
        v[n // 3] = np.nan
        v[n // 2] = VIS_T0
    return v


def _run_vis(v):
    from nsfnet_amd import engine as eng
    plane = torch.tensor(v, device=DEV)                 # exactly n entries: nothing past them may be read
    sums = torch.full((8,), -7.0, dtype=torch.float32, device=DEV)
    info = torch.zeros(eng.MON_INFO, dtype=torch.float64, device=DEV)
    scratch = eng.monitor_scratch(DEV)
    for _ in range(2):                                  # the second launch finds the ticket word at 0 again
        eng.monitor_vis_stats(plane, v.size, float(VIS_T0), sums[eng.MON_VIS_SLOT:], info, scratch)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), info.cpu().numpy(), scratch.cpu().numpy()


@pytest.mark.parametrize("n", VIS_SIZES)
def test_vis_stats_equal_the_model_bit_for_bit(n):
    v = _vis_plane(n, n)
    sums, info, scratch = _run_vis(v)
    slot, want = mm.vis_stats(v, VIS_T0)
    print("n", n, "slot", sums[4], slot, "info", info, want)
    assert _bits(sums[4:5])[0] == _bits(np.array([slot], np.float32))[0]
    assert fm.same_bits(info, want)
    assert (sums[[0, 1, 2, 3, 5, 6, 7]] == -7.0).all() and scratch[0] == 0.0      # one slot written; the ticket is back at 0
    assert info[1] == np.sum(v >= VIS_T0) > 0 or n < 8


def test_vis_stats_with_a_nan_and_an_entry_on_the_cap():
    n = 1025
    v = _vis_plane(n, 7, special=True)
    v[v == VIS_T0] = np.float32(0.5) * VIS_T0           # the one entry equal to vis_t0 is the one written below
    v[n // 2] = VIS_T0
    sums, info, _ = _run_vis(v)
    slot, want = mm.vis_stats(v, VIS_T0)
    assert np.isnan(sums[4]) and np.isnan(slot) and fm.same_bits(info, want)
    assert np.isnan(info[0]) and info[1] == 1.0 and np.isnan(info[2]) and info[3] == n       # >= counts the equal entry


def _scripted_sums(updates, seed):
    """[updates, 24] fp32 loss sums with a decay, a stretch of zeros (a zero previous window mean), a plateau and one
    non-finite row; [updates, 2] balancing weights."""
    rng = np.random.RandomState(seed)
    s = np.zeros((updates, 24), dtype=np.float32)
    scale = np.concatenate([0.8 ** np.arange(12), np.zeros(12), np.full(updates - 24, 0.05)])
    s[:, 0:4] = (rng.rand(updates, 4) + 0.5) * scale[:, None] * 300.0
    s[:, 4] = (rng.rand(updates) * 0.2 + 1.0) * 2.0
    s[:, 8:10] = (rng.rand(updates, 2) + 0.5) * scale[:, None] * 40.0
    s[:, 16:19] = (rng.rand(updates, 3) + 0.5) * scale[:, None] * 9.0
    s[30, 1] = np.inf
    lam = (rng.rand(updates, 2) * 5.0 + 1.0).astype(np.float32)
    return s, lam


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("with_lam", [False, True])
def test_forty_observations_equal_the_model_bit_for_bit(every, with_lam):
    from nsfnet_amd import engine as eng
    updates, cap = 40, 16
    s, lam = _scripted_sums(updates, 11 + every)
    mon = eng._Monitor(every, 4, 1e-3, 2, 0.05, 0, "loss", "any", cap)
    cfg = mm.Config(every=every, window=4, min_rel_improvement=1e-3, patience=2, re_eff_tol=0.05, capacity=cap, ev=True)
    ds, dl = torch.tensor(s, device=DEV), torch.tensor(lam, device=DEV)
    state = torch.zeros(eng.MON_STATE, dtype=torch.float64, device=DEV)
    ring = torch.zeros(cap, eng.MON_RECORD, dtype=torch.float64, device=DEV)
    st, rg = mm.new_state(), mm.new_ring(cfg)
    consts = dict(alpha_b=10.0, alpha_s=0.5, alpha_e=2.0, w4=0.1, n_eq=1000.0, n_b=129.0, n_s=37.0, n_p=29.0, Re=3000.0)
    for k in range(updates):
        eng.monitor_observe(ds[k, 0:8], ds[k, 8:16], ds[k, 16:24], dl[k] if with_lam else None, consts["alpha_b"],
                            consts["alpha_s"], consts["alpha_e"], consts["w4"], consts["n_eq"], consts["n_b"],
                            consts["n_s"], consts["n_p"], consts["Re"], mon.c_struct(True), state, ring)
        mm.observe(cfg, st, rg, s[k, 0:8], s[k, 8:16], s[k, 16:24], lam[k] if with_lam else None, **consts)
    torch.cuda.synchronize()
    got_st, got_rg = state.cpu().numpy(), ring.cpu().numpy()
    print("state", got_st, "model", st)
    assert fm.same_bits(got_st, st) and fm.same_bits(got_rg, rg)
    assert st[mm.S_UPDATES] == updates and st[mm.S_OBS] == updates // every
    if every == 1:      # what the script was written to reach: a zero previous mean, the non-finite row, both bits
        assert st[mm.S_NONFINITE] == 1.0 and st[mm.S_T_NONFINITE] == 31.0 and int(st[mm.S_STOP]) == 7
        assert st[mm.S_T_PLATEAU] > 0 and st[mm.S_T_RE_EFF] > 0 and st[mm.S_OBS] > cap      # and the ring wrapped


# ---------------------------------------------------------------- engines
def _bc(every=16):
    return tuple(a.reshape(-1)[::every].astype(np.float32) for a in ar.cavity_boundary())


def _points(n, seed=5):
    rng = np.random.RandomState(seed)
    return rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32), (0.5 + rng.rand(n)).astype(np.float32)


def _engine(flavour="ev", seed=5, after=None, n=1000):
    """4 x 50 main net, 4 x 40 entropy net, 1000 collocation points, the boundary's every 16th point, fp32."""
    from nsfnet_amd import engine as eng
    x, y, w = _points(n)
    ev = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05) if flavour == "ev" else {}
    E = eng.PinnEngine(DEV, 4, 50, 3000.0, alpha_b=10.0, alpha_e=1.0, precision="fp32", **ev)
    E.net.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(3, 4, 50, seed=seed)).numpy().copy()))
    if flavour == "ev":
        E.net_e.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(1, 4, 40, seed=seed + 1)).numpy().copy()))
    E.set_collocation(x, y, weights=w if flavour == "ev" else None)
    E.set_boundary(*_bc())
    if after is not None:
        after(E)
    return E


def _state(E):
    torch.cuda.synchronize()
    out = [E.net.params, E.net.m, E.net.v]
    if E.net_e is not None:
        out += [E.net_e.params, E.net_e.m, E.net_e.v, E.plan_f.vis_t_minus]
    return [t.cpu().numpy().copy() for t in out]


def test_every_ring_row_is_the_model_on_the_bits_read_after_the_step(monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    E = _engine("ev")
    E.set_convergence_monitor(window=4, patience=2, re_eff_tol=1e-3, history=32)
    cfg = mm.Config(window=4, patience=2, re_eff_tol=1e-3, capacity=32, ev=True)
    st, rg = mm.new_state(), mm.new_ring(cfg)
    n_b = E.n_b_global
    # loss_terms() makes each term in fp32 from the same sums, all positive: along the longest chain a division, three
    # additions, the product with alpha_e and two more additions - seven roundings of half an ulp (2^-24 relative) each -
    # and the eq4 weight 0.1 is an fp32 constant there (2^-26 off the double the row uses): eight bound the distance
    tol = 8 * 2.0 ** -24
    for k in range(30):
        if k == 12:
            E.e_trainable = True                        # both nets move for a while, as where the ev schedule unfreezes
        if k == 14:
            E.e_trainable = False
        E.step(LR)
        s = E.sums.cpu().numpy()
        slot, info = mm.vis_stats(E.plan_f.vis_t.cpu().numpy(), np.float32(E.vis_t0))
        assert _bits(s[4:5])[0] == _bits(np.array([slot], np.float32))[0]
        mm.observe(cfg, st, rg, s[0:8], s[8:16], None, None, 10.0, 0.0, 1.0, 0.1, 1000, n_b, 0, 0, 3000.0)
        row, lt = E.monitor_info()["last"], {k_: float(v) for k_, v in E.loss_terms().items()}
        assert row["t"] == k + 1
        for name in ("loss", "loss_e", "loss_b"):
            assert abs(row[name] - lt[name]) <= tol * abs(row[name]), (k, name, row[name], lt[name])
        for j in range(4):
            assert abs(row["eq%d" % (j + 1)] - lt["loss_eq%d" % (j + 1)]) <= tol * abs(row["eq%d" % (j + 1)])
    torch.cuda.synchronize()
    assert fm.same_bits(E._mon.state.cpu().numpy(), st) and fm.same_bits(E._mon.ring.cpu().numpy(), rg)
    assert fm.same_bits(E._mon.info.cpu().numpy(), info)
    hist = E.monitor_history()
    assert hist.shape == (30, mm.RECORD) and (hist[:, 9] > 0).all() and (hist[:, 10] < 3000.0).all()
    i = E.monitor_info()
    assert i["vis_t_max"] <= np.float32(E.vis_t0) and 0.0 <= i["cap_fraction"] <= 1.0 and i["windows"] == 7


@pytest.mark.parametrize("case", ["plain", "ev", "ev_batch"])
def test_the_monitor_only_observes(case, monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    flavour = "nsfnet" if case == "plain" else "ev"
    batch = (lambda e: e.set_batching(batch_points=256, seed=3)) if case == "ev_batch" else None
    E, R = _engine(flavour, after=batch), _engine(flavour, after=batch)
    E.set_convergence_monitor(window=3, patience=1, re_eff_tol=None if case == "plain" else 1e-2, history=8)
    for k in range(20):
        if k == 7 and flavour == "ev":
            E.e_trainable = R.e_trainable = True
        E.step(LR); R.step(LR)
    for a, b in zip(_state(E), _state(R)):              # the twin without the monitor: the same bits
        np.testing.assert_array_equal(_bits(a), _bits(b))
    i = E.monitor_info()
    assert i["updates"] == i["observations"] == 20 and i["windows"] == 6 and i["nonfinite"] == 0
    if case == "ev_batch":                              # the statistics are the batch plan's
        assert E._mon.info.cpu().numpy()[3] == 256.0
    assert R.monitor_info() is None and float(R.sums[4]) == 0.0


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_monitor_gpu as t
assert t.os.environ["NSFNET_GRAPH"] == "1"
E = t._engine({flavour!r})
E.set_convergence_monitor(every={every}, window=3, patience=1, re_eff_tol={re_tol!r}, history=8)
for _ in range(20):
    E.step(t.LR)
assert len(E._graphs) == 1
np.savez({out!r}, *t._state(E), state=E._mon.state.cpu().numpy(), ring=E._mon.ring.cpu().numpy())
"""


@pytest.mark.parametrize("flavour,every", [("ev", 1), ("nsfnet", 3)])
def test_graph_replay_in_a_fresh_process_is_bit_identical_to_eager(flavour, every, tmp_path, monkeypatch):
    re_tol = 1e-2 if flavour == "ev" else None
    out = str(tmp_path / "graph.npz")
    env = dict(os.environ, NSFNET_GRAPH="1")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), flavour=flavour, every=every, re_tol=re_tol, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    E = _engine(flavour)
    E.set_convergence_monitor(every=every, window=3, patience=1, re_eff_tol=re_tol, history=8)
    for _ in range(20):
        E.step(LR)
    eager = _state(E)
    got = np.load(out)
    for k, a in enumerate(eager):
        np.testing.assert_array_equal(_bits(a), _bits(got["arr_%d" % k]))
    assert fm.same_bits(E._mon.state.cpu().numpy(), got["state"]) and fm.same_bits(E._mon.ring.cpu().numpy(), got["ring"])
    assert got["state"][mm.S_UPDATES] == 20 and got["state"][mm.S_OBS] == 20 // every


def test_a_constant_loss_stops_the_stage_at_the_predicted_update(monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    from nsfnet_amd import pinn_solver as ps
    x, y, _ = _points(1000)
    P = ps.PysicsInformedNeuralNetwork(Re=400.0, layers=4, hidden_size=50, N_f=1000, bc_weight=10.0, eq_weight=1.0)
    P.net.dev_net.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(3, 4, 50, seed=5)).numpy().copy()))
    P.set_boundary_data(X=ar.cavity_boundary())
    P.set_eq_training_data(X=(x, y))
    P.save_every, P.log_every = 0, 10
    P.set_early_stopping(window=5, patience=2, min_rel_improvement=1e-3)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=200, lr=0.0)                  # lr = 0: the weights never move
    i = P.engine.monitor_info()
    hist = P.monitor_history()
    assert len(np.unique(_bits(hist[:, 1]))) == 1 and np.isfinite(hist[0, 1]) and hist[0, 1] > 0    # bit-constant from step 1
    assert i["t_plateau"] == 15 and i["reasons"] == ["plateau"] and i["should_stop"]
    assert list(hist[:, 11]) == [0.0] * 14 + [1.0] * (len(hist) - 14)
    # the log points are epochs 0, 10, 20, ...: the first one after update 15 is epoch 20, the 21st update
    assert i["updates"] == 21 and P.engine.net.adam_t == 21
    assert "early stop after epoch 21: plateau (set by update 15)" in out.getvalue()


def test_a_nan_weight_gives_nonfinite_after_one_update(monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    E = _engine("ev")
    E.set_convergence_monitor(window=5, patience=2, re_eff_tol=1e-3)
    flat = E.net.params.detach().cpu().clone()
    flat[17] = float("nan")
    E.net.set_flat(flat)
    E.step(LR)
    i = E.monitor_info()
    assert i["reasons"] == ["nonfinite"] and i["t_nonfinite"] == 1 and i["nonfinite"] == 1 and i["window_fill"] == 0
    assert E.should_stop() and np.isnan(i["last"]["loss"]) and i["last"]["stop"] == 4.0


def test_k_save_load_k_equals_2k_on_the_device(tmp_path, monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    K = 6
    mon = lambda e: e.set_convergence_monitor(window=2, patience=1, re_eff_tol=0.3, history=8)
    whole = _engine("ev", after=mon)
    for _ in range(2 * K):
        whole.step(LR)
    first = _engine("ev", after=mon)
    for _ in range(K):
        first.step(LR)
    path = str(tmp_path / "state.bin")
    first.save_training_state(path)
    second = _engine("ev", seed=77, after=mon)
    assert second.load_training_state(path)["changed"] == []
    for _ in range(K):
        second.step(LR)
    for a, b in zip(_state(whole), _state(second)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert fm.same_bits(whole._mon.state.cpu().numpy(), second._mon.state.cpu().numpy())
    assert fm.same_bits(whole._mon.ring.cpu().numpy(), second._mon.ring.cpu().numpy())
    assert whole.monitor_info()["updates"] == 2 * K and whole.monitor_history().shape[0] == 8          # the ring wrapped
    assert fm.same_bits(whole.monitor_history(), second.monitor_history())


def test_refusals_raise_by_name():
    E = _engine("nsfnet")
    with pytest.raises(ValueError, match="re_eff_tol needs the ev flavour"):
        E.set_convergence_monitor(re_eff_tol=1e-3)
    E.set_convergence_monitor(window=4)
    with pytest.raises(ValueError, match="convergence monitor needs the MSE loss"):
        E.loss_and_grad(mode="L2")
    x, y, _ = _points(1000)
    with pytest.raises(ValueError, match="convergence monitor needs a resident store"):
        E.set_collocation(x, y, chunk_points=512)
    E.set_convergence_monitor(every=0)
    E.set_collocation(x, y, chunk_points=512)
    with pytest.raises(ValueError, match="convergence monitor needs a resident store"):
        E.set_convergence_monitor(window=4)
