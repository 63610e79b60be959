"""Reynolds-number continuation without a GPU: the host query pinn_visc_schedule_value against the numpy statement of
tests/recont_model.py, the ABI's refusals, the engine's host logic on the model-backed fakes (tests/recont_fakes.py) -
where the launch sits in a step, what holds nu, which plans get the pointers, the refusals, the graph key, the
training-state file -, the YAML key, the solvers, two gloo ranks, and the conditions on the inputs of the ev rows of
tests/test_recont_gpu.py."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fold_model as fm  # noqa: E402
import recont_model as rm  # noqa: E402

L, H, RE, R0, LR = 2, 10, 400.0, 40.0, 1e-3
SHAPE_E = (1, 2, 6)
UPDATES = 1000


def _struct(c):
    from nsfnet_amd import _lib
    return _lib.ViscScheduleStruct(shape=rm.SHAPES[c["shape"]], stairs=c["stairs"], hold=c["hold"], updates=c["updates"],
                                   re_start=c["re_start"], re_end=c["re_end"], cap_factor=c["cap_factor"],
                                   nu_start=c["nu_start"], nu_end=c["nu_end"], cap_start=c["cap_start"], cap_end=c["cap_end"])


# ------------------------------------------------------------------ the schedule on the host
@pytest.mark.parametrize("ends", [(40.0, 400.0), (5.0, 2000.0), (1000.0, 100.0)], ids=["40-400", "5-2000", "1000-100"])
@pytest.mark.parametrize("hold", [0, 7])
@pytest.mark.parametrize("stairs", [0, 1, 4])
@pytest.mark.parametrize("shape", sorted(rm.SHAPES))
def test_schedule_value_is_the_numpy_statement(shape, stairs, hold, ends):
    """Bit for bit for the linear shapes and for every end; geometric within one fp32 ulp (the fp64 exp / log error is
    far below an fp32 ulp: only the final rounding can differ); monotone in t; Re_t between the two ends."""
    from nsfnet_amd import _lib
    lib = _lib.load()
    c = rm.schedule(ends[0], ends[1], UPDATES, hold=hold, shape=shape, stairs=stairs, cap_factor=20.0)
    cs = _struct(c)
    rec = (ctypes.c_double * rm.RECORD)()
    rows = []
    for t in rm.positions(c):
        nu = lib.pinn_visc_schedule_value(ctypes.byref(cs), t, rec)
        got, want = list(rec), rm.value(c, t)
        assert nu == got[3]
        inside = 0.0 < want[1] < 1.0
        if shape == "geometric" and inside:
            assert fm.same_bits(np.array(got[:2] + got[5:]), np.array(want[:2] + want[5:])), (t, got, want)
            for k in (3, 4):
                assert abs(got[k] - want[k]) <= float(np.spacing(np.float32(want[k]))), (t, k, got, want)
            assert abs(got[2] - want[2]) <= 1e-12 * want[2]
        else:
            assert fm.same_bits(np.array(got), np.array(want)), (t, got, want)
        rows.append(got)
    first, last = rows[0], rows[-1]
    assert first[3] == float(np.float32(1.0) / np.float32(ends[0])) and first[4] == float(np.float32(20.0 / ends[0]))
    assert last[3] == float(np.float32(1.0) / np.float32(ends[1])) and last[4] == float(np.float32(20.0 / ends[1]))
    assert rows[1] == [float(hold)] + first[1:] and rows[-2][1:] == last[1:] and last[5] == 1.0 and rows[-3][5] == 0.0
    sign = 1.0 if ends[1] > ends[0] else -1.0
    for a, b in zip(rows, rows[1:]):
        assert sign * (b[2] - a[2]) >= 0.0 and sign * (a[3] - b[3]) >= 0.0 and sign * (a[4] - b[4]) >= 0.0 and b[1] >= a[1]
    for r in rows:
        assert min(ends) <= r[2] <= max(ends)
    if stairs == 0:
        assert rows[2][3] != first[3] and rows[3][3] not in (first[3], last[3])
    if stairs == 1:     # one stair: the start value until the end of the ramp
        assert all(r[3] == first[3] for r in rows[:5])
    # every position of a short ramp, against the model and monotone (no cap: the record's slot stays 0)
    c = rm.schedule(ends[0], ends[1], 12, hold=hold, shape=shape, stairs=stairs)
    cs, prev = _struct(c), None
    for t in range(0, hold + 15):
        lib.pinn_visc_schedule_value(ctypes.byref(cs), t, rec)
        got, want = list(rec), rm.value(c, t)
        assert got[4] == 0.0 and abs(got[3] - want[3]) <= (float(np.spacing(np.float32(want[3]))) if shape == "geometric" else 0.0)
        assert prev is None or sign * (prev - got[3]) >= 0.0
        prev = got[3]


# ------------------------------------------------------------------ the ABI without a device
def test_abi_refuses_bad_arguments_by_name():
    from nsfnet_amd import _lib
    lib = _lib.load()
    assert lib.pinn_abi_version() == 3
    buf = (ctypes.c_double * 16)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)      # aligned host memory: nothing is launched
    odd4, odd2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    good = rm.schedule(40.0, 400.0, 100, cap_factor=20.0)
    for kw, word in ((dict(updates=0), b"updates"), (dict(updates=-3), b"updates"), (dict(hold=-1), b"hold"),
                     (dict(stairs=-1), b"stairs"), (dict(re_start=0.0), b"re_start"), (dict(re_start=-5.0), b"re_start"),
                     (dict(re_start=float("nan")), b"re_start"), (dict(re_start=float("inf")), b"re_start"),
                     (dict(re_end=0.0), b"re_end"), (dict(nu_start=np.float32("inf")), b"nu_start"),
                     (dict(cap_factor=-1.0), b"cap_factor"), (dict(cap_end=np.float32(0.0)), b"cap_start")):
        cs = _struct(dict(good, **kw))
        assert np.isnan(lib.pinn_visc_schedule_value(ctypes.byref(cs), 0, None)), kw
        assert b"pinn_visc_schedule_value" in lib.pinn_last_error() and word in lib.pinn_last_error(), (kw, lib.pinn_last_error())
        assert lib.pinn_visc_schedule_step(ctypes.byref(cs), p, p, p, p, None) == -22 and word in lib.pinn_last_error(), kw
    cs = _struct(dict(good, shape="geometric"))
    cs.shape = 3
    assert np.isnan(lib.pinn_visc_schedule_value(ctypes.byref(cs), 0, None)) and b"shape" in lib.pinn_last_error()
    cs = _struct(good)
    assert np.isnan(lib.pinn_visc_schedule_value(None, 0, None)) and b"null schedule" in lib.pinn_last_error()
    assert np.isnan(lib.pinn_visc_schedule_value(ctypes.byref(cs), -1, None)) and b"t must be" in lib.pinn_last_error()
    assert lib.pinn_visc_schedule_step(ctypes.byref(cs), None, p, p, p, None) == -22 and b"null argument" in lib.pinn_last_error()
    assert lib.pinn_visc_schedule_step(ctypes.byref(cs), p, None, p, p, None) == -22 and b"null argument" in lib.pinn_last_error()
    assert lib.pinn_visc_schedule_step(ctypes.byref(cs), p, p, p, None, None) == -22 and b"null argument" in lib.pinn_last_error()
    for args in ((odd4, p, p, p), (p, odd2, p, p), (p, p, odd2, p), (p, p, p, odd4)):
        assert lib.pinn_visc_schedule_step(ctypes.byref(cs), *args, None) == -22 and b"aligned" in lib.pinn_last_error(), args
    nocap = _struct(rm.schedule(40.0, 400.0, 100))
    assert lib.pinn_visc_schedule_step(ctypes.byref(nocap), p, p, p, p, None) == -22 and b"cap_factor" in lib.pinn_last_error()
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pinn_net_create(3, 2, 8, ctypes.byref(net)) == 0
    try:
        assert lib.pinn_plan_create(net, 69, 1, ctypes.byref(plan)) == 0
        assert lib.pinn_plan_set_viscosity_cap(plan, p) == -22 and b"not a residual" in lib.pinn_last_error()
        lib.pinn_plan_destroy(plan)
        assert lib.pinn_plan_create(net, 69, 4, ctypes.byref(plan)) == 0
        assert lib.pinn_plan_set_viscosity_cap(plan, p) == -22 and b"cap_dev comes with nu_dev" in lib.pinn_last_error()
        assert lib.pinn_plan_set_viscosity(plan, p, None) == 0
        assert lib.pinn_plan_set_viscosity_cap(plan, odd2) == -22 and b"4-byte" in lib.pinn_last_error()
        assert lib.pinn_plan_set_viscosity_cap(plan, odd4) == 0
        a = ctypes.c_void_p()
        assert lib.pinn_plan_viscosity_cap(plan, ctypes.byref(a)) == 0 and a.value == odd4.value
        assert lib.pinn_plan_viscosity_cap(plan, None) == -22
        assert lib.pinn_plan_set_viscosity(plan, None, None) == 0      # nu off takes the cap along
        assert lib.pinn_plan_viscosity_cap(plan, ctypes.byref(a)) == 0 and not a.value
        lib.pinn_plan_destroy(plan)
    finally:
        lib.pinn_net_destroy(net)


# ------------------------------------------------------------------ the engine on the fakes
def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", seed=5, setup=None, attach=True):
    import recont_fakes
    recont_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=SHAPE_E[1], hidden_e=SHAPE_E[2], alpha_evm=0.5) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev)
    rng = np.random.RandomState(seed)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    if attach:
        e.set_collocation(case["x"], case["y"])
        e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    if setup is not None:
        setup(e)
    return e


def _state(e):
    rc = e._rc
    return (int(rc.pos[0]), np.float32(rc.nu.numpy()[0]), None if rc.cap is None else np.float32(rc.cap.numpy()[0]),
            rc.rec.numpy().copy())


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_engine_state_is_the_model_after_every_update(monkeypatch, flavour):
    import recont_fakes
    e = _engine(monkeypatch, _case(), flavour)
    assert e.continuation_info() is None
    e.set_reynolds_continuation(R0, 6, hold=2, shape="linear_re", stairs=3)
    c = rm.schedule(R0, RE, 6, hold=2, shape="linear_re", stairs=3, cap_factor=20.0 if flavour == "ev" else 0.0)
    info = e.continuation_info()
    assert info["t"] == 0 and info["Re_t"] == R0 and info["nu_t"] == float(np.float32(1.0) / np.float32(R0)) and not info["done"]
    assert (info["cap_t"] is None) == (flavour != "ev")
    del recont_fakes.CALLS[:]
    seen = set()
    for k in range(1, 11):
        e.step(LR)
        want = rm.value(c, k)
        t, nu, cap, rec = _state(e)
        assert t == k and fm.same_bits(rec, np.array(want)) and float(nu) == want[3]
        assert cap is None or float(cap) == want[4]
        seen.add(float(nu))
    assert [c_[0] for c_ in recont_fakes.CALLS if c_[0].startswith("visc")] == ["visc_schedule_step"] * 10
    assert len(seen) == 4                                   # the start, two stairs, the end
    info = e.continuation_info()
    assert info["done"] and info["t"] == 10 and info["Re_t"] == RE and info["nu_t"] == float(np.float32(1.0) / np.float32(RE))
    if flavour == "ev":
        assert info["cap_t"] == float(np.float32(e.vis_t0))
        e.loss_and_grad()
        assert float(e.plan_f.vis_t.max()) <= info["cap_t"]
    assert info["shape"] == "linear_re" and info["stairs"] == 3 and info["re_end"] == RE and info["follow_vis_t0"]
    e.reset_reynolds_continuation(5)
    assert fm.same_bits(_state(e)[3], np.array(rm.value(c, 5))) and _state(e)[0] == 5
    e.set_reynolds_continuation(R0, 6)                       # a call restarts the ramp
    assert e.continuation_info()["t"] == 0
    with pytest.raises(ValueError, match="position"):
        e.reset_reynolds_continuation(-1)


def test_the_evaluation_reads_the_scalars_of_the_ramp(monkeypatch):
    """ev flavour: with the scalars inside the ramp the planes are those of the oracle at (nu_t, cap_t), vis_t <= cap_t
    and the cap binds somewhere; follow_vis_t0 False keeps the configured cap."""
    case = _case()
    e = _engine(monkeypatch, case, "ev")
    e.set_reynolds_continuation(R0, 10)
    e.reset_reynolds_continuation(4)
    info = e.continuation_info()
    assert 0.0 < info["s"] < 1.0 and e.vis_t0 < info["cap_t"] < 20.0 / R0
    e.loss_and_grad()
    vt = e.plan_f.vis_t.numpy()
    assert vt.max() == np.float32(info["cap_t"]) and vt.min() < vt.max()
    plain = _engine(monkeypatch, case, "ev")
    plain.Re, plain.vis_t0 = 1.0 / info["nu_t"], info["cap_t"]
    plain.loss_and_grad()
    np.testing.assert_allclose(e.plan_f.field("eq1").numpy(), plain.plan_f.field("eq1").numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(vt, plain.plan_f.vis_t.numpy())
    e.set_reynolds_continuation(R0, 10, follow_vis_t0=False)
    assert e._rc.cap is None and e.plan_f.cap is None and e.continuation_info()["cap_t"] is None
    e.loss_and_grad()
    assert e.plan_f.vis_t.numpy().max() <= np.float32(e.vis_t0)


def test_held_by_lbfgs_and_full_batch_and_off_adds_no_launch(monkeypatch):
    import recont_fakes
    e = _engine(monkeypatch, _case())
    del recont_fakes.CALLS[:]
    e.step(LR)
    off = [c[0] for c in recont_fakes.CALLS]
    assert not [c for c in off if c.startswith("visc")]
    e.set_reynolds_continuation(R0, 8)
    e.set_reynolds_continuation(R0, 8, enabled=False)
    assert e.continuation_info() is None and e.plan_f.nu is None and e.plan_f.cap is None and e.plan_f.lap is None
    del recont_fakes.CALLS[:]
    e.step(LR)
    assert [c[0] for c in recont_fakes.CALLS] == off
    e.set_reynolds_continuation(R0, 8)
    e.step(LR)
    before = _state(e)
    e.lbfgs_step(max_iter=2)
    e.loss_and_grad(full_batch=True)
    e.loss_and_grad()
    after = _state(e)
    assert after[0] == before[0] == 1 and after[1] == before[1] and fm.same_bits(after[3], before[3])
    e.net.reset_adam()                                      # the position is not an optimiser's state
    assert _state(e)[0] == 1
    # a finished ramp switched off leaves a plain engine at Re
    for _ in range(8):
        e.step(LR)
    assert e.continuation_info()["done"]
    e.loss_and_grad()
    eq_on = e.plan_f.field("eq1").numpy().copy()
    e.set_reynolds_continuation(R0, 8, enabled=False)
    e.loss_and_grad()
    np.testing.assert_array_equal(e.plan_f.field("eq1").numpy(), eq_on)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_every_residual_plan_gets_the_pointers_and_no_lap(monkeypatch, flavour):
    case = _case()
    e = _engine(monkeypatch, case, flavour, attach=False)
    e.set_reynolds_continuation(R0, 8)
    e.set_collocation(case["x"], case["y"])
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    e.set_batching(batch_points=35)
    e.set_resample_pool(case["x"][::-1].copy(), case["y"][::-1].copy())
    nu, cap = e._rc.nu, e._rc.cap
    assert (cap is not None) == (flavour == "ev")
    for plan in (e.plan_f, e._batch.f, e._pool):
        assert plan.nu is nu and plan.cap is cap and plan.lap is None
    e.step(LR)
    assert e.continuation_info()["t"] == 1 and e.sums.numpy()[5] == 0.0       # slot 5 stays unused
    e.set_collocation(case["x"], case["y"])
    assert e.plan_f.nu is nu and e._batch.f.nu is nu and e.plan_f.cap is cap and e._batch.f.cap is cap
    # attached after the data, too
    e2 = _engine(monkeypatch, case, flavour)
    e2.set_batching(batch_points=35)
    e2.set_resample_pool(case["x"][::-1].copy(), case["y"][::-1].copy())
    e2.set_reynolds_continuation(R0, 8)
    for plan in (e2.plan_f, e2._batch.f, e2._pool):
        assert plan.nu is e2._rc.nu and plan.cap is e2._rc.cap and plan.lap is None


def test_refusals_name_the_other_option(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    for kw in (dict(re_start=0.0), dict(re_start=float("nan")), dict(re_start=float("inf")), dict(re_start=-3.0),
               dict(updates=0), dict(updates=-2), dict(updates=1.5), dict(hold=-1), dict(stairs=-1), dict(shape="cubic")):
        with pytest.raises(ValueError, match="Reynolds-number continuation"):
            e.set_reynolds_continuation(**dict(dict(re_start=R0, updates=8), **kw))
    assert e.continuation_info() is None
    with pytest.raises(RuntimeError, match="Reynolds-number continuation is off"):
        e.reset_reynolds_continuation()
    e.set_reynolds_continuation(R0, 8)
    with pytest.raises(ValueError, match="convergence monitor is not available with Reynolds-number continuation"):
        e.set_convergence_monitor(window=2)
    with pytest.raises(ValueError, match="viscosity identification is not available with Reynolds-number continuation"):
        e.set_viscosity_identification()
    with pytest.raises(ValueError, match="Reynolds-number continuation needs the MSE loss"):
        e.loss_and_grad(mode="L2")
    with pytest.raises(ValueError, match="Reynolds-number continuation needs a resident store"):
        e.set_collocation(case["x"], case["y"], chunk_points=32)
    e.set_reynolds_continuation(R0, 8, enabled=False)
    e.set_convergence_monitor(window=2)
    with pytest.raises(ValueError, match="Reynolds-number continuation is not available with the convergence monitor"):
        e.set_reynolds_continuation(R0, 8)
    e.set_convergence_monitor(every=0)
    e.set_viscosity_identification()
    with pytest.raises(ValueError, match="Reynolds-number continuation is not available with viscosity identification"):
        e.set_reynolds_continuation(R0, 8)
    e.set_viscosity_identification(enabled=False)
    e.set_collocation(case["x"], case["y"], chunk_points=32)
    with pytest.raises(ValueError, match="Reynolds-number continuation needs a resident store"):
        e.set_reynolds_continuation(R0, 8)
    assert e.continuation_info() is None


def test_the_options_that_need_only_the_pointer_run_with_it(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    e.set_reynolds_continuation(R0, 8)
    e.set_batching(batch_points=35)
    e.set_residual_attention(eta=0.5, gamma=0.9)
    e.set_loss_balancing(every=2)
    for _ in range(4):
        e.step(LR)
    assert e.continuation_info()["t"] == 4
    assert np.isfinite(e.net.params.numpy()).all()      # (conflict-free gradients, pseudo-time: tests/test_recont_gpu.py)


def test_graph_key_carries_the_launch_constants(monkeypatch):
    e = _engine(monkeypatch, _case())
    off = e._graph_key(LR, False)
    e.set_reynolds_continuation(R0, 8)
    on = e._graph_key(LR, False)
    assert on != off and on[:len(off)] == off
    keys = {on}
    for kw in (dict(re_start=50.0), dict(updates=9), dict(hold=1), dict(shape="linear_nu"), dict(stairs=2),
               dict(follow_vis_t0=False)):
        e.set_reynolds_continuation(**dict(dict(re_start=R0, updates=8), **kw))
        keys.add(e._graph_key(LR, False))
    assert len(keys) == 7
    e.set_reynolds_continuation(R0, 8)
    for _ in range(3):
        e.step(LR)
    assert e._graph_key(LR, False) == on                     # the position is device state: one graph serves the ramp
    e.set_reynolds_continuation(R0, 8, enabled=False)
    assert e._graph_key(LR, False) == off


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_state_file_omits_the_segment_when_off_and_round_trips_it(monkeypatch, tmp_path, flavour):
    import state_model as sm
    case = _case()
    never = _engine(monkeypatch, case, flavour)
    toggled = _engine(monkeypatch, case, flavour)
    toggled.set_reynolds_continuation(R0, 8)
    toggled.set_reynolds_continuation(R0, 8, enabled=False)
    for e in (never, toggled):
        for _ in range(3):
            e.step(LR)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    never.save_training_state(a)
    toggled.save_training_state(b)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    header, _ = sm.parse(raw)
    assert "re_continuation" not in header["fingerprint"] and "re_continuation" not in header["info"]
    assert not [s for s in header["segments"] if s["name"].startswith("recont")]
    setup = lambda e: e.set_reynolds_continuation(R0, 12, hold=1, stairs=0)
    K = 4
    whole = _engine(monkeypatch, case, flavour, setup=setup)
    for _ in range(2 * K):
        whole.step(LR)
    first = _engine(monkeypatch, case, flavour, setup=setup)
    for _ in range(K):
        first.step(LR)
    assert 0.0 < first.continuation_info()["s"] < 1.0        # the save falls inside the ramp
    c = str(tmp_path / "c.bin")
    first.save_training_state(c)
    header, _ = sm.parse(open(c, "rb").read())
    assert header["fingerprint"]["re_continuation"] is True
    assert header["info"]["re_continuation"] == [R0, 12, 1, "geometric", 0, True]
    names = ["recont.pos", "recont.nu"] + (["recont.cap"] if flavour == "ev" else []) + ["recont.rec"]
    assert [s["name"] for s in header["segments"] if s["name"].startswith("recont")] == names
    with pytest.raises(ValueError, match="fingerprint key 're_continuation'"):
        never.load_training_state(c)
    second = _engine(monkeypatch, case, flavour, seed=77, setup=setup)
    assert second.load_training_state(c)["changed"] == []
    for x, y in zip(_state(second), _state(first)):
        assert np.array_equal(x, y)
    for _ in range(K):
        second.step(LR)
    assert _state(second)[0] == 2 * K and fm.same_bits(_state(second)[3], _state(whole)[3])
    assert _state(second)[1] == _state(whole)[1] and _state(second)[2] == _state(whole)[2]
    np.testing.assert_array_equal(second.net.params.numpy(), whole.net.params.numpy())


# ------------------------------------------------------------------ the solvers, the YAML key
def _plain(monkeypatch, case):
    import recont_fakes
    recont_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=L, hidden_size=H, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_every, P.save_every = 2, 0
    return P


def _ev(monkeypatch, case):
    import recont_fakes
    recont_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(0)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=L, layers_1=SHAPE_E[1], hidden_size=H, hidden_size_1=SHAPE_E[2],
                                       N_f=70, alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_interval = 2
    return P


@pytest.mark.parametrize("kind", ["plain", "ev"])
def test_solvers_log_re_t_and_do_not_reset_at_a_stage_start(monkeypatch, kind):
    case = _case()
    P = (_plain if kind == "plain" else _ev)(monkeypatch, case)
    assert not P._recont
    P.set_reynolds_continuation(40.0, 10, hold=1)
    assert P._recont
    P.save = lambda *a, **k: None
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.train(num_epoch=4, lr=1e-3)
    assert "Re_t=" in out.getvalue() and "updates=" in out.getvalue()
    assert P.engine.continuation_info()["t"] == 4
    if kind == "ev":
        assert "vis_t0=" in out.getvalue()
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=3, lr=5e-4)                        # the next stage (ev: with a re-created Adam) carries on
    info = P.engine.continuation_info()
    c = rm.schedule(40.0, float(P.Re), 10, hold=1, cap_factor=20.0 if kind == "ev" else 0.0)
    assert info["t"] == 7 and info["nu_t"] == rm.value(c, 7)[3] and 0.0 < info["s"] < 1.0
    opt = torch.optim.LBFGS(P.net.parameters(), lr=1.0, max_iter=1)
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=1, lr=1.0, optimizer=opt)            # held during an L-BFGS stage
    assert P.engine.continuation_info()["t"] == 7
    P.set_reynolds_continuation(40.0, 10, enabled=False)
    assert not P._recont and P.engine.continuation_info() is None


def test_yaml_key_parses_and_is_validated(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_recont", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    cfg = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = cfg
    spec.loader.exec_module(cfg)
    prod = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml"))
    assert prod.config.training.re_continuation is None             # absent: off
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  re_continuation: {re_start: 400, updates: 500000, hold: 1000, shape: linear_re, stairs: 8}\n")
    rc = cfg.ConfigManager.from_file(str(p)).config.training.re_continuation
    assert (rc.re_start, rc.updates, rc.hold, rc.shape, rc.stairs) == (400.0, 500000, 1000, "linear_re", 8)
    p.write_text("training:\n  re_continuation: {re_start: 400, updates: 10}\n")
    rc = cfg.ConfigManager.from_file(str(p)).config.training.re_continuation
    assert (rc.hold, rc.shape, rc.stairs) == (0, "geometric", 0)
    for bad in ("re_start: 0, updates: 10", "re_start: 400", "re_start: 400, updates: 0", "re_start: .inf, updates: 10",
                "re_start: 400, updates: 10, hold: -1", "re_start: 400, updates: 10, stairs: -2",
                "re_start: 400, updates: 10, shape: cubic"):
        p.write_text("training:\n  re_continuation: {%s}\n" % bad)
        with pytest.raises(ValueError, match="training.re_continuation"):
            cfg.ConfigManager.from_file(str(p))
    for other in ("early_stop: {window: 500}", "identify_viscosity: {re0: 10}"):
        p.write_text("training:\n  re_continuation: {re_start: 400, updates: 10}\n  %s\n" % other)
        with pytest.raises(ValueError, match="training.re_continuation does not go together"):
            cfg.ConfigManager.from_file(str(p))
    p.write_text("training:\n  re_continuation: null\n")
    assert cfg.ConfigManager.from_file(str(p)).config.training.re_continuation is None
    out = io.StringIO()
    p.write_text("training:\n  re_continuation: {re_start: 400, updates: 10}\n")
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "Re ramp    : re_start=400 updates=10 hold=0 shape=geometric stairs=0" in out.getvalue()


# ------------------------------------------------------------------ two gloo ranks
def _run_rank(rank, world, out_dir):
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
        import recont_fakes
        recont_fakes.install(None)
        from nsfnet_amd import ev_pinn_solver as es
        torch.manual_seed(3)
        case = _case(N=71)
        P = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=10, hidden_size_1=6, N_f=71,
                                           alpha_evm=0.05, bc_weight=10, eq_weight=1)
        P.set_boundary_data(X=(case["xb"].reshape(-1, 1), case["yb"].reshape(-1, 1), case["ub"].reshape(-1, 1),
                               case["vb"].reshape(-1, 1)))
        P.set_eq_training_data(X=(case["x"].reshape(-1, 1), case["y"].reshape(-1, 1)))
        assert P.is_distributed and P.engine.world_size == world
        P.set_reynolds_continuation(80.0, 6, hold=1)
        e = P.engine
        nus = []
        for _ in range(4):
            e.step(1e-3)
            nus.append(e._rc.nu.numpy()[0])
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), rec=e._rc.rec.numpy(), nu=np.array(nus), cap=e._rc.cap.numpy(),
                 pos=e._rc.pos.numpy(), n=np.array(e.plan_f.n), params=e.net.params.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_hold_the_same_scalar_bits(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_run_rank, args=(world, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    assert sorted((int(r0["n"]), int(r1["n"]))) == [35, 36]
    for k in ("rec", "nu", "cap", "pos"):
        assert fm.same_bits(r0[k], r1[k]), k
    np.testing.assert_array_equal(r0["params"], r1["params"])
    c = rm.schedule(80.0, 800.0, 6, hold=1, cap_factor=20.0)
    assert fm.same_bits(r0["rec"], np.array(rm.value(c, 4))) and int(r0["pos"][0]) == 4
    assert [float(v) for v in r0["nu"]] == [rm.value(c, t)[3] for t in (1, 2, 3, 4)]


# ------------------------------------------------------------------ the inputs of the ev rows of the GPU test
from test_viscosity_cpu import ROW_BARS  # noqa: E402  (the bars of the GPU rows per quantity: the project's own)

_EV = {}


def _ev_refs(name):
    r = rm.EV_ROWS[name]
    key = (r["L"], r["H"])
    if key not in _EV:
        seed = rm.ev_seed(name)
        assert seed is not None
        c = rm.ev_case(name, seed)
        _EV[key] = (seed, c, rm.ev_reference(c, c["R0"]), rm.ev_reference(c, c["Re"]))
    return _EV[key]


@pytest.mark.parametrize("name", sorted(rm.EV_ROWS))
def test_ev_rows_bind_the_cap_at_part_of_the_points_and_tell_the_ends_apart(name):
    seed, c, start, end = _ev_refs(name)
    assert seed == rm.ev_seed(name)
    quarter = rm.N_ROW / 4.0
    b = start["binds"]
    assert b.sum() >= quarter and (~b).sum() >= quarter
    assert (start["vis_t"][b] == start["cap"]).all() and (start["vis_t"][~b] < start["cap"]).all()
    # no point sits on the threshold: the device's fp32 / bf16x3 entropy net decides as the oracle does
    assert (np.abs(start["vtm"] - start["cap"]) > rm.MARGIN * start["cap"]).all()
    # at the end the cap is another: a forward that keeps the configured cap is told apart by vis_t itself
    assert np.abs(start["vis_t"] - end["vis_t"]).max() > 0.5 * start["cap"]
    bar = ROW_BARS[c["prec"]]
    e0, e1 = start["eqs"][0], end["eqs"][0]
    assert np.abs(e0 - e1).max() > 10.0 * bar["plane"] * np.abs(e0).max()
    assert np.linalg.norm(start["grad"] - end["grad"]) > 10.0 * bar["grad"] * np.linalg.norm(start["grad"])
    # and the cap alone (nu of the start, the cap of the end) moves eq1 beyond ten bars, too
    mixed = rm.ev_reference(c, nu=np.float32(1.0) / np.float32(c["R0"]), cap=np.float32(rm.EV_FACTOR / c["Re"]))
    assert np.abs(e0 - mixed["eqs"][0]).max() > 10.0 * bar["plane"] * np.abs(e0).max()
