"""Reynolds-number continuation on the GPU (csrc/visc_sched.hip, the nu_dev / cap_dev members of the residual plans,
PinnEngine.set_reynolds_continuation) against the numpy statement of tests/recont_model.py:

  1. the step kernel alone: every shape, stairs and hold at the positions of the CPU test, twenty launches in a row, a
     start at position 3e9
  2. device scalars against the launch constants, per kernel family and variant (the rows of tests/visc_model.py, and an
     ev row per forward family, the fused kernel and PINN_FUSE=0 included): the engine configured at Re held at
     re_start = R0 and a plain engine configured at Re = R0 hold the same bits in every field plane, vis_t, the loss
     sums, the gradient and the loss; and so do the engine after a finished ramp and a plain engine at Re.  A kernel that
     ignores either pointer in a tile, a prologue or one of the fused kernel's argument blocks fails
  3. inside the ramp, one fp32 and one bf16x3 ev row: planes, loss sums and gradient at the model's (nu_t, cap_t) within
     the project's bars; vis_t <= cap_t everywhere, = cap_t where the oracle says the cap binds
  4. 20 engine updates over a ramp of 12 with hold = 3: the state is the model's after every update; hipGraph replays
     equal eager steps bit for bit, from one captured graph
  5. the options at 203 points: a batch of 75, attention, pseudo-time, conflict-free gradients, the resampling pool
  6. the training state: K updates, save inside the ramp, load into other weights, K more = 2 K in one go"""
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
import visc_model as vm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402
from test_viscosity_gpu import BARS, SWITCHES  # noqa: E402  (the project's bars per precision; the switches a row clears)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAR = 1 << 40           # a hold no test reaches: the ramp stays at its start
PLANES = ("u", "v", "u_x", "u_y", "v_x", "v_y", "eq1", "eq2", "eq3", "eq4", "p")


def _rel_max(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def _bc():
    return tuple(a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())


def _clean_env(monkeypatch, env=()):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def _engine(c, Re, **kw):
    """The engine of a row's case configured at Re, before any point set is attached."""
    from nsfnet_amd import engine as eng
    ev = {}
    if c.get("ev"):
        ev = dict(flavour="ev", n_hidden_e=rm.EV_NET[0], hidden_e=rm.EV_NET[1], alpha_evm=c.get("alpha_evm", vm.ALPHA_EVM))
    E = eng.PinnEngine(torch.device(DEV), c["L"], c["H"], Re, alpha_b=10.0, alpha_e=1.0, precision=c["prec"],
                       coord_scale=c["scale"], **ev, **kw)
    E.net.set_flat(torch.tensor(c["flat"]))
    if c.get("ff"):
        E.set_fourier_features(frequencies=c["B"])
    if c.get("ev"):
        E.net_e.set_flat(torch.tensor(c["flat_e"]))
        E.e_trainable = True
    if c.get("hard_bc"):
        E.set_hard_boundary()
    return E


def _attach(E, c):
    E.set_collocation(c["x"], c["y"], weights=c["w"])
    E.set_boundary(*_bc())
    assert E.plan_f.kernel_names() == c["names"], E.plan_f.kernel_names()


def _evaluate(E, times=1):
    for _ in range(times):
        E.loss_and_grad()
    torch.cuda.synchronize()
    f = E.plan_f
    return dict(fields=f.fields[:, :f.n].cpu().numpy().copy(), vis_t=f.vis_t.cpu().numpy().copy(),
                sums=E.sums.cpu().numpy().copy(), grads=E.grads.cpu().numpy().copy(),
                grads_e=E.grads_e.cpu().numpy().copy(), loss=float(E.loss_terms()["loss"]))


def _same(a, b, what):
    for k, plane in enumerate(PLANES):
        assert fm.same_bits(a["fields"][k], b["fields"][k]), (what, plane)
    assert np.abs(a["fields"][6]).max() > 0.0
    assert fm.same_bits(a["vis_t"], b["vis_t"]), (what, "vis_t")
    assert fm.same_bits(a["sums"], b["sums"]), (what, a["sums"], b["sums"])
    assert fm.same_bits(a["grads"], b["grads"]), (what, int((a["grads"] != b["grads"]).sum()))
    assert fm.same_bits(a["grads_e"], b["grads_e"]), (what, "grads_e")
    assert a["loss"] == b["loss"], what


def _scalars(E):
    rc = E._rc
    return (int(rc.pos.item()), np.float32(rc.nu.cpu().numpy()[0]),
            None if rc.cap is None else np.float32(rc.cap.cpu().numpy()[0]), rc.rec.cpu().numpy().copy())


# ------------------------------------------------------------------ 1. the kernel alone
def _struct(c):
    from nsfnet_amd import _lib
    return _lib.ViscScheduleStruct(shape=rm.SHAPES[c["shape"]], stairs=c["stairs"], hold=c["hold"], updates=c["updates"],
                                   re_start=c["re_start"], re_end=c["re_end"], cap_factor=c["cap_factor"],
                                   nu_start=c["nu_start"], nu_end=c["nu_end"], cap_start=c["cap_start"], cap_end=c["cap_end"])


def _close(got, want, geometric):
    """The record against the model's: bit for bit, but nu_t, cap_t within one fp32 ulp (and Re_t to 1e-12) inside a
    geometric ramp - the device's exp / log may differ from numpy's in the last bit of the double."""
    if not (geometric and 0.0 < want[1] < 1.0):
        return fm.same_bits(np.array(got), np.array(want))
    ulp = lambda v: float(np.spacing(np.float32(v)))
    return (got[0], got[1], got[5]) == (want[0], want[1], want[5]) and abs(got[2] - want[2]) <= 1e-12 * want[2] and \
        abs(got[3] - want[3]) <= ulp(want[3]) and abs(got[4] - want[4]) <= ulp(want[4])


def test_step_kernel_is_the_numpy_statement():
    from nsfnet_amd import engine as eng
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    nu = torch.zeros(1, dtype=torch.float32, device=DEV)
    cap = torch.zeros(1, dtype=torch.float32, device=DEV)
    rec = torch.zeros(rm.RECORD, dtype=torch.float64, device=DEV)
    ran = 0
    for shape in sorted(rm.SHAPES):
        for stairs in (0, 1, 4):
            for hold in (0, 7):
                c = rm.schedule(40.0, 400.0, 1000, hold=hold, shape=shape, stairs=stairs, cap_factor=20.0)
                cs, prev = _struct(c), None
                for t in rm.positions(c)[1:] + [1]:           # (position 0 is never written by a step: t = pos + 1 >= 1)
                    pos.fill_(t - 1)
                    nu.fill_(float("nan"))
                    cap.fill_(float("nan"))
                    eng.visc_schedule_step(cs, pos, nu, cap, rec)
                    got, want = rec.cpu().tolist(), rm.value(c, t)
                    assert int(pos.item()) == t and _close(got, want, shape == "geometric"), (shape, stairs, hold, t, got, want)
                    assert float(nu.item()) == got[3] and float(cap.item()) == got[4]
                    assert 40.0 <= got[2] <= 400.0
                    assert prev is None or t == 1 or (got[3] <= prev[3] and got[4] <= prev[4] and got[2] >= prev[2])
                    prev = got
                    ran += 1
    assert ran == 3 * 3 * 2 * 7
    # an ascending viscosity (re_start > Re): the clamp's other side, monotone the other way
    for shape in sorted(rm.SHAPES):
        c = rm.schedule(1000.0, 100.0, 1000, hold=7, shape=shape, cap_factor=20.0)
        cs, prev = _struct(c), None
        for t in rm.positions(c)[1:]:
            pos.fill_(t - 1)
            eng.visc_schedule_step(cs, pos, nu, cap, rec)
            got, want = rec.cpu().tolist(), rm.value(c, t)
            assert _close(got, want, shape == "geometric") and 100.0 <= got[2] <= 1000.0, (shape, t, got, want)
            assert prev is None or (got[3] >= prev[3] and got[4] >= prev[4] and got[2] <= prev[2])
            prev = got
        assert prev[3] == float(np.float32(1.0) / np.float32(100.0)) and prev[4] == float(np.float32(0.2))
    # twenty launches in a row advance the position by twenty, every record the model's; no cap: the word is not written
    c = rm.schedule(40.0, 400.0, 12, hold=3, shape="linear_re")
    cs = _struct(c)
    pos.zero_()
    cap.fill_(7.0)
    recs = []
    for _ in range(20):
        eng.visc_schedule_step(cs, pos, nu, None, rec)
        recs.append(rec.clone())
    assert int(pos.item()) == 20 and float(cap.item()) == 7.0
    for t, r in enumerate(recs, 1):
        assert fm.same_bits(r.cpu().numpy(), np.array(rm.value(c, t))), t
    # a start beyond 2^31
    c = rm.schedule(40.0, 400.0, 1000, hold=3_000_000_000 - 500, shape="linear_nu", cap_factor=20.0)
    cs = _struct(c)
    pos.fill_(3_000_000_000 - 1)
    for k in range(3):
        eng.visc_schedule_step(cs, pos, nu, cap, rec)
        want = rm.value(c, 3_000_000_000 + k)
        assert fm.same_bits(rec.cpu().numpy(), np.array(want)) and 0.0 < want[1] < 1.0
    assert int(pos.item()) == 3_000_000_002


# ------------------------------------------------------------------ 2. device scalars = the launch constants
def _row(name):
    if name in rm.EV_ROWS:
        seed = rm.ev_seed(name)
        assert seed is not None
        c = rm.ev_case(name, seed)
        return c, c["Re"], c["R0"]
    c = vm.row_case(name)
    return c, c["Re"], c["re0"]


ALL_ROWS = list(vm.ROWS) + list(vm.BIT_ROWS) + list(rm.EV_ROWS)


@pytest.mark.parametrize("name", ALL_ROWS)
def test_device_scalars_give_the_bits_of_the_launch_constants(monkeypatch, name):
    c, Re, R0 = _row(name)
    assert Re != R0
    _clean_env(monkeypatch, c.get("env", ()))
    ev = bool(c.get("ev"))
    A = _engine(c, Re)
    A.set_reynolds_continuation(R0, 10, hold=FAR)
    _attach(A, c)
    assert A.plan_f.nu is A._rc.nu and A.plan_f.lap is None and (A.plan_f.cap is not None) == ev
    B = _engine(c, R0)
    _attach(B, c)
    _same(_evaluate(A), _evaluate(B), "start")
    if ev:      # the cap at R0 binds at part of the points (tests/test_recont_cpu.py): vis_t tells the two caps apart
        vt = A.plan_f.vis_t.cpu().numpy()
        cap0 = np.float32(rm.EV_FACTOR / R0) if name in rm.EV_ROWS else np.float32(20.0 / R0)
        assert vt.max() <= cap0 and (name not in rm.EV_ROWS or (vt == cap0).sum() >= rm.N_ROW // 4)
    del B
    # the finished ramp: the bits of a plain engine at Re (both evaluate twice: an ev forward rewrites its lagged state)
    A.reset_reynolds_continuation(FAR + 10)
    info = A.continuation_info()
    assert info["done"] and info["nu_t"] == float(np.float32(1.0) / np.float32(Re))
    C = _engine(c, Re)
    _attach(C, c)
    C.loss_and_grad()
    _same(_evaluate(A), _evaluate(C), "end")
    if ev:
        assert info["cap_t"] == float(np.float32(C.vis_t0))
    # switched off after the ramp: a plain engine at Re
    A.set_reynolds_continuation(R0, 10, enabled=False)
    assert A.plan_f.nu is None and A.plan_f.cap is None
    _same(_evaluate(A), _evaluate(C), "off")


# ------------------------------------------------------------------ 3. inside the ramp
@pytest.mark.parametrize("name", ["ev-4x50-fp32", "ev-3x256-bf16x3-fused"])
def test_inside_the_ramp_the_evaluation_is_the_model_at_nu_t_and_cap_t(monkeypatch, name):
    from oracle import fwdmode_ref as fr
    c, Re, R0 = _row(name)
    _clean_env(monkeypatch, c.get("env", ()))
    E = _engine(c, Re)
    # early in a long ramp: the cap has left its start and still lies inside the range of alpha_evm |e|
    E.set_reynolds_continuation(R0, 100)
    _attach(E, c)
    E.reset_reynolds_continuation(5)
    t, nu, cap, rec = _scalars(E)
    want = rm.value(rm.schedule(R0, Re, 100, cap_factor=rm.EV_FACTOR), 5)
    assert t == 5 and abs(float(nu) - want[3]) <= float(np.spacing(np.float32(want[3])))
    assert abs(float(cap) - want[4]) <= float(np.spacing(np.float32(want[4]))) and np.float32(E.vis_t0) < cap < np.float32(20.0 / R0)
    got = _evaluate(E)
    r = rm.ev_reference(c, nu=nu, cap=cap)
    P = fr.unflatten(c["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
    xb, yb, ub, vb = _bc()
    b = fr.bc_loss_and_grad(P, xb.astype(np.float64), yb.astype(np.float64), ub, vb, alpha_b=10.0)
    bar = BARS[c["prec"]]
    errs = {"eq%d" % (k + 1): _rel_max(got["fields"][6 + k], r["eqs"][k]) for k in range(4)}
    errs["sums"] = _rel_max(got["sums"][:4], np.asarray(r["sums"]))
    ref_loss = 10.0 * (b["sums"][0] + b["sums"][1]) / xb.size + r["loss_e"]
    errs["loss"] = abs(got["loss"] - ref_loss) / ref_loss
    blocks = lambda g: [q for wb in fr.unflatten(np.asarray(g, np.float64), 2, 3, c["L"], c["H"]) for q in wb]
    errs["grad"] = max(float(np.linalg.norm(p - q) / max(np.linalg.norm(q), 1e-300))
                       for p, q in zip(blocks(got["grads"]), blocks(r["grad"] + b["grad"])))
    print("[recont] %s inside the ramp (Re_t %.2f): %s" % (name, rec[2], " ".join("%s %.2e" % kv for kv in errs.items())))
    for k, v in errs.items():
        assert v <= (bar["eq"] if k.startswith("eq") else bar[k]), (k, v)
    vt = got["vis_t"]
    assert (vt <= cap).all()
    clear = np.abs(r["vtm"] - r["cap"]) > 1e-3 * r["cap"]        # (a point on the threshold may fall either way in fp32)
    assert (vt[r["binds"] & clear] == cap).all() and (vt[~r["binds"] & clear] < cap).all()
    assert (r["binds"] & clear).sum() >= 5 and (~r["binds"] & clear).sum() >= 5


# ------------------------------------------------------------------ 4. the engine's trajectory; replay = eager
def test_engine_trajectory_is_the_model_after_every_update(monkeypatch):
    _clean_env(monkeypatch)
    c = vm.row_case("2x8-fp32")
    E = _engine(c, c["Re"])
    E.set_reynolds_continuation(c["re0"], 12, hold=3)
    _attach(E, c)
    sched = rm.schedule(c["re0"], c["Re"], 12, hold=3)
    for k in range(1, 21):
        E.step(1e-3)
        t, nu, cap, rec = _scalars(E)
        assert t == k and cap is None and _close(rec.tolist(), rm.value(sched, k), True), (k, rec)
        assert float(nu) == rec[3]
    info = E.continuation_info()
    assert info["done"] and info["t"] == 20 and info["nu_t"] == float(np.float32(1.0) / np.float32(c["Re"]))


def _train(monkeypatch, graph, steps, name):
    _clean_env(monkeypatch, (("NSFNET_GRAPH", "1"),) if graph else ())
    c = vm.row_case(name)
    E = _engine(c, c["Re"])
    E.set_reynolds_continuation(c["re0"], 12, hold=3)
    _attach(E, c)
    for _ in range(steps):
        E.step(1e-3)
    torch.cuda.synchronize()
    t, nu, cap, rec = _scalars(E)
    out = dict(p=E.net.params.cpu().numpy().copy(), nu=np.array([nu]), rec=rec, pos=np.array([t]), graphs=len(E._graphs))
    if c.get("ev"):
        out.update(pe=E.net_e.params.cpu().numpy().copy(), cap=np.array([cap]))
    return out


@pytest.mark.parametrize("name", ["2x8-fp32", "4x50-fp32-ev"])
def test_replayed_steps_equal_eager_ones_from_a_single_graph(monkeypatch, name):
    eager = _train(monkeypatch, False, 20, name)
    replay = _train(monkeypatch, True, 20, name)            # 1 eager step + the capture, then 19 replays across the ramp
    for k in eager:
        if k != "graphs":
            assert fm.same_bits(eager[k], replay[k]), k
    assert replay["graphs"] == 1 and eager["graphs"] == 0 and eager["pos"][0] == 20 and eager["rec"][5] == 1.0
    assert ("cap" in eager) == (name == "4x50-fp32-ev")


# ------------------------------------------------------------------ 5. the options at 203 points
def _option_engine(monkeypatch, Re=None, setup=None, ramp=None):
    _clean_env(monkeypatch)
    c = vm.row_case("2x8-fp32", n=vm.N_OPT)
    E = _engine(c, c["Re"] if Re is None else Re)
    if setup is not None:
        setup(E)
    if ramp is not None:
        E.set_reynolds_continuation(c["re0"], **ramp)
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(*_bc())
    return E, c


def test_a_batch_of_75_under_the_ramp_holds_the_model_state(monkeypatch):
    E, c = _option_engine(monkeypatch, ramp=dict(updates=6, hold=1, shape="linear_re"))
    E.set_batching(vm.B_OPT, seed=3)
    assert E._batch.f.nu is E._rc.nu and E._batch.f.lap is None
    sched = rm.schedule(c["re0"], c["Re"], 6, hold=1, shape="linear_re")
    for k in range(1, 9):
        nu_read = float(E._rc.nu.item())
        E.step(1e-3)
        assert E.evaluated_batch and fm.same_bits(_scalars(E)[3], np.array(rm.value(sched, k))), k
        if k == 4:      # the batch plan's planes are the model's at the viscosity the step read
            idx = E.batch_indices().cpu().numpy()
            r = vm.evaluate(flat, c["L"], c["H"], c["x"][idx], c["y"][idx], nu_read, want_grad=False)
            err = _rel_max(E._batch.f.field("eq1").cpu().numpy(), r["eqs"][0])
            assert 0.0 < rm.value(sched, 3)[1] < 1.0 and err <= BARS["fp32"]["eq"], err
        flat = E.net.params.cpu().numpy().copy()
    assert E.batch_info()["draws"] == 8 and E.continuation_info()["done"]


@pytest.mark.parametrize("option", ["rba", "ptime", "confgrad"])
def test_first_evaluation_with_an_option_equals_a_plain_engine_at_the_start(monkeypatch, option):
    setup = dict(rba=lambda E: None, ptime=lambda E: E.set_pseudo_time(dtau=0.1, every=2),
                 confgrad=lambda E: E.set_conflict_free_gradients())[option]
    after = (lambda E: E.set_residual_attention(eta=0.5, gamma=0.9)) if option == "rba" else (lambda E: None)
    c0 = vm.row_case("2x8-fp32", n=vm.N_OPT)
    A, c = _option_engine(monkeypatch, setup=setup, ramp=dict(updates=6, hold=FAR))
    after(A)
    B, _ = _option_engine(monkeypatch, Re=c0["re0"], setup=setup)
    after(B)
    _same(_evaluate(A), _evaluate(B), option)
    A.adam_step(1e-3)
    B.adam_step(1e-3)
    _same(_evaluate(A), _evaluate(B), option + ", second")      # the option's own state moved alike (weights, anchors)
    assert A.continuation_info()["t"] == 1 and not A.continuation_info()["done"]


def test_the_pool_s_forward_reads_the_ramp(monkeypatch):
    E, c = _option_engine(monkeypatch, ramp=dict(updates=10, shape="linear_nu"))
    xp, yp = vm.pool_points()
    E.set_resample_pool(xp, yp)
    assert E._pool.nu is E._rc.nu and E._pool.lap is None
    E.reset_reynolds_continuation(4)
    nu_t = float(E._rc.nu.item())
    assert nu_t == rm.value(rm.schedule(c["re0"], c["Re"], 10, shape="linear_nu"), 4)[3]
    at = lambda nu: vm.evaluate(c["flat"], c["L"], c["H"], xp, yp, nu, want_grad=False)["eqs"][0]
    E.resample(seed=1)
    torch.cuda.synchronize()
    got = E._pool.field("eq1").cpu().numpy()
    err, far = _rel_max(got, at(nu_t)), _rel_max(got, at(1.0 / c["Re"]))
    print("[recont] pool eq1 against the model at nu_t %.2e, at 1 / Re %.2e" % (err, far))
    assert err <= BARS["fp32"]["eq"] and far > 10.0 * BARS["fp32"]["eq"]


# ------------------------------------------------------------------ 6. the training state
@pytest.mark.parametrize("name", ["2x8-fp32", "4x50-fp32-ev"])
def test_training_state_resumes_inside_the_ramp_bit_for_bit(monkeypatch, tmp_path, name):
    _clean_env(monkeypatch)
    c = vm.row_case(name)
    K = 4

    def make(flat_scale=1.0):
        E = _engine(dict(c, flat=(c["flat"] * np.float32(flat_scale))), c["Re"])
        E.set_reynolds_continuation(c["re0"], 12, hold=1)
        E.set_collocation(c["x"], c["y"], weights=c["w"])
        E.set_boundary(*_bc())
        return E

    whole = make()
    for _ in range(2 * K):
        whole.step(1e-3)
    first = make()
    for _ in range(K):
        first.step(1e-3)
    assert 0.0 < first.continuation_info()["s"] < 1.0
    path = str(tmp_path / "state.bin")
    first.save_training_state(path)
    second = make(flat_scale=0.5)
    assert second.load_training_state(path)["changed"] == []
    for _ in range(K):
        second.step(1e-3)
    torch.cuda.synchronize()
    a, b = _scalars(second), _scalars(whole)
    assert a[0] == b[0] == 2 * K and a[1] == b[1] and a[2] == b[2] and fm.same_bits(a[3], b[3])
    assert (a[2] is not None) == bool(c.get("ev"))
    assert fm.same_bits(second.net.params.cpu().numpy(), whole.net.params.cpu().numpy())
    if c.get("ev"):
        assert fm.same_bits(second.net_e.params.cpu().numpy(), whole.net_e.params.cpu().numpy())
