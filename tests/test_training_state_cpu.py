"""CPU tests of the training-state snapshots: the real library's host-only entry points against
the numpy model of tests/state_model.py, the file (round trip, byte-identical repeats, refusals that leave the engine
untouched, the atomic rename) and, on the model-backed fakes, the bit-for-bit continuation of every training option
across save, a fresh engine and load.  The kernels are checked against the model in test_training_state_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import state_model as sm  # noqa: E402

L, H, RE = 2, 10, 400.0
SHAPE_E = (1, 2, 6)
LR = 2.0 ** -10
K = 4


# ------------------------------------------------------------------ the host-only entry points against the model
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def _lib_digest(lib, a):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    out = (ctypes.c_uint64 * 2)()
    assert lib.pinn_state_digest_host(ctypes.c_void_p(raw.ctypes.data if raw.size else 0), raw.size, out) == 0
    return int(out[0]), int(out[1])


def test_digest_known_answer(lib):
    a = np.arange(1, 9, dtype=np.float32)
    assert sm.digest(a) == sm.KNOWN_ANSWER
    assert _lib_digest(lib, a) == sm.KNOWN_ANSWER


@pytest.mark.parametrize("nbytes", [0, 4, 12, 16, 20, 16384 - 4, 16384, 16384 + 4])
def test_digest_host_equals_the_model(lib, nbytes):
    raw = np.random.RandomState(nbytes).randint(0, 256, nbytes).astype(np.uint8)
    assert _lib_digest(lib, raw) == sm.digest(raw)


def test_digest_wraps_on_32_mib_of_ones(lib):
    raw = np.full(32 << 20, 0xFF, dtype=np.uint8)
    n = raw.size // 4
    assert (2 ** 32 - 1) * n * (n + 1) // 2 >= 2 ** 64           # B wraps
    want = (((2 ** 32 - 1) * n) % 2 ** 64, ((2 ** 32 - 1) * n * (n + 1) // 2) % 2 ** 64)
    assert sm.digest(raw) == want
    assert _lib_digest(lib, raw) == want


def test_layout_equals_the_model_and_refuses_odd_sizes(lib):
    sizes = [0, 4, 12, 16, 20, 16380, 16384, 16388, 0, 256, 260, 8]
    b = (ctypes.c_int64 * len(sizes))(*sizes)
    o = (ctypes.c_int64 * len(sizes))()
    total = lib.pinn_state_layout(len(sizes), b, o)
    offs, want = sm.layout(sizes)
    assert (list(o), total) == (offs, want)
    assert all(v % 256 == 0 for v in offs)
    b[3] = 18
    assert lib.pinn_state_layout(len(sizes), b, o) == -1 and b"multiple of 4" in lib.pinn_last_error()
    out = (ctypes.c_uint64 * 2)()
    assert lib.pinn_state_digest_host(ctypes.c_void_p(0), 6, out) < 0
    assert lib.pinn_state_scratch_bytes() > 0


# ------------------------------------------------------------------ the engine on the fakes
def _case(seed=42, N=70, Nb=33, Nv=41, Ns=19):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    x, y = f32(rng.rand(N)), f32(rng.rand(N))
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    xv, yv = f32(rng.rand(Nv)), f32(rng.rand(Nv))
    xs, ys = f32(rng.rand(Ns)), f32(rng.rand(Ns))
    ps = f32(xs * ys)
    ps[::4] = np.nan
    return dict(x=x, y=y, w=f32(0.5 + rng.rand(N)), xb=xb, yb=yb, ub=ub, vb=vb,
                val=(xv, yv, f32(np.sin(3 * xv) * yv), f32(np.cos(2 * yv) * xv), f32(0.2 + xv * yv)),
                sup=(xs, ys, f32(np.sin(xs)), f32(np.cos(ys)), ps))


def _engine(monkeypatch, case, flavour="nsfnet", seed=5, base=None, setup=None, weights=False, sup=False):
    import state_fakes
    import val_fakes
    state_fakes.install(monkeypatch, base or val_fakes)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=SHAPE_E[1], hidden_e=SHAPE_E[2], alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, alpha_s=2.0 if sup else 0.0, **ev)
    rng = np.random.RandomState(seed)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"], case["w"] if weights else None)
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    if sup:
        e.set_supervised(*case["sup"])
    if setup is not None:
        setup(e)
    return e


def _snapshot(e):
    """Every state tensor (by segment name), the host mirrors and the loss terms of the last evaluation."""
    out = {name: t.detach().clone().numpy() for name, t, stored in e._state_segments() if stored}
    out["host"] = e._state_host()
    out["loss"] = {k: np.asarray(v) for k, v in e.loss_terms().items()}
    return out


def _assert_same(a, b, loss=True):
    assert sorted(a) == sorted(b)
    assert a["host"] == b["host"]
    for k in a:
        if k == "loss" and not loss:        # (the loss terms are not state: after a load they are the next evaluation's)
            continue
        if k == "loss":
            for name in a[k]:
                np.testing.assert_array_equal(a[k][name], b[k][name], err_msg=name)
        elif k != "host":
            np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


def _continuation(monkeypatch, tmp_path, case, advance, k=K, **kw):
    """2k updates in one go against k, save, a fresh engine with other weights, load, k more."""
    whole = _engine(monkeypatch, case, **kw)
    for i in range(2 * k):
        advance(whole, i)
    first = _engine(monkeypatch, case, **kw)
    for i in range(k):
        advance(first, i)
    path = str(tmp_path / "state.bin")
    first.save_training_state(path, extra=dict(next=k))
    second = _engine(monkeypatch, case, seed=77, **kw)
    got = second.load_training_state(path)
    assert got == dict(extra=dict(next=k), changed=[])
    for i in range(k, 2 * k):
        advance(second, i)
    _assert_same(_snapshot(whole), _snapshot(second))
    return whole, second


def _step(e, i):
    e.step(LR)


def test_file_round_trip_is_byte_identical_and_matches_the_model(monkeypatch, tmp_path):
    case = _case()
    e = _engine(monkeypatch, case, setup=lambda e: e.set_loss_balancing(every=2))
    for i in range(3):
        e.step(LR)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    e.save_training_state(a, extra=dict(tag="x"))
    e.save_training_state(b, extra=dict(tag="x"), wait=False)
    info = e.training_state_info()
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    assert not os.path.exists(b + ".tmp")
    header, payload = sm.parse(raw)
    segs = e._state_segments()
    assert [s["name"] for s in header["segments"]] == [name for name, _, _ in segs] == info["segments"]
    want, offs, digs = sm.pack([t.numpy() for _, t, _ in segs], [stored for _, _, stored in segs])
    assert payload == want and info["bytes"] == len(want)
    assert [s["offset"] for s in header["segments"]] == offs
    assert [tuple(s["digest"]) for s in header["segments"]] == digs
    assert raw == sm.file_bytes(header, want)                       # sorted keys, zero padding, nothing else
    assert header["extra"] == dict(tag="x") and header["fingerprint"]["balancing"] is True
    assert any(not stored for _, _, stored in segs)                 # the boundary set is digested, not stored
    before = _snapshot(e)
    assert e.load_training_state(a) == dict(extra=dict(tag="x"), changed=[])
    _assert_same(before, _snapshot(e))


def test_damaged_files_are_refused_and_leave_the_engine_untouched(monkeypatch, tmp_path):
    from nsfnet_amd.engine import StateFileError
    case = _case()
    e = _engine(monkeypatch, case)
    e.step(LR)
    path = str(tmp_path / "s.bin")
    e.save_training_state(path)
    raw = open(path, "rb").read()
    other = _engine(monkeypatch, case, seed=9)
    other.step(LR)
    before = _snapshot(other)
    header, _ = sm.parse(raw)
    first = len(raw) - max(s["offset"] + s["bytes"] for s in header["segments"] if s["offset"] >= 0)
    flipped = bytearray(raw)
    flipped[first + 5] ^= 0x10
    for name, data in (("short", raw[:-8]), ("flip", bytes(flipped)), ("head", raw[:40]), ("magic", b"X" + raw[1:])):
        bad = str(tmp_path / name)
        open(bad, "wb").write(data)
        with pytest.raises(StateFileError):
            other.load_training_state(bad)
        _assert_same(before, _snapshot(other))
    other.load_training_state(path)
    _assert_same(_snapshot(e), _snapshot(other), loss=False)


def test_a_failing_rename_leaves_the_old_file_loadable(monkeypatch, tmp_path):
    case = _case()
    e = _engine(monkeypatch, case)
    e.step(LR)
    path = str(tmp_path / "s.bin")
    e.save_training_state(path)
    old = open(path, "rb").read()
    at_save = _snapshot(e)
    e.step(LR)

    def boom(*a):
        raise OSError("no rename today")

    monkeypatch.setattr(os, "replace", boom)
    with pytest.raises(OSError):
        e.save_training_state(path)
    e.save_training_state(path, wait=False)
    with pytest.raises(OSError):                                     # the writer's error surfaces at the join
        e.training_state_info()
    monkeypatch.undo()
    assert open(path, "rb").read() == old
    other = _engine(monkeypatch, case, seed=3)
    other.load_training_state(path)
    _assert_same(at_save, _snapshot(other), loss=False)


def test_fingerprint_refusals_name_their_key(monkeypatch, tmp_path):
    from nsfnet_amd import schedule
    case = _case()
    e = _engine(monkeypatch, case, setup=lambda e: e.set_residual_attention(eta=0.01))
    e.step(LR)
    path = str(tmp_path / "s.bin")
    e.save_training_state(path)
    rba = lambda e: e.set_residual_attention(eta=0.01)

    def both(e):
        rba(e)
        e.set_lr_schedule(schedule.LrSchedule("exponential", gamma=0.9))

    small = dict(case, x=case["x"][:-1], y=case["y"][:-1])
    for key, kw, c in (("attention", {}, case), ("schedule_or_clipping", dict(setup=both), case),
                       ("points_colloc", dict(setup=rba), small), ("flavour", dict(setup=rba, flavour="ev"), case)):
        other = _engine(monkeypatch, c, **kw)
        with pytest.raises(ValueError, match="fingerprint key %r" % key):
            other.load_training_state(path)
    other = _engine(monkeypatch, case, setup=rba)
    monkeypatch.setattr(other, "_rank", lambda: 1)
    with pytest.raises(ValueError, match="fingerprint key 'rank'"):
        other.load_training_state(path)
    other.world_size = 2
    with pytest.raises(FileNotFoundError):                           # several ranks: every rank its own file
        other.load_training_state(path)


def test_strict_checks_the_sets_that_are_not_stored(monkeypatch, tmp_path):
    case = _case()
    e = _engine(monkeypatch, case)
    e.step(LR)
    path = str(tmp_path / "s.bin")
    e.save_training_state(path)
    moved = dict(case, ub=case["ub"] + np.float32(0.5))
    other = _engine(monkeypatch, moved)
    before = _snapshot(other)
    with pytest.raises(ValueError, match="boundary.target0"):
        other.load_training_state(path)
    other.loss_and_grad()
    before["loss"] = _snapshot(other)["loss"]
    _assert_same(before, _snapshot(other))                          # refused before anything was written
    assert other.load_training_state(path, strict=False)["changed"] == []
    np.testing.assert_array_equal(other.net.params.numpy(), e.net.params.numpy())


def test_changed_info_is_reported_not_refused(monkeypatch, tmp_path):
    case = _case()
    e = _engine(monkeypatch, case)
    e.step(LR)
    path = str(tmp_path / "s.bin")
    e.save_training_state(path)
    other = _engine(monkeypatch, case)
    other.Re, other.alpha_b = 500.0, 3.0
    assert other.load_training_state(path)["changed"] == ["Re", "alpha_b"]


# ------------------------------------------------------------------ every option continues bit for bit
def test_plain_and_balancing_continue(monkeypatch, tmp_path):
    case = _case()
    _continuation(monkeypatch, tmp_path, case, _step)
    whole, _ = _continuation(monkeypatch, tmp_path, case, _step, k=4, sup=True,
                             setup=lambda e: e.set_loss_balancing(every=3, beta=0.3))
    assert whole.balance_info()["updates"] == 3                      # updates 0, 3 | 6: both sides of the cut


def test_batching_continues(monkeypatch, tmp_path):
    whole, second = _continuation(monkeypatch, tmp_path, _case(), _step, flavour="ev", weights=True,
                                  setup=lambda e: e.set_batching(batch_points=20, seed=11))
    assert whole.batch_info()["draws"] == second.batch_info()["draws"] == 2 * K


def test_attention_continues(monkeypatch, tmp_path):
    whole, _ = _continuation(monkeypatch, tmp_path, _case(), _step, weights=True,
                             setup=lambda e: e.set_residual_attention(eta=0.05, gamma=0.9))
    assert whole.attention_info()["updates"] == 2 * K


def test_schedule_and_clipping_continue(monkeypatch, tmp_path):
    from nsfnet_amd import schedule

    def setup(e):
        e.set_lr_schedule(schedule.LrSchedule("cosine", t_max=20, warmup_epochs=5))
        e.set_grad_clipping(0.05)

    whole, second = _continuation(monkeypatch, tmp_path, _case(), _step, setup=setup)
    assert second.optimizer_info()["next_epoch"] == 2 * K


def test_weight_factorization_continues(monkeypatch, tmp_path):
    whole, second = _continuation(monkeypatch, tmp_path, _case(), _step, flavour="ev",
                                  setup=lambda e: e.set_weight_factorization(mean=0.5, std=0.1, seed=3))
    np.testing.assert_array_equal(whole.net.params.numpy(), second.net.params.numpy())


def test_validation_continues(monkeypatch, tmp_path):
    case = _case()
    whole, second = _continuation(monkeypatch, tmp_path, case, _step,
                                  setup=lambda e: e.set_validation(*case["val"], every=3, history=2))
    assert whole.validation_info() == second.validation_info() and whole.validation_info()["records"] == 2
    sd, sd2 = whole.best_state_dict(), second.best_state_dict()
    assert sd is not None and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_conflict_free_gradients_continue(monkeypatch, tmp_path):
    import confgrad_fakes
    whole, _ = _continuation(monkeypatch, tmp_path, _case(), _step, base=confgrad_fakes, sup=True,
                             setup=lambda e: e.set_conflict_free_gradients(True))
    assert whole.conflict_info()["steps"] == 2 * K


def test_ev_freeze_and_unfreeze_continue(monkeypatch, tmp_path):
    def advance(e, i):
        if i in (1, 2, 5):
            e.e_trainable = not e.e_trainable
            if not e.e_trainable:
                e.net_e.reset_adam()
        e.step(LR)

    whole, second = _continuation(monkeypatch, tmp_path, _case(), advance, flavour="ev")
    assert second.e_trainable is True and second.net_e.adam_t == whole.net_e.adam_t > 0


def test_lbfgs_continues_and_is_adopted_by_a_new_owner(monkeypatch, tmp_path):
    def advance(e, i):
        e.lbfgs_step(max_iter=3, history_size=4, line_search_fn="strong_wolfe", owner=e)

    whole, second = _continuation(monkeypatch, tmp_path, _case(), advance, k=2)
    ls, ls2 = whole._lbfgs_state, second._lbfgs_state
    assert (ls.n_iter, ls.func_evals, ls.t, ls.prev_loss) == (ls2.n_iter, ls2.func_evals, ls2.t, ls2.prev_loss)
    assert ls.n_iter > 3                                             # the history carried across the cut


# ------------------------------------------------------------------ the solver loops with start_epoch
def _plain_solver(monkeypatch, case, seed):
    import state_fakes
    state_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    from nsfnet_amd import schedule
    torch.manual_seed(seed)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=L, hidden_size=H, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.set_lr_schedule(schedule.LrSchedule("exponential", gamma=0.9, warmup_epochs=3))
    P.set_loss_balancing(every=3)
    P.log_every, P.save_every = 2, 0
    return P


def _ev_solver(monkeypatch, case, seed):
    import state_fakes
    state_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(seed)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=L, layers_1=SHAPE_E[1], hidden_size=H, hidden_size_1=SHAPE_E[2],
                                       N_f=70, alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.set_residual_attention(eta=0.05, gamma=0.9)
    P.log_interval = 2
    P.freeze_period = 4             # unfreeze at 4 and 8, re-freeze at 5 and 9: the cut at 5 falls between the two
    P.save = lambda *a, **k: None
    return P


def _train(P, capsys, **kw):
    capsys.readouterr()
    P.train(lr=LR, **kw)
    return [ln for ln in capsys.readouterr().out.splitlines() if "it/s=" not in ln]


def _blocks(lines, num_epoch):
    """{epoch (1-based): the lines logged for it}: a block starts at the line that carries 'epoch / num_epoch'."""
    import re
    out, cur = {}, None
    for ln in lines:
        m = re.search(r"(\d+)\s*/\s*%d\b" % num_epoch, ln)
        if m:
            cur = int(m.group(1))
        if cur is not None:
            out.setdefault(cur, []).append(ln)
    return out


@pytest.mark.parametrize("make,cut", [(_plain_solver, 5), (_ev_solver, 5)])
def test_solver_loops_continue_with_start_epoch(monkeypatch, tmp_path, capsys, make, cut):
    monkeypatch.chdir(tmp_path)
    case = _case()
    whole = make(monkeypatch, case, 1)
    lines = _train(whole, capsys, num_epoch=2 * cut)
    first = make(monkeypatch, case, 1)
    path = str(tmp_path / "ckpt.bin")
    first.set_checkpointing(path, every=cut)
    _train(first, capsys, num_epoch=2 * cut, stop_epoch=cut)         # the last epoch this call runs writes the snapshot
    first.engine.training_state_info()
    second = make(monkeypatch, case, 2)
    extra = second.load_training_state(path)
    assert extra["next_epoch"] == cut and extra["num_epoch"] == 2 * cut
    tail = _train(second, capsys, num_epoch=2 * cut, start_epoch=extra["next_epoch"])
    _assert_same(_snapshot(whole.engine), _snapshot(second.engine))
    assert getattr(whole, "global_step", None) == getattr(second, "global_step", None)
    assert second.opt.param_groups[0]["lr"] == whole.opt.param_groups[0]["lr"] and second._lr0 == whole._lr0
    # every line logged after the cut (the rate line carries wall time and is left out)
    want, got = _blocks(lines, 2 * cut), _blocks(tail, 2 * cut)
    assert {e: b for e, b in want.items() if e > cut} == got and len(got) >= 2


def test_checkpointing_cadence_and_default(monkeypatch, tmp_path, capsys):
    monkeypatch.chdir(tmp_path)
    case = _case()
    P = _plain_solver(monkeypatch, case, 1)
    calls = []
    monkeypatch.setattr(P, "save_training_state", lambda path, **kw: calls.append((path, kw["next_epoch"], kw["wait"])))
    P.train(num_epoch=3, lr=LR)
    assert calls == []                                                # off by default
    P.set_checkpointing("c.bin", every=2)
    P.train(num_epoch=5, lr=LR)
    assert calls == [("c.bin", 2, False), ("c.bin", 4, False), ("c.bin", 5, False)]


# ------------------------------------------------------------------ configuration and scripts
def _config_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_state", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_yaml_key_is_off_by_default_and_parses(tmp_path, capsys):
    cfg = _config_module()
    prod = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml")
    mgr = cfg.ConfigManager.from_file(prod)
    ck = mgr.config.training.checkpoint
    assert (ck.path, ck.every, ck.enabled) == ("", 0, False)
    mgr.print_config()
    assert "checkpoint" not in capsys.readouterr().out               # existing configs print what they printed
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  checkpoint: {path: run/state.bin, every: 5000}\n")
    mgr = cfg.ConfigManager.from_file(str(p))
    ck = mgr.config.training.checkpoint
    assert (ck.path, ck.every, ck.enabled) == ("run/state.bin", 5000, True)
    mgr.print_config()
    assert "checkpoint : path=run/state.bin every=5000" in capsys.readouterr().out
    p.write_text("training:\n  checkpoint: {every: 10}\n")
    with pytest.raises(ValueError, match="training.checkpoint"):
        cfg.ConfigManager.from_file(str(p))
    train = open(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "train.py")).read()
    assert '"--resume"' in train and train.index("set_validation_data") < train.index("load_training_state(args.resume)")


def _converge(monkeypatch, out, *extra):
    import contextlib
    import importlib.util
    import io
    import state_fakes
    state_fakes.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    spec = importlib.util.spec_from_file_location("converge_ev_state", os.path.join(ROOT, "scripts", "converge_ev.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    dns = os.path.join(ROOT, "tests", "golden", "dns", "cavity_Re3000_256_Uniform.mat")
    monkeypatch.setattr(sys, "argv", ["converge_ev.py", "--dns", dns, "--out", str(out), "--first", "1", "--last", "2",
                                      "--epochs-scale", "1e-5", "--nf", "40", "--layers", "2", "--hidden", "8",
                                      "--balance-every", "2", "--rba-eta", "0.01", "--scheduler", "cosine",
                                      "--validate-every", "2"] + list(extra))
    cwd = os.getcwd()
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            mod.main()
    finally:
        os.chdir(cwd)
    return buf.getvalue()


def test_converge_ev_slices_end_anywhere_and_continue(monkeypatch, tmp_path):
    """Two stages of 5 updates: in one call, and in calls of at most 3 updates that share a state file - the cuts fall
    inside stage 1, at its end... wherever 3 updates lead.  The final weights are the same bits."""
    whole = tmp_path / "whole"
    _converge(monkeypatch, whole)
    cut = tmp_path / "cut"
    state = str(tmp_path / "cut.state")
    outs = [_converge(monkeypatch, cut, "--state", state, "--max-steps", "3") for _ in range(4)]
    assert ['"next_epoch": 3' in o for o in outs[:2]] == [True, False] and "SLICE" in outs[0]
    for name in ("net.pth", "net_evm.pth"):
        a = torch.load(whole / name, map_location="cpu", weights_only=True)
        b = torch.load(cut / name, map_location="cpu", weights_only=True)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), name
    import json
    recs = [json.loads(l) for l in open(cut / "stages.jsonl")]
    want = [json.loads(l) for l in open(whole / "stages.jsonl")]
    assert [r["stage"] for r in recs] == [1, 2]
    for key in ("loss", "loss_b", "loss_e", "err_u", "err_v", "best_metric", "best_t"):
        assert [r[key] for r in recs] == [r[key] for r in want], key


def test_run_stages_skips_finished_stages_and_enters_the_saved_one(monkeypatch):
    """The ev drop-in's stage loop with the `extra` of a loaded state: stages before current_stage do not run, the
    saved stage starts at next_epoch, the later ones at 0; a state of an unknown stage is refused."""
    import importlib.util
    from types import SimpleNamespace
    here = os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet")
    monkeypatch.syspath_prepend(here)
    import types
    for name in ("cavity_data", "pinn_solver", "config", "logger"):      # the drop-in's own modules, by their bare names:
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))  # imported fresh here, gone again at teardown
        del sys.modules[name]
    spec = importlib.util.spec_from_file_location("ev_dropin_train_state", os.path.join(here, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    cfg = sys.modules["config"]
    stages = [cfg.TrainingStage(0.05, 10, 1e-3, "Stage 1"), cfg.TrainingStage(0.03, 10, 2e-4, "Stage 2", scheduler="cosine"),
              cfg.TrainingStage(0.01, 10, 4e-5, "Stage 3")]
    calls = []
    PINN = SimpleNamespace(set_alpha_evm=lambda a: calls.append(("alpha", a)),
                           train=lambda **kw: calls.append((kw["num_epoch"], kw["lr"], kw["start_epoch"], "scheduler" in kw)))
    log = SimpleNamespace(stage=lambda *a: None)
    train.run_stages(PINN, stages, 1.0, 0, log, resume=dict(current_stage="Stage 2", next_epoch=4))
    assert calls == [("alpha", 0.03), (10, 2e-4, 4, True), ("alpha", 0.01), (10, 4e-5, 0, False)]
    assert PINN.current_stage == "Stage 3"
    del calls[:]
    train.run_stages(PINN, stages, 1.0, 0, log)
    assert [c for c in calls if c[0] == 10] == [(10, 1e-3, 0, False), (10, 2e-4, 0, True), (10, 4e-5, 0, False)]
    with pytest.raises(ValueError, match="Stage 9"):
        train.run_stages(PINN, stages, 1.0, 0, log, resume=dict(current_stage="Stage 9", next_epoch=0))
