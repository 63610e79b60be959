"""GPU tests of the device learning-rate schedules and gradient clipping: pinn_grad_sqnorm and
pinn_adam_step_sched against the fp64 model of tests/optim_model.py and against pinn_adam_step_dev (bitwise: only lr and
the scaled gradient differ), against torch.optim.Adam + CosineAnnealingLR + clip_grad_norm_, the counters, and the whole
step eager against graph replay (bitwise, one captured graph for the stage), also with mini-batching."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fold_model as fm  # noqa: E402
import optim_model as om  # noqa: E402
from nsfnet_amd.schedule import LrSchedule  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P_MAIN, P_E = 330499, 5161        # the 6x256 main net and the 4x40 entropy net


def _lib_ptr():
    from nsfnet_amd import _lib, engine as eng
    return _lib.load(), eng._ptr


def _vec(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(n) * 10.0 ** rng.uniform(-4, 1, size=n)).astype(np.float32)


# ---------------------------------------------------------------- the norm
@pytest.mark.parametrize("n0,n1", [(1, 0), (63, 0), (64, 0), (65, 0), (P_MAIN, 0), (P_MAIN, P_E)])
def test_sqnorm_is_within_the_reordering_bound_and_reproducible(n0, n1):
    """Relative error against the fp64 numpy sum at most n 2^-53, the reordering bound of an fp64 sum of n exact
    non-negative terms.  The two vectors are views of one buffer, as the engine's grads and grads_e are: the second one
    is not 16-byte aligned."""
    from nsfnet_amd import engine as eng
    n = n0 + n1
    host = _vec(n + 3, seed=n)
    host[n:] = np.nan                                       # nothing past the vectors may be read into the result
    flat = torch.tensor(host, device=DEV)
    g0, g1 = flat[:n0], (flat[n0:n] if n1 else None)
    scratch = eng.grad_sqnorm_scratch(DEV)
    runs = []
    for _ in range(2):
        eng.grad_sqnorm(g0, g1, scratch)
        torch.cuda.synchronize()
        s = scratch.cpu().numpy()
        assert s[1] == 0.0                                  # the ticket is 0 between calls
        runs.append(s[0])
    want = float(np.sum(host[:n].astype(np.float64) ** 2))
    rel = abs(runs[0] - want) / want
    print("n=%d+%d rel err %.3e (bound %.3e)" % (n0, n1, rel, n * 2.0 ** -53))
    assert rel <= n * 2.0 ** -53
    assert runs[0].tobytes() == runs[1].tobytes()


@pytest.mark.parametrize("n0,n1", [(1, 0), (63, 0), (64, 0), (65, 0), (P_MAIN, 0), (P_MAIN, P_E)])
def test_sqnorm_equals_the_fold_model_bit_for_bit(n0, n1):
    """The sum is the folds of csrc/fixed_fold.h in their fixed order: 256 threads x 4 entries per block, at most 256
    blocks per vector, vector 0's blocks numbered before vector 1's.  Equal to tests/fold_model.py bit for bit."""
    from nsfnet_amd import engine as eng
    n = n0 + n1
    host = _vec(n + 3, seed=n)
    flat = torch.tensor(host, device=DEV)
    scratch = eng.grad_sqnorm_scratch(DEV)
    eng.grad_sqnorm(flat[:n0], flat[n0:n] if n1 else None, scratch)
    torch.cuda.synchronize()
    got = scratch[0].item()
    sq = host[:n].astype(np.float64) ** 2
    parts = [fm.grid_partials(v, min(-(-v.size // 1024), 256)) for v in (sq[:n0], sq[n0:]) if v.size]
    want = fm.strided_tree_fold(np.concatenate(parts)[:, None], [fm.SUM])[0]
    print("n=%d+%d device %r model %r numpy %r" % (n0, n1, got, want, float(np.sum(sq))))
    assert fm.same_bits(got, want), (got, want)


@pytest.mark.parametrize("n0,n1,where", [(65, 0, 64), (P_MAIN, P_E, 1234), (P_MAIN, P_E, P_MAIN + P_E - 1)])
def test_sqnorm_propagates_a_nan(n0, n1, where):
    from nsfnet_amd import engine as eng
    host = _vec(n0 + n1, seed=3)
    host[where] = np.nan
    flat = torch.tensor(host, device=DEV)
    scratch = eng.grad_sqnorm_scratch(DEV)
    eng.grad_sqnorm(flat[:n0], flat[n0:] if n1 else None, scratch)
    torch.cuda.synchronize()
    assert np.isnan(scratch[0].item()) and scratch[1].item() == 0.0


# ---------------------------------------------------------------- the update
class _Net:
    """Parameters, moments and counters of one flat vector on the device."""

    def __init__(self, n, seed):
        rng = np.random.RandomState(seed)
        self.n = n
        self.p = torch.tensor(rng.randn(n).astype(np.float32), device=DEV)
        self.m = torch.tensor((0.1 * rng.randn(n)).astype(np.float32), device=DEV)
        self.v = torch.tensor((0.01 * rng.rand(n)).astype(np.float32), device=DEV)
        self.t = torch.tensor([4, 0], dtype=torch.int64, device=DEV)         # four updates made already

    def clone(self):
        c = _Net.__new__(_Net)
        c.n = self.n
        c.p, c.m, c.v, c.t = (x.clone() for x in (self.p, self.m, self.v, self.t))
        return c

    def state(self):
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (self.p, self.m, self.v, self.t)]


def _sched_step(net, g, spec, lr0, epoch, rec, sq=None, max_norm=0.0, advance=1):
    lib, ptr = _lib_ptr()
    from nsfnet_amd import _lib
    st = spec.c_struct()
    _lib.check(lib.pinn_adam_step_sched(ptr(net.p), ptr(g), ptr(net.m), ptr(net.v), net.n, ctypes.byref(st), lr0, 0.9,
                                        0.999, 1e-8, ptr(net.t), ptr(epoch), advance, ptr(sq), max_norm, ptr(rec),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pinn_adam_step_sched")


def _dev_step(net, g, lr):
    lib, ptr = _lib_ptr()
    from nsfnet_amd import _lib
    _lib.check(lib.pinn_adam_step_dev(ptr(net.p), ptr(g), ptr(net.m), ptr(net.v), net.n, lr, 0.9, 0.999, 1e-8, ptr(net.t),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pinn_adam_step_dev")


SPECS = [LrSchedule(),
         LrSchedule("multistep", milestones=(300, 1000, 1000, 2500), gamma=0.3),
         LrSchedule("step", step_size=700, gamma=0.5),
         LrSchedule("exponential", gamma=0.999),
         LrSchedule("cosine", t_max=2500, eta_min=1e-6),
         LrSchedule("cosine", t_max=2500, eta_min=1e-6, warmup_epochs=100, warmup_start=0.1),
         LrSchedule("exponential", gamma=0.999, warmup_epochs=50)]
EPOCHS = [0, 1, 37, 99, 100, 299, 300, 700, 1000, 1399, 2499, 2500, 2999, 20000]


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s.kind + ("+warmup" if s.warmup_epochs else ""))
@pytest.mark.parametrize("clip", [False, True])
def test_update_is_adam_step_dev_with_the_recorded_lr_and_coefficient(spec, clip):
    """At several epochs, set through the counter: the recorded lr_e is within one fp32 ulp of the model's (the
    device's fp64 pow and cos may differ from libm's in the last place before the rounding), the recorded coefficient
    likewise, and params / m / v / t are bit-identical to pinn_adam_step_dev with the RECORDED lr on grads times the
    RECORDED coefficient (the fp32 multiply done by torch).  The gradient buffer is not written."""
    from nsfnet_amd import engine as eng
    lr0, n = 1e-3, 5161
    g = torch.tensor(_vec(n, seed=11), device=DEV)
    g_host = g.cpu().numpy().copy()
    sq_model = om.sqnorm(g_host)
    max_norm = 0.25 * np.sqrt(sq_model)
    scratch = eng.grad_sqnorm_scratch(DEV)
    if clip:
        eng.grad_sqnorm(g, None, scratch)
    rec = torch.zeros(om.RECORD, dtype=torch.float64, device=DEV)
    epoch = torch.zeros(1, dtype=torch.int64, device=DEV)
    for k, e in enumerate(EPOCHS):
        a = _Net(n, seed=e)
        b = a.clone()
        epoch.fill_(e)
        _sched_step(a, g, spec, lr0, epoch, rec, scratch if clip else None, max_norm)
        torch.cuda.synchronize()
        r = rec.cpu().numpy()
        want = om.lr_e(lr0, e, **dataclasses.asdict(spec))
        assert r[om.R_EPOCH] == e and int(epoch.item()) == e + 1
        assert r[om.R_LR] == float(np.float32(r[om.R_LR]))                      # an fp32 value
        assert abs(r[om.R_LR] - want) <= 2.0 ** -23 * abs(want), (e, r[om.R_LR], want)
        if spec == LrSchedule():
            assert r[om.R_LR] == float(np.float32(lr0))
        if clip:
            norm, coef = om.clip(sq_model, max_norm)
            assert abs(r[om.R_NORM] - norm) <= 2.0 ** -40 * norm and abs(r[om.R_COEF] - float(coef)) <= 2.0 ** -23 * coef
            assert r[om.R_COEF] < 1.0 and r[om.R_CLIPPED] == k + 1
            gs = g * torch.tensor(r[om.R_COEF], dtype=torch.float32, device=DEV)
        else:
            assert r[om.R_NORM] == 0.0 and r[om.R_COEF] == 1.0 and r[om.R_CLIPPED] == 0
            gs = g
        assert r[om.R_UPDATES] == k + 1
        _dev_step(b, gs, r[om.R_LR])
        for x, y in zip(a.state(), b.state()):
            np.testing.assert_array_equal(x, y)
        assert a.state()[3].tolist() == [5, 0]                                  # t advanced, the ticket is 0
    np.testing.assert_array_equal(g.cpu().numpy(), g_host)


def test_constant_schedule_without_clipping_is_adam_step_dev_bitwise():
    n = P_MAIN
    a = _Net(n, seed=1)
    a.t.zero_()
    b = a.clone()
    rec = torch.zeros(om.RECORD, dtype=torch.float64, device=DEV)
    epoch = torch.zeros(1, dtype=torch.int64, device=DEV)
    for k in range(4):
        g = torch.tensor(_vec(n, seed=20 + k), device=DEV)
        _sched_step(a, g, LrSchedule(), 1e-3, epoch, rec)
        _dev_step(b, g, 1e-3)
        for x, y in zip(a.state(), b.state()):
            np.testing.assert_array_equal(x, y)
    assert rec[om.R_LR].item() == float(np.float32(1e-3)) and epoch.item() == 4


def test_counters_advance_once_per_step_and_advance_zero_holds_the_epoch():
    """Two nets per step, as the ev flavour launches them: the entropy net with advance = 0 first, the main net with
    advance = 1 last.  Both use the lr_e of the same epoch; after k steps epoch = k and both Adam counters = k."""
    spec = LrSchedule("exponential", gamma=0.5)
    main, ent = _Net(3000, seed=1), _Net(200, seed=2)
    main.t.zero_(); ent.t.zero_()
    rec = torch.zeros(om.RECORD, dtype=torch.float64, device=DEV)
    epoch = torch.zeros(1, dtype=torch.int64, device=DEV)
    g, ge = torch.tensor(_vec(3000, 3), device=DEV), torch.tensor(_vec(200, 4), device=DEV)
    for k in range(5):
        _sched_step(ent, ge, spec, 1e-3, epoch, rec, advance=0)
        torch.cuda.synchronize()
        r = rec.cpu().numpy()
        assert epoch.item() == k and r[om.R_EPOCH] == k and r[om.R_UPDATES] == k      # held; not counted
        lr_e_net = r[om.R_LR]
        _sched_step(main, g, spec, 1e-3, epoch, rec, advance=1)
        torch.cuda.synchronize()
        r = rec.cpu().numpy()
        assert epoch.item() == k + 1 and r[om.R_EPOCH] == k and r[om.R_LR] == lr_e_net == float(np.float32(1e-3 * 0.5 ** k))
        assert r[om.R_UPDATES] == k + 1
        assert main.t.tolist() == [k + 1, 0] and ent.t.tolist() == [k + 1, 0]


def test_matches_torch_adam_cosine_and_clip_grad_norm():
    """20 steps against torch.optim.Adam + CosineAnnealingLR + clip_grad_norm_ on a (main, entropy net) pair, at the
    tolerance of test_hip_kernels.test_adam_matches_torch."""
    from nsfnet_amd import engine as eng
    n0, n1, lr0, max_norm = 4000, 300, 1e-3, 5.0
    torch.manual_seed(0)
    p0, p1 = torch.randn(n0), torch.randn(n1)
    refs = [p0.clone().requires_grad_(True), p1.clone().requires_grad_(True)]
    opt = torch.optim.Adam(refs, lr=lr0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=15, eta_min=1e-5)
    spec = LrSchedule("cosine", t_max=15, eta_min=1e-5)
    nets = [_Net(n0, 1), _Net(n1, 2)]
    for net, p in zip(nets, (p0, p1)):
        net.p.copy_(p); net.m.zero_(); net.v.zero_(); net.t.zero_()
    flat = torch.zeros(n0 + n1, device=DEV)
    scratch = eng.grad_sqnorm_scratch(DEV)
    rec = torch.zeros(om.RECORD, dtype=torch.float64, device=DEV)
    epoch = torch.zeros(1, dtype=torch.int64, device=DEV)
    clipped = 0
    for k in range(20):
        gs = [torch.randn(n0) * (10.0 ** (-(k % 4))), torch.randn(n1) * (10.0 ** (-(k % 4)))]
        for r, g in zip(refs, gs):
            r.grad = g.clone()
        total = float(torch.nn.utils.clip_grad_norm_(refs, max_norm))
        opt.step()
        sched.step()
        flat.copy_(torch.cat(gs))
        eng.grad_sqnorm(flat[:n0], flat[n0:], scratch)
        _sched_step(nets[1], flat[n0:], spec, lr0, epoch, rec, scratch, max_norm, advance=0)
        _sched_step(nets[0], flat[:n0], spec, lr0, epoch, rec, scratch, max_norm, advance=1)
        torch.cuda.synchronize()
        r = rec.cpu().numpy()
        np.testing.assert_allclose(r[om.R_NORM], total, rtol=1e-6)
        clipped += total > max_norm
        for net, ref in zip(nets, refs):
            np.testing.assert_allclose(net.p.cpu().numpy(), ref.detach().numpy(), rtol=2e-6, atol=1e-8)
    assert 0 < clipped < 20 and rec[om.R_CLIPPED].item() == clipped and epoch.item() == 20


# ---------------------------------------------------------------- the whole step
def _bc(every=16):
    return tuple(a.reshape(-1)[::every].astype(np.float32) for a in ar.cavity_boundary())


def _engine(flavour, L, H, x, y, seed=5):
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=2, hidden_e=24, alpha_evm=0.05) if flavour == "ev" else {}
    E = eng.PinnEngine(DEV, L, H, 2000.0, alpha_b=10.0, alpha_e=1.0, precision="fp32", **ev)
    E.net.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().copy()))
    if flavour == "ev":
        E.net_e.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(1, 2, 24, seed=seed + 1)).numpy().copy()))
        E.e_trainable = True                                 # both nets take the scheduled, clipped update
    E.set_collocation(x, y)
    E.set_boundary(*_bc())
    return E


def _state(E):
    torch.cuda.synchronize()
    out = [E.net.params, E.net.m, E.net.v, E.net.adam_t_dev]
    if E.net_e is not None:
        out += [E.net_e.params, E.net_e.m, E.net_e.v, E.net_e.adam_t_dev, E.plan_f.vis_t_minus]
    return [t.cpu().numpy().copy() for t in out]


@pytest.mark.parametrize("batch", [0, 500], ids=["full", "minibatch"])
@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_graph_replay_is_bit_identical_to_eager_with_one_graph_for_the_stage(flavour, batch, monkeypatch):
    """40 eager steps against one eager step (the capture) and 39 replays under a cosine schedule with warm-up and a
    clipping bound below the first gradient's norm: bit-identical state, ONE captured graph although lr_e differs on
    every step, and the same optimizer_info()."""
    N, L, H, steps, lr0 = 2000, 3, 24, 40, 1e-3
    rng = np.random.RandomState(5)
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    spec = LrSchedule("cosine", t_max=steps, eta_min=1e-5, warmup_epochs=5, warmup_start=0.1)
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    probe = _engine(flavour, L, H, x, y)
    probe.loss_and_grad()
    torch.cuda.synchronize()
    max_norm = 0.7 * float(np.sqrt(om.sqnorm(probe.grads.cpu().numpy(), probe.grads_e.cpu().numpy())))

    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E = _engine(flavour, L, H, x, y)
        if batch:
            E.set_batching(batch, seed=3)
        E.set_lr_schedule(spec)
        E.set_grad_clipping(max_norm)
        lrs = []
        for _ in range(steps):
            E.step(lr0)
            if not graph:
                lrs.append(E.optimizer_info()["lr"])
        assert len(E._graphs) == (1 if graph else 0)
        return _state(E), E.optimizer_info(), lrs

    (eager, info_e, lrs), (graph, info_g, _) = run(False), run(True)
    for a, b in zip(eager, graph):
        np.testing.assert_array_equal(a, b)
    assert info_e == info_g
    print("optimizer_info:", info_e)
    assert info_e["epoch"] == steps - 1 and info_e["next_epoch"] == steps and info_e["updates"] == steps
    assert 0 < info_e["clipped"] <= steps
    assert eager[3].tolist() == [steps, 0]
    for k, lr in enumerate(lrs):                                        # every step had its own rate
        want = spec.value(lr0, k)
        assert abs(lr - want) <= 2.0 ** -23 * want
    assert len(set(lrs)) > steps // 2
