"""Round-3 regression tests for the advisor's findings on the role-split (schedule 2) path:
 * two live plans that share a kernel instantiation but differ in depth must not lower each other's dynamic-LDS limit;
 * gradient parity of the DEFAULT path (24-bit spill of tanh, layer 0 recomputed) on TRAINED 6x256 weights, against the
   fp64 oracle and against the fp32-spill 8-wave kernels (schedule 0);
 * mixed schedules (pipelined forward + 8-wave reverse sweep and the reverse) agree with schedule 0: the fp32 S layout and
   its layer-0 slot are shared between them."""
import os

import numpy as np
import pytest
import torch

from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1); b = np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _engine(L, H, N, prec, seed, Re=1500.0):
    from nsfnet_amd import engine as eng
    dev = torch.device("cuda:0")
    flat = ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().copy()
    rng = np.random.RandomState(seed)
    x = rng.rand(N).astype(np.float32); y = rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())
    E = eng.PinnEngine(dev, L, H, Re, alpha_b=10.0, alpha_e=1.0, precision=prec)
    E.net.set_flat(torch.tensor(flat))
    E.set_collocation(x, y)
    E.set_boundary(xb, yb, ub, vb)
    return E, flat, x, y, (xb, yb, ub, vb)


def _oracle_grad(flat, L, H, x, y, bc, Re):
    P = fr.unflatten(flat.astype(np.float64), 2, 3, L, H)
    r = fr.pde_loss_and_grad(P, x.astype(np.float64), y.astype(np.float64), Re, alpha_e=1.0)
    b = fr.bc_loss_and_grad(P, *(a.astype(np.float64) for a in bc), alpha_b=10.0)
    return r["grad"] + b["grad"]


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_deep_plan_survives_a_shallow_plan_of_the_same_width(monkeypatch, prec):
    """A 7x256 plan, THEN a 2x256 plan of the same kernel instantiations (their dynamic LDS differs only through the
    run-time depth), then a launch of the first: the limit is the device maximum for every plan (layout.h PINN_LDS_MAX)."""
    for k in ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED"):
        monkeypatch.delenv(k, raising=False)
    deep, flat, x, y, bc = _engine(7, 256, 700, prec, 7)
    shallow, *_ = _engine(2, 256, 700, prec, 8)
    shallow.loss_and_grad()
    deep.loss_and_grad()
    torch.cuda.synchronize()
    g = deep.grads.cpu().numpy()
    assert np.isfinite(g).all()
    assert _rel_l2(g, _oracle_grad(flat, 7, 256, x, y, bc, 1500.0)) < 1e-4


def test_default_path_gradient_on_trained_6x256_weights(monkeypatch):
    """tests/golden/trained/ev_re2000_6x256_net.pth (1.16 M Adam steps of this engine at the headline shape, 3.3 % vs DNS):
    saturated tanh units make d1 = 1 - t^2 sensitive to the 24-bit rounding of the spilled t.  Gradient of the plain
    NS loss at these weights, half the sample in the lid corners: schedule 2 (24-bit spill) against the fp64 oracle and
    against schedule 0 (fp32 spill)."""
    from nsfnet_amd import engine as eng
    dev = torch.device("cuda:0")
    L, H, N, Re = 6, 256, 2048, 2000.0
    sd = torch.load(os.path.join(HERE, "golden", "trained", "ev_re2000_6x256_net.pth"), weights_only=True)
    rng = np.random.RandomState(11)
    x = np.concatenate([rng.rand(N // 2), np.clip(rng.rand(N // 2) ** 4, 1e-4, 1)]).astype(np.float32)
    y = np.concatenate([rng.rand(N // 2), 1.0 - np.clip(rng.rand(N // 2) ** 4 * 0.2, 1e-4, 1)]).astype(np.float32)
    bc = tuple(a.reshape(-1).astype(np.float32) for a in ar.cavity_boundary())
    grads = {}
    for sched in ("2", "0"):
        monkeypatch.setenv("PINN_SCHED", sched)
        E = eng.PinnEngine(dev, L, H, Re, alpha_b=10.0, alpha_e=1.0, precision="bf16x3")
        E.net.load_state_dict(sd)
        E.set_collocation(x, y); E.set_boundary(*bc)
        assert E.plan_f.kernel_names()[0] == ("fwd_split_kernel" if sched == "2" else "fwd_bf16_kernel")
        E.loss_and_grad()
        torch.cuda.synchronize()
        grads[sched] = E.grads.cpu().numpy().astype(np.float64)
        flat = E.net.params.cpu().numpy().copy()
    ref = _oracle_grad(flat, L, H, x, y, bc, Re)
    e2, e0 = _rel_l2(grads["2"], ref), _rel_l2(grads["0"], ref)
    print("trained 6x256 gradient rel-L2 vs fp64: schedule 2 (24-bit spill) %.3e, schedule 0 (fp32 spill) %.3e, 2 vs 0 %.3e"
          % (e2, e0, _rel_l2(grads["2"], grads["0"])))
    # the bf16x3 bar on trained weights (tests/test_supervised_and_configs.py: 1e-3; fresh-init nets sit at 3e-6), and
    # the 24-bit spill must not cost more than a factor two over the fp32 spill
    assert e2 < 1e-3 and e0 < 1e-3
    assert e2 < 2.0 * e0 + 1e-5


@pytest.mark.parametrize("fs,bs", [("1", "0"), ("0", "1")])
def test_mixed_schedules_share_the_fp32_spill_layout(monkeypatch, fs, bs):
    """PINN_FWD_SCHED / PINN_BWD_SCHED mixed: a pipelined forward feeds the 8-wave reverse sweep and dW (and the reverse)
    through the same fp32 S blocks, layer-0 slot included."""
    out = {}
    for tag, (f, b) in {"mixed": (fs, bs), "ref": ("0", "0")}.items():
        monkeypatch.setenv("PINN_FWD_SCHED", f); monkeypatch.setenv("PINN_BWD_SCHED", b)
        monkeypatch.delenv("PINN_SCHED", raising=False)
        E, flat, x, y, bc = _engine(5, 256, 333, "bf16x3", 21)
        names = E.plan_f.kernel_names()
        if tag == "mixed":
            assert names[0] == ("fwd_pipe_kernel" if fs == "1" else "fwd_bf16_kernel")
            assert names[1] == ("bwd_pipe_kernel" if bs == "1" else "bwd_bf16_kernel")
        E.loss_and_grad()
        torch.cuda.synchronize()
        out[tag] = E.grads.cpu().numpy().astype(np.float64)
    assert _rel_l2(out["mixed"], out["ref"]) < 1e-4
    assert _rel_l2(out["mixed"], _oracle_grad(flat, 5, 256, x, y, bc, 1500.0)) < 1e-4


@pytest.mark.parametrize("H,L,N", [(128, 4, 333), (256, 3, 150), (50, 2, 40)])
def test_fp32_layer0_recompute_matches_the_spilled_version(monkeypatch, H, L, N):
    """fp32 mode does not spill layer 0 (Spill::skip0): the reverse sweep and the layer-1 workgroups of the dW kernel
    recompute (tanh(w0x x + w0y y + b0), w0x, w0y, 0) with the forward's own fmaf chain and tanhf.  The loss sums (forward
    only) must be BITWISE those of the spilled version ($PINN_S0_SKIP32=0); the gradient agrees to fp32 rounding (the
    compiler specialises the layer-0 epilogue for z_D = 0 and contracts a few products differently), in the narrow and in
    the 64-column fp32 kernels."""
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("PINN_S0_SKIP32", flag)
        E, flat, x, y, bc = _engine(L, H, N, "fp32", 31)
        E.loss_and_grad()
        torch.cuda.synchronize()
        out[flag] = (E.grads.cpu().numpy().copy(), E.sums.cpu().numpy().copy())
    assert np.array_equal(out["1"][1], out["0"][1])
    d = _rel_l2(out["1"][0], out["0"][0])
    print("fp32 layer-0 recompute vs spill: gradient rel-L2 difference %.2e" % d)
    assert d < 1e-6
    ref = _oracle_grad(flat, L, H, x, y, bc, 1500.0)
    assert _rel_l2(out["1"][0], ref) < 1e-5 and _rel_l2(out["0"][0], ref) < 1e-5


def test_rccl_moves_the_exchange_buffer_on_this_gpu(tmp_path):
    """One lease has one GPU, so the N > 1 step (ONE all-reduce of [grads | grads_e | 24 sums], engine.py) runs under gloo
    in the rank-logic tests.  What CAN run here is RCCL itself: a one-rank "nccl" group (= RCCL on ROCm) created the way
    bench.py creates it (device_id), all-reducing the engine's real exchange buffer on the launch stream behind the
    kernels that fill it.  SUM over one rank must return the buffer unchanged; the point is that RCCL initialises and
    launches on this box and that the buffer is a valid RCCL operand (contiguous fp32, device memory of this process)."""
    import subprocess, sys, textwrap
    script = tmp_path / "rccl_one_rank.py"
    script.write_text(textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r)
        import numpy as np, torch, torch.distributed as dist
        from nsfnet_amd import engine as eng
        from oracle import autograd_ref as ar
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:29731", rank=0, world_size=1, device_id=dev)
        E = eng.PinnEngine(dev, 3, 64, 1000.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3", process_group=dist.group.WORLD, world_size=1)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, 3, 64, seed=5)))
        rng = np.random.RandomState(0)
        E.set_collocation(rng.rand(500).astype(np.float32), rng.rand(500).astype(np.float32))
        xb, yb, ub, vb = (a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())
        E.set_boundary(xb, yb, ub, vb)
        E.loss_and_grad()
        before = E.flat.clone()
        dist.all_reduce(E.flat, group=E.pg)          # the call the step makes when world_size > 1
        torch.cuda.synchronize()
        assert torch.equal(before, E.flat) and bool(torch.isfinite(E.flat).all())
        print("RCCL_OK", dist.get_backend(), E.flat.numel())
        dist.destroy_process_group()
    """ % os.path.dirname(HERE)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "RCCL_OK nccl" in out.stdout
