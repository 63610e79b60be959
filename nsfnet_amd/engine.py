"""Host-side driver of the HIP PINN pipeline (one process = one GPU).

PyTorch is plumbing here: it owns device memory, the stream and (for N > 1 GPUs) the
RCCL communicator.  All arithmetic of the training step happens in
lib/libnsfnet_pinn.so through the C ABI of include/nsfnet_pinn.h.

The step implemented is the reference's solve_Adam loop body
(NSFnet/pinn_solver.py:250-254, ev-NSFnet/pinn_solver.py:456-472):
loss (BC MSE + PDE residual MSE [+ supervised MSE]) -> d loss/d theta -> Adam.
"""
import contextlib
import ctypes
import json
import math
import os
import threading
import time

import numpy as np
import torch

from . import _lib
from . import lbfgs as _lbfgs
from . import schedule as _schedule
from . import state_file as _state_file
from .state_file import StateFileError

NLOSS = 8
FLD = dict(u=0, v=1, u_x=2, u_y=3, v_x=4, v_y=5, eq1=6, eq2=7, eq3=8, eq4=9, p=10)
FLD_COUNT = 11

# slots of the per-step sums vector (all-reduced together with the gradients)
# (three blocks of NLOSS, each written whole by one loss-sum launch: no per-step zeroing or copies)
S_EQ = 0        # 0..3   sum w*eq_k^2
S_BC = 8        # 8,9    sum (u-u_b)^2, sum (v-v_b)^2
S_SUP = 16      # 16..18 sum sq err u,v,p ; 19 = number of finite p targets
NSUMS = 24


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def layer_shapes(n_out, n_hidden, hidden):
    widths = [2] + [hidden] * n_hidden + [n_out]
    return [(widths[i + 1], widths[i]) for i in range(len(widths) - 1)]


def fourier_first_layer(B):
    """(W0 fp32 [hidden, 2], b0 fp32 [hidden]) of the Fourier-feature embedding with frequencies B (fp64 [hidden / 2, 2];
    DESIGN.md section 7.13): rows 2k and 2k + 1 of W0 are fp32(2 pi B_k), the biases fp32(pi / 2) and 0, so that
    sin(W0 x + b0) is [cos(2 pi B_k x), sin(2 pi B_k x)] interleaved."""
    B = torch.as_tensor(B, dtype=torch.float64)
    w0 = (2.0 * math.pi * B).to(torch.float32).repeat_interleave(2, dim=0)
    b0 = torch.zeros(2 * B.shape[0], dtype=torch.float32)
    b0[0::2] = float(np.float32(math.pi / 2.0))
    return w0, b0


PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16": 2}


def resolve_precision(precision=None):
    """'fp32' | 'bf16x3' | 'bf16' or a (fwd, bwd, dw) triple of those; default from
    $NSFNET_PRECISION, else fp32 (the bit-exact fp32 MFMA path)."""
    if precision is None:
        precision = os.environ.get("NSFNET_PRECISION", "fp32")
    if isinstance(precision, str):
        precision = tuple(precision.split(",")) if "," in precision else (precision,) * 3
    if len(precision) != 3 or any(p not in PRECISIONS for p in precision):
        raise ValueError("precision must be one of %s (or a fwd,bwd,dw triple)" % sorted(PRECISIONS))
    return tuple(precision)


class DeviceNet:
    """One FCNet on the device: flat fp32 parameters in reference state_dict order
    (NSFnet/net.py:36-46) plus their MFMA-fragment-ordered copy.

    With the random weight factorization on (set_factorization) the trainable vector is
    theta = [params with V where W stands | s] of num_train = num_params + rwf_rows entries: the Adam entry points
    update theta (m and v have its size) with gtheta, the gradient rwf_grad makes of the effective one, and rebuild
    params from it (compose) before prepare.  params stays what prepare, state_dict and every plan read."""
    theta = gtheta = None       # the factorization is off
    hard_bc = None              # _lib.HardBcStruct: every plan of this net is created constrained (PinnEngine.set_hard_boundary)
    first_layer = 0             # 0 tanh | 1 frozen sine (set_first_layer; PinnEngine.set_fourier_features)

    def __init__(self, n_out, n_hidden, hidden, device, precision=None):
        self.lib = _lib.load()
        self.n_out, self.n_hidden, self.hidden, self.device = n_out, n_hidden, hidden, device
        self.precision = resolve_precision(precision)
        h = ctypes.c_void_p()
        _lib.check(self.lib.pinn_net_create(n_out, n_hidden, hidden, ctypes.byref(h)), "pinn_net_create")
        _lib.check(self.lib.pinn_net_set_precision(h, *[PRECISIONS[p] for p in self.precision]),
                   "pinn_net_set_precision")
        self.handle = h
        self.num_params = int(self.lib.pinn_net_num_params(h))
        self.params = torch.zeros(self.num_params, dtype=torch.float32, device=device)
        self.prep = torch.zeros(int(self.lib.pinn_net_prep_floats(h)), dtype=torch.float32, device=device)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.adam_t = 0                                                   # steps taken (host mirror)
        self.adam_t_dev = torch.zeros(2, dtype=torch.int64, device=device)   # [count, scratch] the kernel uses

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.pinn_net_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def set_first_layer(self, kind):
        """The kind of layer 0: 0 tanh, 1 the frozen sine layer of a Fourier-feature
        embedding.  It belongs to the net: every plan created from here on sees it, and the library refuses plans
        created before a change.  The weights are the caller's to set (PinnEngine.set_fourier_features does both)."""
        _lib.check(self.lib.pinn_net_set_first_layer(self.handle, int(kind)), "pinn_net_set_first_layer")
        self.first_layer = int(self.lib.pinn_net_first_layer(self.handle))

    # ---- state_dict interop (checkpoint format of the reference) ----
    def keys_and_shapes(self):
        out = []
        for i, (o, k) in enumerate(layer_shapes(self.n_out, self.n_hidden, self.hidden)):
            out.append(("layers.layer_%d.weight" % i, (o, k)))
            out.append(("layers.layer_%d.bias" % i, (o,)))
        return out

    def load_state_dict(self, sd):
        flat = []
        for key, shape in self.keys_and_shapes():
            t = sd[key]
            if tuple(t.shape) != tuple(shape):
                raise ValueError("state_dict[%s] has shape %s, expected %s" % (key, tuple(t.shape), shape))
            flat.append(t.detach().to(torch.float32).reshape(-1).cpu())
        self.set_flat(torch.cat(flat))

    def state_dict(self):
        return self.flat_state_dict(self.params)

    def set_flat(self, flat):
        flat = torch.as_tensor(flat, dtype=torch.float32).reshape(-1)
        if flat.numel() != self.num_params:
            raise ValueError("expected %d parameters, got %d" % (self.num_params, flat.numel()))
        self.params.copy_(flat.to(self.device))
        if self.theta is not None:      # params is exactly what was given; V follows from it and the current s
            self._rwf_split(self.theta[self.num_params:].clone())
        self.prepare()

    # ---- random weight factorization ----
    @property
    def rwf_rows(self):
        """Number of scale factors: one per row of every Linear layer."""
        return self.n_hidden * self.hidden + self.n_out

    @property
    def num_train(self):
        """Entries of the vector the optimizers update."""
        return self.num_params + (self.rwf_rows if self.theta is not None else 0)

    @property
    def trainable(self):
        """The vector the optimizers update: theta with the factorization on, else params."""
        return self.params if self.theta is None else self.theta

    def set_factorization(self, s):
        """s = fp32 [rwf_rows] (layers ascending, rows ascending): theta = split(params, s); params itself is not
        rewritten before the first update.  None: off (params stays as composed).  Either way Adam starts afresh, with
        moments of the trainable vector's size."""
        if s is None:
            self.theta = self.gtheta = None
        else:
            s = torch.as_tensor(s, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            if s.numel() != self.rwf_rows:
                raise ValueError("expected %d scale factors, got %d" % (self.rwf_rows, s.numel()))
            n = self.num_params + self.rwf_rows
            self.theta = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.gtheta = torch.zeros(n, dtype=torch.float32, device=self.device)
            self._rwf_split(s)
        self.m = torch.zeros_like(self.trainable)
        self.v = torch.zeros_like(self.trainable)
        self.reset_adam()

    def _rwf_split(self, s):
        _lib.check(self.lib.pinn_rwf_split(self.handle, _ptr(self.params), _ptr(s), _ptr(self.theta), _stream()),
                   "pinn_rwf_split")

    def compose(self):
        """params = the effective weights of theta."""
        _lib.check(self.lib.pinn_rwf_compose(self.handle, _ptr(self.theta), _ptr(self.params), _stream()),
                   "pinn_rwf_compose")

    def composed(self, x):
        """The effective weights (a fresh tensor like params) of x, a vector like the trainable one."""
        if self.theta is None:
            return x.clone()
        out = torch.empty_like(self.params)
        _lib.check(self.lib.pinn_rwf_compose(self.handle, _ptr(x), _ptr(out), _stream()), "pinn_rwf_compose")
        return out

    def flat_state_dict(self, flat):
        """flat (a vector like params) in the checkpoint format of state_dict."""
        sd, off = {}, 0
        flat = flat.detach().cpu()
        for key, shape in self.keys_and_shapes():
            n = int(np.prod(shape))
            sd[key] = flat[off:off + n].reshape(shape).clone()
            off += n
        return sd

    def rwf_grad(self, grads):
        """gtheta = d loss / d theta from the effective gradient; returns it."""
        _lib.check(self.lib.pinn_rwf_grad(self.handle, _ptr(self.theta), _ptr(grads), _ptr(self.gtheta), _stream()),
                   "pinn_rwf_grad")
        return self.gtheta

    def factors(self):
        """The per-layer scale factors s as views of theta (updated in place); None when off."""
        if self.theta is None:
            return None
        out, off = [], self.num_params
        for rows, _ in layer_shapes(self.n_out, self.n_hidden, self.hidden):
            out.append(self.theta[off:off + rows])
            off += rows
        return out

    def update_params(self):
        """After an update of the trainable vector: compose (factorization on) and re-layout."""
        if self.theta is not None:
            self.compose()
        self.prepare()

    def prepare(self):
        _lib.check(self.lib.pinn_net_prepare(self.handle, _ptr(self.params), _ptr(self.prep), _stream()),
                   "pinn_net_prepare")

    def reset_adam(self):
        self.m.zero_(); self.v.zero_(); self.adam_t = 0
        self.adam_t_dev.zero_()

    def adam_step(self, grads, lr, betas=(0.9, 0.999), eps=1e-8):
        """One Adam update + weight re-layout.  The step count lives on the device so the call is
        identical every step (hipGraph-capturable).  Factorization on: grads is gtheta, the update is theta's."""
        self.adam_t += 1
        x = self.trainable
        _lib.check(self.lib.pinn_adam_step_dev(_ptr(x), _ptr(grads), _ptr(self.m), _ptr(self.v),
                                               x.numel(), lr, betas[0], betas[1], eps,
                                               _ptr(self.adam_t_dev), _stream()), "pinn_adam_step_dev")
        self.update_params()

    def adam_step_sched(self, grads, lr0, opt, advance, betas=(0.9, 0.999), eps=1e-8):
        """adam_step with the learning rate of the device epoch counter opt.epoch under opt's schedule (lr0 = its
        base rate) and, when opt.max_norm > 0, the gradient scaled by the clipping coefficient of the squared norm in
        opt.scratch (pinn_adam_step_sched).  advance: this call moves the epoch counter on."""
        self.adam_t += 1
        x = self.trainable
        _lib.check(self.lib.pinn_adam_step_sched(
            _ptr(x), _ptr(grads), _ptr(self.m), _ptr(self.v), x.numel(), ctypes.byref(opt.cstruct),
            float(lr0), betas[0], betas[1], eps, _ptr(self.adam_t_dev), _ptr(opt.epoch), 1 if advance else 0,
            _ptr(opt.scratch if opt.max_norm > 0.0 else None), float(opt.max_norm), _ptr(opt.rec), _stream()),
            "pinn_adam_step_sched")
        self.update_params()


class PointPlan:
    """A fixed set of points evaluated by one DeviceNet (residual or value mode)."""

    def __init__(self, net, x, y, streams, with_backward=True, ws=None, pseudo_time=False):
        self.lib, self.net, self.streams = net.lib, net, streams
        dev = net.device
        self.x = torch.as_tensor(np.asarray(x, dtype=np.float32).reshape(-1)).to(dev).contiguous()
        self.y = torch.as_tensor(np.asarray(y, dtype=np.float32).reshape(-1)).to(dev).contiguous()
        self.n = self.x.numel()
        if self.y.numel() != self.n or self.n == 0:
            raise ValueError("x and y must be non-empty and of equal length")
        h = ctypes.c_void_p()
        bc = getattr(net, "hard_bc", None)
        if pseudo_time:     # pseudo-time stepping, with or without hard walls
            _lib.check(self.lib.pinn_plan_create_pseudo_time(net.handle, self.n, None if bc is None else ctypes.byref(bc),
                                                             ctypes.byref(h)), "pinn_plan_create_pseudo_time")
        elif bc is None:
            _lib.check(self.lib.pinn_plan_create(net.handle, self.n, streams, ctypes.byref(h)), "pinn_plan_create")
        else:       # hard wall conditions
            _lib.check(self.lib.pinn_plan_create_constrained(net.handle, self.n, streams, ctypes.byref(bc), ctypes.byref(h)),
                       "pinn_plan_create_constrained")
        self.handle = h
        self.npad = int(self.lib.pinn_plan_padded_points(h))
        self.with_backward = with_backward
        nbytes = int(self.lib.pinn_plan_workspace_bytes(h, 1 if with_backward else 0))
        if ws is not None and ws.numel() < nbytes:
            raise ValueError("shared workspace too small: %d < %d bytes" % (ws.numel(), nbytes))
        self.ws = ws if ws is not None else torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        self.sums = torch.zeros(NLOSS, dtype=torch.float32, device=dev)

    def hard_bc(self):
        """The hard wall conditions the plan carries, as dict(kind, lift_power, x0, y0, inv_len, lid_sharpness); None for
        an unconstrained plan."""
        bc = _lib.HardBcStruct()
        _lib.check(self.lib.pinn_plan_hard_bc(self.handle, ctypes.byref(bc)), "pinn_plan_hard_bc")
        return None if bc.kind == 0 else {name: getattr(bc, name) for name, _ in bc._fields_}

    def kernel_names(self):
        """(forward, reverse sweep, weight-gradient) kernel family names this plan launches (for profiling)."""
        return tuple((self.lib.pinn_plan_kernel(self.handle, k) or b"").decode() for k in (0, 1, 2))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.pinn_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class ResidualPlan(PointPlan):
    def __init__(self, net, x, y, weights=None, with_backward=True, ws=None, pseudo_time=False):
        super().__init__(net, x, y, 4, with_backward, ws, pseudo_time)
        dev = net.device
        self.anchor = None          # [3, npad] anchors u*, v*, p* of a pseudo-time plan (set_pseudo_time)
        self.fields = torch.zeros(FLD_COUNT, self.npad, dtype=torch.float32, device=dev)
        self.w = None if weights is None else torch.as_tensor(
            np.asarray(weights, dtype=np.float32).reshape(-1)).to(dev).contiguous()
        if self.w is not None and self.w.numel() != self.n:
            raise ValueError("weights must have one entry per collocation point")
        self.vis_t = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.vis_t_minus = None     # lagged alpha_evm*|e| state (ev flavour)
        self.ebar = None

    def forward(self, Re, e=None, vis_t0=0.0, alpha_evm=0.0, scale=1.0, save=True, sums_out=None):
        if save and not self.with_backward:
            raise RuntimeError("plan was created without backward workspace")
        _lib.check(self.lib.pinn_residual_forward(
            self.handle, _ptr(self.ws), _ptr(self.net.prep), _ptr(self.x), _ptr(self.y), _ptr(e), _ptr(self.w),
            _ptr(self.vis_t_minus), _ptr(self.vis_t), _ptr(self.fields), float(Re), float(vis_t0),
            float(alpha_evm), float(scale), 1 if save else 0,
            _ptr(self.sums if sums_out is None else sums_out), _stream()), "pinn_residual_forward")

    def backward(self, Re, coef_eq, e=None, scale=1.0, want_ebar=False, phases=3):
        if want_ebar and self.ebar is None:
            self.ebar = torch.zeros(((self.n + 127) // 128) * 128, dtype=torch.float32, device=self.net.device)
        coef = (ctypes.c_float * 4)(*[float(c) for c in coef_eq])
        _lib.check(self.lib.pinn_residual_backward_phases(
            self.handle, _ptr(self.ws), _ptr(self.net.prep), _ptr(self.x), _ptr(self.y), _ptr(e), _ptr(self.w),
            _ptr(self.vis_t), _ptr(self.fields), coef, float(Re), float(scale),
            _ptr(self.ebar if want_ebar else None), int(phases), _stream()), "pinn_residual_backward")

    def forward_backward(self, Re, coef_eq, e=None, vis_t0=0.0, alpha_evm=0.0, scale=1.0, want_ebar=False,
                         sums_out=None):
        """forward(save=True) then backward(coef_eq) in one call, for seeds known before the forward (MSE loss):
        on the role-split hidden-256 plan both sweeps of a tile run in one kernel."""
        if not self.with_backward:
            raise RuntimeError("plan was created without backward workspace")
        if want_ebar and self.ebar is None:
            self.ebar = torch.zeros(((self.n + 127) // 128) * 128, dtype=torch.float32, device=self.net.device)
        coef = (ctypes.c_float * 4)(*[float(c) for c in coef_eq])
        _lib.check(self.lib.pinn_residual_forward_backward(
            self.handle, _ptr(self.ws), _ptr(self.net.prep), _ptr(self.x), _ptr(self.y), _ptr(e), _ptr(self.w),
            _ptr(self.vis_t_minus), _ptr(self.vis_t), _ptr(self.fields), coef, float(Re), float(vis_t0),
            float(alpha_evm), float(scale), _ptr(self.sums if sums_out is None else sums_out),
            _ptr(self.ebar if want_ebar else None), _stream()), "pinn_residual_forward_backward")

    def field(self, name):
        return self.fields[FLD[name], :self.n]

    def set_pseudo_time(self, sigma, sigma_p):
        """Hand the anchors (allocated as zeros at the first call) and the rates to a pseudo-time plan."""
        if self.anchor is None:
            self.anchor = torch.zeros(3, self.npad, dtype=torch.float32, device=self.net.device)
        _lib.check(self.lib.pinn_plan_set_pseudo_time(self.handle, _ptr(self.anchor), float(sigma), float(sigma_p)),
                   "pinn_plan_set_pseudo_time")

    def set_viscosity(self, nu, with_lap=True):
        """Viscosity identification: every residual launch of the plan reads the fp32 device scalar `nu` in place of
        1 / Re, and (with_lap) its forward leaves Lap u, Lap v in self.lap [2, npad].  nu None: off."""
        self.nu = nu
        self.lap = None
        if nu is not None and with_lap:
            self.lap = torch.zeros(2, self.npad, dtype=torch.float32, device=self.net.device)
        _lib.check(self.lib.pinn_plan_set_viscosity(self.handle, _ptr(nu), _ptr(self.lap)), "pinn_plan_set_viscosity")
        self.cap = None

    def set_viscosity_cap(self, cap):
        """Reynolds-number continuation: the plan's forward launches read the fp32 device scalar `cap` in place of
        vis_t0.  Only on a plan that carries nu (set_viscosity first, which drops the cap).  None: off."""
        _lib.check(self.lib.pinn_plan_set_viscosity_cap(self.handle, _ptr(cap)), "pinn_plan_set_viscosity_cap")
        self.cap = cap

    def pseudo_time(self):
        """(sigma, sigma_p) the plan carries."""
        a, b = ctypes.c_float(), ctypes.c_float()
        _lib.check(self.lib.pinn_plan_pseudo_time(self.handle, ctypes.byref(a), ctypes.byref(b)), "pinn_plan_pseudo_time")
        return float(a.value), float(b.value)


class ChunkedResidual:
    """Collocation set processed in passes of `chunk_points` points that SHARE one activation workspace
    (forward -> reverse sweep -> gradient assembly per pass, gradients and loss sums accumulated), for
    point sets whose saved activations would not fit in HBM at once - the mini-batching of the
    reference's roadmap (ev-NSFnet/README.md:118; its `batchsize` argument is dead).  Full-batch
    semantics are unchanged: every pass uses the global normalisation.  Presents the attributes of a
    ResidualPlan (field(), vis_t, vis_t_minus, ebar, n)."""

    ALIGN = 128      # chunk boundaries on a multiple of every tile size (16 / 32 / 128 points)

    def __init__(self, net, x, y, weights=None, chunk_points=1 << 20):
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        y = np.asarray(y, dtype=np.float32).reshape(-1)
        w = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1)
        if w is not None and w.size != x.size:
            raise ValueError("weights must have one entry per collocation point")
        self.net, self.n = net, x.size
        chunk = max(self.ALIGN, int(chunk_points) // self.ALIGN * self.ALIGN)
        self.bounds = [(a, min(a + chunk, self.n)) for a in range(0, self.n, chunk)]
        self.chunks, ws = [], None
        for a, b in self.bounds:       # the first pass is the largest: it sizes the shared workspace
            c = ResidualPlan(net, x[a:b], y[a:b], None if w is None else w[a:b], ws=ws)
            ws = c.ws
            self.chunks.append(c)
        self.npad = sum(c.npad for c in self.chunks)
        self.tmp_sums = torch.zeros(NLOSS, dtype=torch.float32, device=net.device)

    def field(self, name):
        return torch.cat([c.field(name) for c in self.chunks])

    @property
    def w(self):
        return None if self.chunks[0].w is None else torch.cat([c.w for c in self.chunks])

    @property
    def vis_t(self):
        return torch.cat([c.vis_t for c in self.chunks])

    @property
    def vis_t_minus(self):
        if self.chunks[0].vis_t_minus is None:
            return None
        return torch.cat([c.vis_t_minus for c in self.chunks])

    @vis_t_minus.setter
    def vis_t_minus(self, t):
        for (a, b), c in zip(self.bounds, self.chunks):
            c.vis_t_minus = None if t is None else t.reshape(-1)[a:b].contiguous()

    @property
    def ebar(self):
        """d loss / d e for all points, padded like a ResidualPlan's (seed of the entropy-net backward)."""
        out = torch.zeros(((self.n + 127) // 128) * 128, dtype=torch.float32, device=self.net.device)
        for (a, b), c in zip(self.bounds, self.chunks):
            out[a:b] = c.ebar[:b - a]
        return out


def _passes(f):
    """The passes of a collocation set as [((lo, hi), plan), ...]: one for a ResidualPlan, one per chunk for a
    ChunkedResidual."""
    if isinstance(f, ChunkedResidual):
        return list(zip(f.bounds, f.chunks))
    return [((0, f.n), f)]


class ValuePlan(PointPlan):
    def __init__(self, net, x, y, targets=None, with_backward=True):
        super().__init__(net, x, y, 1, with_backward)
        dev = net.device
        self.pred = torch.zeros(net.n_out, self.n, dtype=torch.float32, device=dev)
        self.targets = [None, None, None]
        if targets is not None:
            for c, t in enumerate(targets):
                if t is not None:
                    tt = torch.as_tensor(np.asarray(t, dtype=np.float32).reshape(-1)).to(dev).contiguous()
                    if tt.numel() != self.n:
                        raise ValueError("target %d must have one entry per point" % c)
                    self.targets[c] = tt

    def forward(self, coef=(0.0, 0.0, 0.0), save=False, use_targets=True, sums_out=None):
        if save and not self.with_backward:
            raise RuntimeError("plan was created without backward workspace")
        n_out = self.net.n_out
        pred = (ctypes.c_void_p * 3)(*[self.pred[c].data_ptr() if c < n_out else 0 for c in range(3)])
        tgt = (ctypes.c_void_p * 3)(*[(self.targets[c].data_ptr() if (use_targets and self.targets[c] is not None) else 0)
                                      for c in range(3)])
        cf = (ctypes.c_float * 3)(*[float(c) for c in coef])
        _lib.check(self.lib.pinn_value_forward(
            self.handle, _ptr(self.ws), _ptr(self.net.prep), _ptr(self.x), _ptr(self.y), pred, tgt, cf,
            1 if save else 0, _ptr(self.sums if sums_out is None else sums_out), _stream()), "pinn_value_forward")

    def backward(self, out_adj=None):
        _lib.check(self.lib.pinn_value_backward(
            self.handle, _ptr(self.ws), _ptr(self.net.prep), _ptr(self.x), _ptr(self.y), _ptr(out_adj), _stream()),
            "pinn_value_backward")


def resample_scratch(n_pool, device):
    """Device scratch of the two resampling calls for a pool of n_pool points."""
    nbytes = int(_lib.load().pinn_resample_scratch_bytes(int(n_pool)))
    if nbytes < 0:
        raise ValueError("bad pool size %d" % n_pool)
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def resample_select(pool, w4, k, c, u, m, scratch):
    """Systematic-resampling selection of m points of the evaluated forward-only ResidualPlan `pool`
    (pinn_resample_select).  Returns (ascending int64 pool indices [m], S = sum of a as a host float):
    reading S is the one host synchronisation of a resample."""
    out = torch.empty(int(m), dtype=torch.int64, device=pool.fields.device)
    _lib.check(_lib.load().pinn_resample_select(pool.n, _ptr(pool.fields), pool.npad, float(w4), float(k), float(c),
                                                float(u), int(m), _ptr(scratch), _ptr(out), _stream()),
               "pinn_resample_select")
    return out, float(scratch[:8].view(torch.float64).item())


def resample_gather(idx, lo, hi, n_pool, src, dst, scratch, w_sum=None):
    """dst[name][j - lo] = src[name][idx[j]] for j in [lo, hi), name in x, y, w, vtm (w / vtm where both are
    given); w_sum: a one-element fp64 device tensor that receives the fixed-order sum of the gathered w."""
    _lib.check(_lib.load().pinn_resample_gather(
        _ptr(idx), int(lo), int(hi), int(n_pool), _ptr(src["x"]), _ptr(src["y"]), _ptr(src.get("w")), _ptr(src.get("vtm")),
        _ptr(dst["x"]), _ptr(dst["y"]), _ptr(dst.get("w")), _ptr(dst.get("vtm")), _ptr(scratch), _ptr(w_sum), _stream()),
        "pinn_resample_gather")


def grad_reduce(net, plans, grads_out, accumulate=False):
    lib = net.lib
    n = len(plans)
    ph = (ctypes.c_void_p * n)(*[p.handle.value for p in plans])
    wh = (ctypes.c_void_p * n)(*[p.ws.data_ptr() for p in plans])
    _lib.check(lib.pinn_grad_reduce(net.handle, n, ph, wh, _ptr(grads_out), 1 if accumulate else 0, _stream()),
               "pinn_grad_reduce")


def grad_reduce_terms(net, groups, outs, acc_mask=0, partials=None, gram=None):
    """pinn_grad_reduce_terms: groups = three lists of plans (collocation, boundary, supervised), outs = three output
    vectors (None: group not written; a written group without plans gets zeros).  acc_mask bit t: add to outs[t].
    partials: fp64 device tensor of balance_partials_count(P) entries for the max|g| / sum|g| block partials.
    gram: fp64 device tensor of confgrad_partials(P) entries for the Gram block partials
    (pinn_grad_reduce_terms_gram, the same single launch)."""
    lib = net.lib
    plans = [p for grp in groups for p in grp]
    n = len(plans)
    ns = (ctypes.c_int * 3)(*[len(grp) for grp in groups])
    ph = (ctypes.c_void_p * max(n, 1))(*[p.handle.value for p in plans])
    wh = (ctypes.c_void_p * max(n, 1))(*[p.ws.data_ptr() for p in plans])
    out = (ctypes.c_void_p * 3)(*[0 if o is None else o.data_ptr() for o in outs])
    if gram is not None:
        _lib.check(lib.pinn_grad_reduce_terms_gram(net.handle, ns, ph, wh, out, int(acc_mask), _ptr(partials),
                                                   _ptr(gram), _stream()), "pinn_grad_reduce_terms_gram")
        return
    _lib.check(lib.pinn_grad_reduce_terms(net.handle, ns, ph, wh, out, int(acc_mask), _ptr(partials), _stream()),
               "pinn_grad_reduce_terms")


def balance_partials(n, device):
    """Zeroed fp64 device tensor for the block partials of n parameters."""
    count = int(_lib.load().pinn_balance_partials_count(int(n)))
    if count < 0:
        raise ValueError("bad parameter count %d" % n)
    return torch.zeros(count, dtype=torch.float64, device=device)


def balance_stats(vecs, n, partials):
    """Block partials of three vectors (None = zeros): pinn_balance_stats."""
    v = (ctypes.c_void_p * 3)(*[0 if t is None else t.data_ptr() for t in vecs])
    _lib.check(_lib.load().pinn_balance_stats(v, int(n), _ptr(partials), _stream()), "pinn_balance_stats")


def balance_update(partials, n, terms, beta, lam, record):
    """One balance update on the device (pinn_balance_update): record / lam are updated in place."""
    _lib.check(_lib.load().pinn_balance_update(_ptr(partials), int(n), int(terms), float(beta), _ptr(lam), _ptr(record),
                                               _stream()), "pinn_balance_update")


def balance_combine(g, gr, gb, gs, lam):
    """g = g_r + lam[0] g_b + lam[1] g_s (gs None: no supervised term): pinn_balance_combine."""
    _lib.check(_lib.load().pinn_balance_combine(_ptr(g), _ptr(gr), _ptr(gb), _ptr(gs), _ptr(lam), g.numel(), _stream()),
               "pinn_balance_combine")


BALANCE_RECORD = 12      # PINN_BALANCE_RECORD


def confgrad_partials(n, device):
    """Zeroed fp64 device tensor for the Gram block partials of n parameters."""
    count = int(_lib.load().pinn_confgrad_partials_count(int(n)))
    if count < 0:
        raise ValueError("bad parameter count %d" % n)
    return torch.zeros(count, dtype=torch.float64, device=device)


def confgrad_gram(vecs, n, partials):
    """Gram block partials rr, bb, ss, rb, rs, bs of three vectors (None = zeros): pinn_confgrad_gram."""
    v = (ctypes.c_void_p * 3)(*[0 if t is None else t.data_ptr() for t in vecs])
    _lib.check(_lib.load().pinn_confgrad_gram(v, int(n), _ptr(partials), _stream()), "pinn_confgrad_gram")


def confgrad_coef(partials, n, nterms, coef, record):
    """The ConFIG coefficients of nterms (2 or 3) terms on the device (pinn_confgrad_coef): coef [3] fp32 is
    written, record is updated in place."""
    _lib.check(_lib.load().pinn_confgrad_coef(_ptr(partials), int(n), int(nterms), _ptr(coef), _ptr(record), _stream()),
               "pinn_confgrad_coef")


def confgrad_combine(g, gr, gb, gs, coef):
    """g = coef[0] g_r + coef[1] g_b + coef[2] g_s (gs None: no supervised term): pinn_confgrad_combine."""
    _lib.check(_lib.load().pinn_confgrad_combine(_ptr(g), _ptr(gr), _ptr(gb), _ptr(gs), _ptr(coef), g.numel(),
                                                 _stream()), "pinn_confgrad_combine")


CONFGRAD_RECORD = 13     # PINN_CONFGRAD_RECORD


def batch_draw(store, batch, idx, n, b, seed, rank, counter):
    """pinn_batch_draw: draw b of the n store points (stratified; counter = device [t, scratch], advanced by one) into
    idx and gather store['x' | 'y' | 'w' | 'vtm'] at them into batch[...] (w / vtm None: absent).  One launch."""
    _lib.check(_lib.load().pinn_batch_draw(
        int(n), int(b), int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), _ptr(counter), _ptr(store["x"]), _ptr(store["y"]),
        _ptr(store.get("w")), _ptr(store.get("vtm")), _ptr(batch["x"]), _ptr(batch["y"]), _ptr(batch.get("w")),
        _ptr(batch.get("vtm")), _ptr(idx), _stream()), "pinn_batch_draw")


def batch_scatter(idx, b, n, batch_vtm, store_vtm):
    """pinn_batch_scatter: store_vtm[idx[j]] = batch_vtm[j] for j in [0, b).  One launch."""
    _lib.check(_lib.load().pinn_batch_scatter(_ptr(idx), int(b), int(n), _ptr(batch_vtm), _ptr(store_vtm), _stream()),
               "pinn_batch_scatter")


RBA_RECORD = 12          # PINN_RBA_RECORD


def rba_scratch(n, device):
    """Zeroed device scratch of the two attention calls for evaluations of up to n points."""
    nbytes = int(_lib.load().pinn_rba_scratch_bytes(int(n)))
    if nbytes < 0:
        raise ValueError("bad point count %d" % n)
    return torch.zeros(nbytes // 8, dtype=torch.float64, device=device)


def rba_stats(plan, w4, scratch):
    """pinn_rba_stats over the evaluated ResidualPlan `plan`: rmax into scratch[0], the unweighted sums of
    eq1^2..eq4^2 into scratch[1:5].  One launch."""
    _lib.check(_lib.load().pinn_rba_stats(plan.n, _ptr(plan.fields), plan.npad, float(w4), _ptr(scratch), _stream()),
               "pinn_rba_stats")


def rba_apply(plan, w4, gamma, eta, idx, s, lam, w, scratch, record):
    """pinn_rba_apply: lam <- gamma lam + eta r / scratch[0] and w <- s lam^2 at the store points idx (None: the
    plan's points are the store's), from the residual planes of the evaluated `plan`.  One launch."""
    _lib.check(_lib.load().pinn_rba_apply(plan.n, _ptr(plan.fields), plan.npad, float(w4), float(gamma), float(eta),
                                          _ptr(idx), lam.numel(), _ptr(s), _ptr(lam), _ptr(w), _ptr(scratch),
                                          _ptr(record), _stream()), "pinn_rba_apply")


def rba_fill(init, s, lam, w):
    """pinn_rba_fill: lam = init, w = s init^2.  One launch."""
    _lib.check(_lib.load().pinn_rba_fill(lam.numel(), float(init), _ptr(s), _ptr(lam), _ptr(w), _stream()),
               "pinn_rba_fill")


PTIME_RECORD = 8         # PINN_PTIME_RECORD: [sum w eq1^2, eq2^2, eq3^2, sum w (du^2 + dv^2), sum w dp^2, max|du|,|dv|, since, refreshes]


def ptime_scratch(n, device):
    """Zeroed device scratch of ptime_advance for n points (the launch leaves its ticket word 0 again)."""
    nbytes = int(_lib.load().pinn_ptime_scratch_bytes(int(n)))
    if nbytes < 0:
        raise ValueError("bad point count %d" % n)
    return torch.zeros(nbytes // 8, dtype=torch.float64, device=device)


def ptime_advance(plan, every, force, scratch, record):
    """pinn_ptime_advance over the planes the last evaluation of the pseudo-time ResidualPlan `plan` left: the record,
    and the anchor refresh on its cadence (or forced).  One launch."""
    _lib.check(_lib.load().pinn_ptime_advance(plan.n, _ptr(plan.fields), plan.npad, _ptr(plan.w), _ptr(plan.anchor),
                                              int(every), 1 if force else 0, _ptr(scratch), _ptr(record), _stream()),
               "pinn_ptime_advance")


VAL_RECORD = 8           # PINN_VAL_RECORD: [t, e_u, e_v, e_p, e_p0, metric, improved, n_p]
VAL_STATE = 8            # PINN_VAL_STATE: [n_records, best_metric, best_t, stale, nonfinite, improved, cadence records, 0]
VAL_METRICS = dict(uv=0, u=1, v=2, p=3, p0=4)
VAL_ROW = ("t", "e_u", "e_v", "e_p", "e_p0", "metric", "improved", "n_p")


def val_scratch(device):
    """Zeroed device scratch of val_stats."""
    return torch.zeros(int(_lib.load().pinn_val_scratch_bytes()) // 8, dtype=torch.float64, device=device)


def val_planes(n, device):
    """fp32 [3, ceil4(n)]: prediction or target planes whose rows start 16-byte aligned."""
    return torch.zeros(3, (int(n) + 3) // 4 * 4, dtype=torch.float32, device=device)


def val_stats(pred, tgt, n, with_p, metric, t, every, scratch, state, ring):
    """pinn_val_stats: one validation of the prediction planes pred against the target planes tgt (both val_planes;
    with_p False: no pressure) - a row into ring, state updated; t = -1: the cadence position from the state.  One
    launch."""
    rows = 3 if with_p else 2
    pp = (ctypes.c_void_p * 3)(*[pred[c].data_ptr() if c < rows else 0 for c in range(3)])
    tp = (ctypes.c_void_p * 3)(*[tgt[c].data_ptr() if c < rows else 0 for c in range(3)])
    _lib.check(_lib.load().pinn_val_stats(int(n), pp, tp, int(metric), float(t), int(every), _ptr(scratch), _ptr(state),
                                          _ptr(ring), ring.shape[0], _stream()), "pinn_val_stats")


def val_keep(segs, state):
    """pinn_val_keep: dst = src for the one or two (src, dst) fp32 vector pairs when state's improved word is 1.  One
    launch."""
    (s0, d0), (s1, d1) = segs[0], (segs[1] if len(segs) > 1 else (None, None))
    _lib.check(_lib.load().pinn_val_keep(_ptr(s0), _ptr(d0), s0.numel(), _ptr(s1), _ptr(d1),
                                         0 if s1 is None else s1.numel(), _ptr(state), _stream()), "pinn_val_keep")


FLOW_RECORD = 32         # PINN_FLOW_RECORD
FLOW_STATE = 8           # PINN_FLOW_STATE: [n_records, cadence records, records with non-finite nodes, 0 ...]
FLOW_ROW = ("t", "x_c", "y_c", "psi_min", "omega_c") + tuple(
    "%s_%s" % (k, q) for q in ("bl", "br", "tl", "tr") for k in ("x", "y", "psi_max", "area")) + (
    "counter_area", "mass_defect", "ke", "enstrophy", "div_rms", "div_max", "nonfinite")


def flow_scratch(device):
    """Zeroed device scratch of flow_stats."""
    return torch.zeros(int(_lib.load().pinn_flow_scratch_bytes()) // 8, dtype=torch.float64, device=device)


def flow_stream_function(fields, nx, ny, ys, psi):
    """pinn_flow_stream_function: psi [ny nx] fp64 from the u plane of the field planes `fields` [FLD_COUNT, npad] of a
    residual forward on the nx x ny tensor grid (x fastest), by the trapezoid rule along y.  One launch."""
    _lib.check(_lib.load().pinn_flow_stream_function(int(nx), int(ny), _ptr(fields), fields.shape[1], _ptr(ys), _ptr(psi),
                                                     _stream()), "pinn_flow_stream_function")


def flow_stats(fields, nx, ny, xs, ys, psi, eps, t, every, scratch, state, ring):
    """pinn_flow_stats: one diagnostic record of the field planes and their psi - a row into ring, state updated;
    t = -1: the cadence position from the state.  Two launches."""
    _lib.check(_lib.load().pinn_flow_stats(int(nx), int(ny), _ptr(fields), fields.shape[1], _ptr(xs), _ptr(ys), _ptr(psi),
                                           float(eps), float(t), int(every), _ptr(scratch), _ptr(state), _ptr(ring),
                                           ring.shape[0], _stream()), "pinn_flow_stats")


MON_RECORD = 12          # PINN_MON_RECORD
MON_STATE = 16           # PINN_MON_STATE
MON_INFO = 4             # PINN_MON_INFO: this rank's [max vis_t, entries >= vis_t0, fp64 sum, n]
MON_ROW = ("t", "loss", "loss_e", "loss_b", "loss_s", "eq1", "eq2", "eq3", "eq4", "vis_mean", "Re_eff", "stop")
MON_STATE_NAMES = ("updates", "observations", "nonfinite", "window_fill", "window_sum", "window_sum_re", "windows",
                   "window_mean", "window_mean_re", "stale", "settled", "stop", "t_plateau", "t_re_eff", "t_nonfinite")
MON_QUANTITIES = dict(loss=0, loss_e=1, loss_b=2)
MON_STOP = dict(plateau=1, re_eff=2, nonfinite=4)       # PINN_MON_STOP_*
MON_VIS_SLOT = 4         # the slot of the equation block of the loss sums that carries the vis_t sum (4..7 are free)


def monitor_scratch(device):
    """Zeroed device scratch of monitor_vis_stats."""
    return torch.zeros(int(_lib.load().pinn_monitor_scratch_bytes()) // 8, dtype=torch.float64, device=device)


def monitor_vis_stats(vis_t, n, vis_t0, sum_out, info, scratch):
    """pinn_monitor_vis_stats: the fixed-order fp64 sum of vis_t [n], rounded to fp32, into sum_out[0]; this rank's max,
    cap count, fp64 sum and n into info.  One launch."""
    _lib.check(_lib.load().pinn_monitor_vis_stats(int(n), _ptr(vis_t), float(vis_t0), _ptr(sum_out), _ptr(info),
                                                  _ptr(scratch), _stream()), "pinn_monitor_vis_stats")


def monitor_observe(eq, bc, sup, lam, alpha_b, alpha_s, alpha_e, w4, n_eq, n_b, n_s, n_p, Re, cfg, state, ring):
    """pinn_monitor_observe: count one optimiser update and, on the cadence, observe the loss sums eq / bc / sup (None:
    no supervised term; lam None: the constants alpha_b, alpha_s) - a row into ring, state updated.  cfg: a
    MonitorConfigStruct.  One launch."""
    _lib.check(_lib.load().pinn_monitor_observe(_ptr(eq), _ptr(bc), _ptr(sup), _ptr(lam), float(alpha_b), float(alpha_s),
                                                float(alpha_e), float(w4), float(n_eq), float(n_b), float(n_s), float(n_p),
                                                float(Re), ctypes.byref(cfg), _ptr(state), _ptr(ring), _stream()),
               "pinn_monitor_observe")


VISC_STATE = 8           # PINN_VISC_STATE: [theta, m, v, beta1^t, beta2^t, t, last G, skipped]
VISC_STATE_NAMES = ("theta", "m", "v", "beta1_t", "beta2_t", "updates", "grad", "skipped")
VISC_SLOT = 5            # the slot of the equation block of the loss sums that carries S of d loss / d nu = -(2 alpha_e / N) S


def visc_scratch(n, device):
    """Zeroed device scratch of visc_grad for n points (the launch leaves its ticket word 0 again)."""
    nbytes = int(_lib.load().pinn_visc_scratch_bytes(int(n)))
    if nbytes < 0:
        raise ValueError("bad point count %d" % n)
    return torch.zeros(nbytes // 8, dtype=torch.float64, device=device)


def visc_grad(plan, w4, sum_out, scratch):
    """pinn_visc_grad over the planes (fields, lap) the last evaluation of the ResidualPlan `plan` left: the fixed-order
    fp64 sum S of the per-point terms of d loss / d nu, rounded to fp32, into sum_out[0].  One launch."""
    _lib.check(_lib.load().pinn_visc_grad(plan.n, _ptr(plan.fields), plan.npad, _ptr(plan.lap), _ptr(plan.w), float(w4),
                                          _ptr(sum_out), _ptr(scratch), _stream()), "pinn_visc_grad")


def visc_update(sum_in, coef, lr, betas, eps, theta_bounds, state, nu):
    """pinn_visc_update: Adam on theta = ln nu from the (exchanged) sum sum_in[0], G = coef * sum; state and the fp32 nu
    the sweeps read are rewritten in place.  One launch."""
    _lib.check(_lib.load().pinn_visc_update(_ptr(sum_in), float(coef), float(lr), float(betas[0]), float(betas[1]),
                                            float(eps), float(theta_bounds[0]), float(theta_bounds[1]), _ptr(state),
                                            _ptr(nu), _stream()), "pinn_visc_update")


RAMP_RECORD = 6          # PINN_RAMP_RECORD
RAMP_RECORD_NAMES = ("t", "s", "Re_t", "nu_t", "cap_t", "done")
RAMP_SHAPES = dict(geometric=0, linear_re=1, linear_nu=2)       # PINN_RAMP_*


def visc_schedule_value(cstruct, t):
    """pinn_visc_schedule_value: the record [t, s, Re_t, nu_t, cap_t, done] of position t on the host, by the same
    function the step launch runs (nu_t and cap_t are the fp32 values as doubles)."""
    rec = (ctypes.c_double * RAMP_RECORD)()
    nu = _lib.load().pinn_visc_schedule_value(ctypes.byref(cstruct), int(t), rec)
    if nu != nu:
        _lib.check(-22, "pinn_visc_schedule_value")
    return list(rec)


def visc_schedule_step(cstruct, pos, nu, cap, rec):
    """pinn_visc_schedule_step: the position pos [1] int64 moves on by one update; the fp32 nu, the fp32 cap (or None)
    and the record are rewritten in place for it.  One launch."""
    _lib.check(_lib.load().pinn_visc_schedule_step(ctypes.byref(cstruct), _ptr(pos), _ptr(nu), _ptr(cap), _ptr(rec),
                                                   _stream()), "pinn_visc_schedule_step")


OPTIM_RECORD = 6         # PINN_OPTIM_RECORD


def grad_sqnorm_scratch(device):
    """Zeroed device scratch of grad_sqnorm."""
    return torch.zeros(int(_lib.load().pinn_grad_sqnorm_scratch_bytes()) // 8, dtype=torch.float64, device=device)


def grad_sqnorm(g0, g1, scratch):
    """pinn_grad_sqnorm: the fp64 sum of squares of g0 and (not None) g1 into scratch[0], fixed order.  One launch."""
    _lib.check(_lib.load().pinn_grad_sqnorm(_ptr(g0), g0.numel(), _ptr(g1), 0 if g1 is None else g1.numel(),
                                            _ptr(scratch), _stream()), "pinn_grad_sqnorm")


def state_scratch(device):
    """Zeroed device scratch of state_pack / state_unpack."""
    return torch.zeros(int(_lib.load().pinn_state_scratch_bytes()) // 8, dtype=torch.float64, device=device)


def _state_tables(tensors, offsets):
    n = len(tensors)
    for t in tensors:
        if not t.is_contiguous():
            raise ValueError("training state: a segment must be a contiguous tensor")
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() if t.numel() else 0 for t in tensors])
    nbytes = (ctypes.c_int64 * n)(*[t.numel() * t.element_size() for t in tensors])
    return n, ptrs, nbytes, (ctypes.c_int64 * n)(*[int(o) for o in offsets])


def state_pack(srcs, offsets, staging, digests, scratch):
    """pinn_state_pack: the device tensors srcs[k] into the uint8 staging buffer at offsets[k] (-1: digest only, nothing
    stored; staging may then be None), padding zeroed, the digests (A, B) into the int64 device tensor digests [n, 2]
    (the bits of the unsigned words).  One launch per 64 segments."""
    n, ptrs, nbytes, offs = _state_tables(srcs, offsets)
    _lib.check(_lib.load().pinn_state_pack(n, ptrs, nbytes, offs, _ptr(staging), 0 if staging is None else staging.numel(),
                                           _ptr(digests), _ptr(scratch), _stream()), "pinn_state_pack")


def state_unpack(staging, offsets, dsts, digests, scratch):
    """pinn_state_unpack: the reverse scatter, from staging at offsets[k] into the live tensors dsts[k] in place (-1:
    dsts[k] is digested as it stands); digests as in state_pack, of what was written."""
    n, ptrs, nbytes, offs = _state_tables(dsts, offsets)
    _lib.check(_lib.load().pinn_state_unpack(n, _ptr(staging), 0 if staging is None else staging.numel(), nbytes, offs, ptrs,
                                             _ptr(digests), _ptr(scratch), _stream()), "pinn_state_unpack")


class _Snapshot:
    """What save_training_state keeps between calls: the staging buffer (allocated once per segment layout), its pinned
    host copy, the digests, the scratch, the side stream with its events, and the one snapshot in flight."""

    def __init__(self):
        self.sig = None                 # (name, bytes, stored) of every segment the buffers were sized for
        self.offsets, self.total = [], 0
        self.staging = self.host = self.digests = self.digests_host = self.scratch = None
        self.stream = self.ev = None
        self.thread, self.error = None, None
        self.info = None


class LbfgsHistory:
    """Device state of the L-BFGS direction (csrc/lbfgs.hip): the workspace with history_size + 1 (s, y) slots,
    g_prev, R and Y'Y, plus the direction d, the line search's x0 and the two result blocks."""

    def __init__(self, n, history_size, device):
        self.lib = _lib.load()
        self.n, self.history_size, self.device = int(n), int(history_size), torch.device(device)
        nbytes = int(self.lib.pinn_lbfgs_workspace_bytes(self.n, self.history_size))
        if nbytes < 0:
            raise ValueError("L-BFGS: bad size (n=%d, history_size=%d; history_size must be 1..1024)"
                             % (self.n, self.history_size))
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.d = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.x0 = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.result = torch.zeros(8, dtype=torch.float64, device=self.device)
        self.probe_result = torch.zeros(8, dtype=torch.float64, device=self.device)

    def reset(self):
        _lib.check(self.lib.pinn_lbfgs_reset(_ptr(self.ws), self.n, self.history_size, _stream()), "pinn_lbfgs_reset")

    def direction(self, g, t_prev):
        """New d at gradient g (t_prev = 0: first iteration).  Device result block [g'd, max|d|, sum|g|, max|g|,
        accepted, pairs, gamma, y's] (no sync)."""
        _lib.check(self.lib.pinn_lbfgs_direction(_ptr(self.ws), self.n, self.history_size, _ptr(g), float(t_prev),
                                                 _ptr(self.d), _ptr(self.result), _stream()), "pinn_lbfgs_direction")
        return self.result

    def probe(self, g):
        """[g'd, max|d|, sum|g|, max|g|] of a trial gradient against d (device, no sync)."""
        _lib.check(self.lib.pinn_lbfgs_probe(_ptr(self.ws), self.n, self.history_size, _ptr(g), _ptr(self.d),
                                             _ptr(self.probe_result), _stream()), "pinn_lbfgs_probe")
        return self.probe_result


class _EngineSpace:
    """The vector space of lbfgs.step over a PinnEngine: x = the main net's parameters, g = grads (the kept copies
    are the whole exchange buffer, so the loss sums of an accepted point come back with its gradient).  With the
    weight factorization on, x = theta and g = gtheta (kept beside the exchange buffer)."""

    def __init__(self, engine, hist):
        self.e, self.h = engine, hist
        self.rwf = engine.net.theta is not None

    def _g(self):
        return self.e.net.gtheta if self.rwf else self.e.grads

    def evaluate(self):
        e = self.e
        e.loss_and_grad()
        loss = e.loss_terms()["loss"]
        if self.rwf:
            e.net.rwf_grad(e.grads)
        r = self.h.probe(self._g())
        v = torch.cat([loss.reshape(1).to(torch.float64), r[:4]]).cpu().tolist()      # the one readback
        return v[0], v[1], v[4]

    def direction(self, t_prev):
        if t_prev > 0 and float(np.float32(t_prev)) == 0.0:
            t_prev = -1.0            # below fp32 range: a zero step (torch's s = t d rounds to 0, the pair is rejected)
        r = self.h.direction(self._g(), t_prev).cpu().tolist()
        return r[0], r[1], r[2], r[3]

    def save_x(self):
        self.h.x0.copy_(self.e.net.trainable)

    def set_x(self, t):
        torch.add(self.h.x0, self.h.d, alpha=float(t), out=self.e.net.trainable)  # in place: captured steps stay valid
        self.e.net.update_params()

    def keep(self):
        if self.rwf:
            return self.e.flat.clone(), self.e.net.gtheta.clone()
        return self.e.flat.clone()

    def restore(self, h):
        if self.rwf:
            self.e.flat.copy_(h[0])
            self.e.net.gtheta.copy_(h[1])
            return
        self.e.flat.copy_(h)


class _Option:
    """What a training option adds to the parts of PinnEngine that cut across the options; the defaults add nothing.
    PinnEngine._options() lists the options that are on: the refusals, the graph key and the header and segments of a
    training state are loops over it."""
    resident = mse = None       # "<subject> needs": the option refuses a chunked collocation set / the loss mode 'L2'
    stored = ()                 # (segment prefix, attribute, ...): the device tensors a training state stores
    off = ({}, {}, {})          # header() while the option is off ({}: the keys are absent, as in older files)

    def graph_key(self):        # the launch constants a captured step depends on (beyond those in _graph_key's head)
        return ()

    def header(self):           # the entries of a training state's (fingerprint, settings, host mirrors)
        return {}, {}, {}

    def restore_host(self, host):       # the host mirrors back from a training state's
        pass


class _TermCombiner(_Option):
    """What the rules that combine the per-term gradients share: buf = [grads | grads_e | sums | g_b | g_s], the
    engine's exchange buffer (content kept; engine.flat becomes the view of it) with the term vectors gb / gs behind
    it, so several ranks all-reduce the used prefix in one message.  A rule tells _loss_and_grad what the final
    term-split assembly writes besides the vectors (assembly) and makes the gradient of g_r, g_b and g_s (finish)."""
    unit_seeds = False      # the boundary / supervised adjoints carry alpha_b / alpha_s

    def __init__(self, engine):
        n_ex = engine.flat.numel()
        self.buf = torch.zeros(n_ex + 2 * engine.P, dtype=torch.float32, device=engine.device)
        self.buf[:n_ex].copy_(engine.flat)
        engine.flat = self.buf[:n_ex]
        self.gb, self.gs = self.buf[n_ex:n_ex + engine.P], self.buf[n_ex + engine.P:]

    def _allreduce_terms(self, e, sup_on):
        """The global term vectors [grads (= g_r) | grads_e | sums | g_b (| g_s)], in one message."""
        torch.distributed.all_reduce(self.buf[:e.flat.numel() + e.P * (2 if sup_on else 1)], group=e.pg)


class _Balance(_TermCombiner):
    """Host side of the loss balancing: the cadence (Adam updates n counted since set_loss_balancing; `done` = the
    last n whose balance update has run) and the device tensors: lam [2] fp32, rec [BALANCE_RECORD] fp64 (the
    state and the statistics of the last balance step), parts (block partials), buf / gb / gs (term vectors)."""
    unit_seeds = True       # the weights are applied by the combine (device memory, not a launch argument)
    mse, stored = "loss balancing needs", ("bal", "lam", "rec")
    off = (dict(balancing=False), dict(balancing=None), dict(bal=None))

    def __init__(self, engine, every, beta):
        super().__init__(engine)
        self.every, self.beta = every, beta
        self.n, self.done = 0, -1
        self.lam = torch.tensor([engine.alpha_b, engine.alpha_s], dtype=torch.float32).to(engine.device)
        rec = np.zeros(BALANCE_RECORD)
        rec[9], rec[10] = engine.alpha_b, engine.alpha_s
        self.rec = torch.tensor(rec, dtype=torch.float64).to(engine.device)
        self.parts = balance_partials(engine.P, engine.device)

    def header(self):
        return dict(balancing=True), dict(balancing=[self.every, self.beta]), dict(bal=[self.n, self.done])

    def restore_host(self, host):
        self.n, self.done = (int(v) for v in host["bal"])

    def assembly(self, e, update):      # one rank: the local vectors are the global ones, their partials come along
        return dict(partials=self.parts if update and e.world_size == 1 else None)

    def finish(self, e, update, sup_on):
        gs = self.gs if sup_on else None
        if update:
            if e.world_size > 1:
                self._allreduce_terms(e, sup_on)
                balance_stats([e.grads, self.gb, gs], e.P, self.parts)
            balance_update(self.parts, e.P, 1 | (2 if sup_on else 0), self.beta, self.lam, self.rec)
        balance_combine(e.grads, e.grads, self.gb, gs, self.lam)
        if not update and e.world_size > 1:
            # the combine is linear: combining before the one all-reduce gives every rank the same global g
            torch.distributed.all_reduce(e.flat, group=e.pg)


class _ConflictFree(_TermCombiner):
    """Device tensors of the conflict-free gradient combination (set_conflict_free_gradients): buf / gb / gs (the
    exchange buffer with the term vectors alpha_b g_b / alpha_s g_s behind it), parts (Gram block partials), coef [3]
    fp32 and rec [CONFGRAD_RECORD] fp64 (the statistics of the last step and the counters)."""
    mse, stored = "conflict-free gradients need", ("cfg", "coef", "rec")
    off = (dict(confgrad=False), {}, {})

    def __init__(self, engine):
        super().__init__(engine)
        self.coef = torch.ones(3, dtype=torch.float32, device=engine.device)
        self.rec = torch.zeros(CONFGRAD_RECORD, dtype=torch.float64, device=engine.device)
        self.parts = confgrad_partials(engine.P, engine.device)

    def graph_key(self):
        return ("confgrad",)

    def header(self):
        return dict(confgrad=True), {}, {}

    def assembly(self, e, update):      # one rank: the local vectors are the global ones, their Gram partials too
        return dict(gram=self.parts if e.world_size == 1 else None)

    def finish(self, e, update, sup_on):
        gs = self.gs if sup_on else None
        if e.world_size > 1:        # the rule is not linear: every rank computes it from the global vectors
            self._allreduce_terms(e, sup_on)
            confgrad_gram([e.grads, self.gb, gs], e.P, self.parts)
        confgrad_coef(self.parts, e.P, 3 if sup_on else 2, self.coef, self.rec)
        confgrad_combine(e.grads, e.grads, self.gb, gs, self.coef)


class _Batching(_Option):
    """State of the stochastic mini-batching (set_batching): the batch plan f of B points (and, ev flavour, the
    entropy net's plan e on the same x / y buffers), the device index vector idx [B] int64 and the device draw
    counter [t, scratch]."""
    resident = mse = "mini-batching needs"
    stored, off = ("batch", "counter", "idx"), (dict(batch_points=0), dict(batch_seed=None), {})

    def __init__(self, B, seed, rank):
        self.B, self.seed, self.rank = B, seed, rank
        self.f = self.e = self.idx = self.counter = None

    def header(self):
        return dict(batch_points=self.B), dict(batch_seed=self.seed), {}


class _Attention(_Option):
    """State of the residual-based attention (set_residual_attention): the device tensors lam [N] (multipliers),
    s [N] or None (the static weights given to set_collocation), w [N] (the effective weights s lam^2, which is what
    plan_f.w points to while the feature is on), scratch (statistics) and rec [RBA_RECORD] fp64 (the last update);
    n_eval = local points of the last evaluation that updated."""
    resident = mse = "residual attention needs"
    stored, off = ("rba", "lam", "w", "rec"), (dict(attention=False), dict(attention=None), dict(rba_n_eval=None))

    def __init__(self, eta, gamma, init):
        self.eta, self.gamma, self.init = eta, gamma, init
        self.lam = self.s = self.w = self.scratch = self.rec = None
        self.n_eval = 0

    def header(self):
        return dict(attention=True), dict(attention=[self.eta, self.gamma, self.init]), dict(rba_n_eval=self.n_eval)

    def restore_host(self, host):
        self.n_eval = int(host["rba_n_eval"])


class _PseudoTime(_Option):
    """State of the pseudo-time stepping (PinnEngine.set_pseudo_time): the launch constants here, anchors on the
    collocation plan, scratch and record in device memory (_state_segments adds anchors and record itself)."""
    resident = mse = "pseudo-time stepping needs"
    off = (dict(pseudo_time=False), dict(pseudo_time=None), {})

    def __init__(self, dtau, every, pressure_dtau):
        self.dtau, self.pressure_dtau, self.every = dtau, pressure_dtau, every
        self.sigma = 1.0 / dtau
        self.sigma_p = 0.0 if pressure_dtau is None else 1.0 / pressure_dtau
        self.scratch = self.record = None

    def graph_key(self):
        return (("ptime", self.sigma, self.sigma_p, self.every),)

    def header(self):
        return dict(pseudo_time=True), dict(pseudo_time=[self.sigma, self.sigma_p, self.every]), {}


class _Optim(_Option):
    """State of the device learning-rate schedule and gradient clipping (set_lr_schedule / set_grad_clipping): the
    schedule (an LrSchedule; constant while only clipping is on) with its C struct, max_norm (0 = no clipping) and the
    device tensors epoch [1] int64 (the schedule position e), rec [OPTIM_RECORD] fp64 (the last update) and scratch
    (the squared norm and its partials)."""
    stored, off = ("opt", "epoch", "rec"), (dict(schedule_or_clipping=False), dict(schedule=None, max_norm=None), {})

    def __init__(self, device):
        self.user_spec, self.max_norm = None, 0.0
        self.epoch = torch.zeros(1, dtype=torch.int64, device=device)
        self.rec = torch.zeros(OPTIM_RECORD, dtype=torch.float64, device=device)
        self.scratch = grad_sqnorm_scratch(device)
        self.set_spec(None)

    def set_spec(self, spec):
        self.user_spec = spec
        self.spec = spec if spec is not None else _schedule.LrSchedule()
        self.cstruct = self.spec.c_struct()

    def header(self):
        return dict(schedule_or_clipping=True), dict(schedule=repr(self.spec.key()), max_norm=self.max_norm), {}


class _Validation(_Option):
    """State of the device validation monitor (set_validation): the forward-only value plan over the validation
    points, whose pred is a view of the prediction planes; tgt (target planes), scratch, state [VAL_STATE] fp64, ring
    [capacity, VAL_RECORD] fp64 and snap (one snapshot vector per net, of its trainable vector's size).  n counts the
    optimizer updates since set_validation on the host (the device counts the cadence records itself).
    (_state_segments adds the snapshots and the digested points and targets itself.)"""
    stored = ("val", "state", "ring")
    off = (dict(points_val=None, validation=None), dict(validation_every=None), dict(val_n=None))

    def __init__(self, every, metric, keep_best, capacity, with_p):
        self.every, self.metric, self.keep_best, self.capacity, self.with_p = every, metric, keep_best, capacity, with_p
        self.n = 0
        self.plan = self.pred = self.tgt = self.scratch = self.state = self.ring = self.snap = None

    def header(self):
        val = dict(capacity=self.capacity, metric=self.metric, with_p=self.with_p, keep_best=self.keep_best)
        return dict(points_val=self.plan.n, validation=val), dict(validation_every=self.every), dict(val_n=self.n)

    def restore_host(self, host):
        self.n = int(host["val_n"])


class _Monitor(_Option):
    """State of the convergence monitor (set_convergence_monitor): the launch constants (every, window, patience,
    min_updates, quantity, the two tolerances - None: that criterion is off -, mode, capacity) and the device tensors
    state [MON_STATE] fp64, ring [capacity, MON_RECORD] fp64, info [MON_INFO] fp64 (this rank's vis_t statistics) and
    scratch (ev flavour)."""
    resident = mse = "the convergence monitor needs"
    stored = ("monitor", "state", "ring")

    def __init__(self, every, window, min_rel, patience, re_tol, min_updates, quantity, mode, capacity):
        self.every, self.window, self.min_rel, self.patience, self.re_tol = every, window, min_rel, patience, re_tol
        self.min_updates, self.quantity, self.mode, self.capacity = min_updates, quantity, mode, capacity
        self.state = self.ring = self.info = self.scratch = None

    def graph_key(self):
        return (("monitor", self.every, self.window, self.min_rel, self.patience, self.re_tol, self.min_updates,
                 self.quantity, self.capacity),)

    def header(self):
        rec = [self.every, self.window, self.min_rel, self.patience, self.re_tol, self.min_updates, self.quantity, self.mode]
        return dict(monitor=dict(capacity=self.capacity)), dict(monitor=rec), {}

    def c_struct(self, ev):
        return _lib.MonitorConfigStruct(
            every=self.every, window=self.window, patience=self.patience, min_updates=self.min_updates,
            capacity=self.capacity, quantity=MON_QUANTITIES[self.quantity], ev=1 if ev else 0,
            plateau_on=0 if self.min_rel is None else 1, re_eff_on=0 if self.re_tol is None else 1,
            min_rel_improvement=0.0 if self.min_rel is None else self.min_rel,
            re_eff_tol=0.0 if self.re_tol is None else self.re_tol)


class _Viscosity(_Option):
    """Identification of the molecular viscosity (PinnEngine.set_viscosity_identification): the constants, the device
    state of the scalar's Adam [VISC_STATE], the fp32 nu every residual plan reads, the scratch of the gradient launch;
    fresh: the last evaluation was made for Adam (its slot holds a gradient the next adam_step may use); n_eq: its
    normalisation."""
    resident = mse = "viscosity identification needs"
    stored = ("visc", "state", "nu")

    def __init__(self, re0, lr, betas, eps, re_bounds):
        self.re0, self.lr, self.betas, self.eps, self.re_bounds = re0, lr, betas, eps, re_bounds
        self.theta_bounds = (math.log(1.0 / re_bounds[1]), math.log(1.0 / re_bounds[0]))
        self.state = self.nu = self.scratch = None
        self.fresh, self.n_eq = False, 0

    def graph_key(self):
        return (("visc", self.lr, self.betas, self.eps, self.re_bounds),)

    def header(self):
        rec = [self.re0, self.lr, list(self.betas), self.eps, list(self.re_bounds)]
        return dict(viscosity=True), dict(viscosity=rec), {}

    def start(self):
        """The state of an optimiser that has made no update, at re0 (in place).  nu is the fp32 quotient 1 / Re the
        launches would have used as a constant, theta its logarithm: exp(theta) rounds back to it."""
        nu = np.float32(1.0) / np.float32(self.re0)
        self.nu.fill_(float(nu))
        self.state.copy_(torch.tensor([math.log(float(nu)), 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64))


class _Continuation(_Option):
    """Reynolds-number continuation (PinnEngine.set_reynolds_continuation): the ramp's constants with their C struct
    and the device tensors pos [1] int64 (Adam updates made), nu [1] fp32 and, ev flavour with follow_vis_t0, cap [1]
    fp32 - what every residual plan reads in place of 1 / Re and vis_t0 - and rec [RAMP_RECORD] fp64 (the last step)."""
    resident = mse = "Reynolds-number continuation needs"
    stored = ("recont", "pos", "nu", "cap", "rec")

    def __init__(self, engine, re_start, updates, hold, shape, stairs, follow):
        self.re_start, self.updates, self.hold, self.shape, self.stairs = re_start, updates, hold, shape, stairs
        self.follow = follow
        with_cap = follow and engine.net_e is not None
        f32 = np.float32
        factor = engine.vis_t0_factor       # (a vis_t0 assigned since: the factor it amounts to)
        if engine.vis_t0 != factor / engine.Re:
            factor = engine.vis_t0 * engine.Re
        # the ends as the launches form them from their constants: 1.0f / (float)Re, (float)vis_t0
        self.cstruct = _lib.ViscScheduleStruct(
            shape=RAMP_SHAPES[shape], stairs=stairs, hold=hold, updates=updates, re_start=re_start, re_end=engine.Re,
            cap_factor=factor if with_cap else 0.0,
            nu_start=f32(1.0) / f32(re_start), nu_end=f32(1.0) / f32(engine.Re),
            cap_start=f32(factor / re_start) if with_cap else 0.0,
            cap_end=f32(engine.vis_t0) if with_cap else 0.0)
        dev = engine.device
        self.pos = torch.zeros(1, dtype=torch.int64, device=dev)
        self.nu = torch.zeros(1, dtype=torch.float32, device=dev)
        self.cap = torch.zeros(1, dtype=torch.float32, device=dev) if with_cap else None
        self.rec = torch.zeros(RAMP_RECORD, dtype=torch.float64, device=dev)

    def graph_key(self):
        return (("recont", self.re_start, self.updates, self.hold, self.shape, self.stairs, self.follow),)

    def header(self):
        rec = [self.re_start, self.updates, self.hold, self.shape, self.stairs, self.follow]
        return dict(re_continuation=True), dict(re_continuation=rec), {}

    def place(self, t):
        """The state of position t (in place: captured steps stay valid), by the formula the step launch runs,
        evaluated on the host: inside a geometric ramp the host's exp / log may leave nu and the cap one fp32 ulp from
        what stepping to t leaves; the linear shapes and the ends are the same bits."""
        rec = visc_schedule_value(self.cstruct, t)
        self.pos.fill_(int(t))
        self.nu.fill_(rec[3])           # (the fp32 value as a double: exact)
        if self.cap is not None:
            self.cap.fill_(rec[4])
        self.rec.copy_(torch.tensor(rec, dtype=torch.float64))


class _FlowDiag(_Option):
    """State of the flow diagnostics (set_flow_diagnostics): the forward-only residual plan over the nx x ny tensor
    grid, whose field planes the kernels read; xs [nx], ys [ny] fp64 (the plan's fp32 coordinates widened), psi
    [ny nx] fp64, scratch, state [FLOW_STATE] fp64 and ring [capacity, FLOW_RECORD] fp64.  n counts the optimizer
    updates since set_flow_diagnostics on the host (the device counts the cadence records itself)."""
    stored = ("flow", "state", "ring")

    def __init__(self, nx, ny, every, eps, capacity):
        self.nx, self.ny, self.every, self.eps, self.capacity = nx, ny, every, eps, capacity
        self.n = 0
        self.plan = self.xs = self.ys = self.psi = self.scratch = self.state = self.ring = None

    def graph_key(self):
        return (("flow", self.nx, self.ny, self.every, self.eps, self.capacity),)

    def header(self):
        return (dict(flow=dict(nx=self.nx, ny=self.ny, capacity=self.capacity)), dict(flow=[self.every, self.eps]),
                dict(flow_n=self.n))

    def restore_host(self, host):
        self.n = int(host["flow_n"])


# The engine attribute of every option (None while it is off) and its class, in the one order every loop over the
# options runs in: that of the options' segments in a training-state file and of their entries in the graph key.
_OPTIONS = (("_opt", _Optim), ("_bal", _Balance), ("_cfg", _ConflictFree), ("_batch", _Batching), ("_rba", _Attention),
            ("_val", _Validation), ("_pt", _PseudoTime), ("_mon", _Monitor), ("_visc", _Viscosity),
            ("_rc", _Continuation), ("_flow", _FlowDiag))


def _refuse_chunked(option, chunked):
    """The refusal of a chunked collocation set by an option (its class or its state) that needs a resident one."""
    if chunked and option.resident is not None:
        raise ValueError("%s a resident store: the collocation set is chunked (chunk_points)" % option.resident)


# What an evaluation is made for.  Each mode holds what the one before it holds, and more:
EVAL_ADAM = 0           # an Adam step: a fresh batch, attention and balance updates, the conflict-free combination
EVAL_FULL_BATCH = 1     # loss_and_grad(full_batch=True): the whole store, the attention weights held
EVAL_LBFGS = 2          # the L-BFGS objective: also the loss weights held, and its own gradient (the plain sum)
_SAME_MODE = contextlib.nullcontext()       # (an evaluation that asks for nothing: no generator on the step's path)
_RESTORED = object()    # the L-BFGS owner after load_training_state: whoever calls lbfgs_step next adopts the state


class PinnEngine:
    """The per-step hot path for one rank.

    flavour 'nsfnet': loss = alpha_b*loss_b + alpha_e*(m(eq1)+m(eq2)+m(eq3)), nu = 1/Re
                      (NSFnet/pinn_solver.py:197-226)
    flavour 'ev':     adds the entropy net e, lagged artificial viscosity, eq4 with weight
                      0.1, SDF weights, optional supervised loss
                      (ev-NSFnet/pinn_solver.py:290-342, 372-428)
    Multi-GPU: every rank holds a shard of the points; ONE all-reduce (RCCL) of
    [grad | grad_e | sums] per step, all normalisations use GLOBAL counts.
    """

    def __init__(self, device, n_hidden, hidden, Re, alpha_b=1.0, alpha_e=1.0, flavour="nsfnet",
                 n_hidden_e=None, hidden_e=None, alpha_evm=0.0, alpha_s=0.0, coord_scale=1.0,
                 vis_t0_factor=20.0, process_group=None, world_size=1, net=None, net_e=None, precision=None):
        self.device = torch.device(device)
        self.flavour = flavour
        self.Re = float(Re)
        self.alpha_b, self.alpha_e, self.alpha_s = float(alpha_b), float(alpha_e), float(alpha_s)
        self.alpha_evm = float(alpha_evm)
        self.scale = float(coord_scale)
        self.vis_t0 = vis_t0_factor / self.Re
        self.vis_t0_factor = float(vis_t0_factor)
        self.net = net if net is not None else DeviceNet(3, n_hidden, hidden, self.device, precision)
        if flavour == "ev":
            self.net_e = net_e if net_e is not None else DeviceNet(1, n_hidden_e, hidden_e, self.device, precision)
        else:
            self.net_e = None
        self.e_trainable = False
        self.pg, self.world_size = process_group, int(world_size)
        self.P, self.P1 = self.net.num_params, (self.net_e.num_params if self.net_e else 0)
        self.flat = torch.zeros(self.P + self.P1 + NSUMS, dtype=torch.float32, device=self.device)
        self.plan_f = self.plan_b = self.plan_s = self.plan_e = None
        self._graphs = {}
        self._side = None
        self._resample_calls = 0        # resample() calls so far: part of each call's seed, kept across pools
        self._overlap = os.environ.get("NSFNET_OVERLAP_BC", "1") not in ("0", "", "false")
        self.n_f_global = self.n_b_global = self.n_s_global = 0
        self._n_p_local, self._n_p_valid, self._sup_stale = 0, None, False
        self.eq4_weight = 0.1
        self._lbfgs = None                  # LbfgsHistory (created by the first lbfgs_step)
        self._lbfgs_state = _lbfgs.LbfgsState()
        self._lbfgs_owner = None            # what the state belongs to (lbfgs_step's `owner`)
        self._mode = EVAL_ADAM              # what the evaluations are made for (_evaluating)
        self._bal = None                    # adaptive loss-weight balancing (set_loss_balancing; None = off)
        self._cfg = None                    # conflict-free combination (set_conflict_free_gradients; None = off)
        self._batch = None                  # stochastic mini-batching (set_batching; None = off)
        self._eval_batch = False            # the last evaluation ran on the batch plan (loss_terms' normalisation)
        self._rba = None                    # residual-based attention (set_residual_attention; None = off)
        self._pool = self._pool_w = self._pool_e = self._pool_scratch = None     # set_resample_pool
        self._opt = None                    # device lr schedule / gradient clipping (set_lr_schedule, set_grad_clipping)
        self._rwf = None                    # random weight factorization (set_weight_factorization; None = off)
        self._val = None                    # device validation monitor (set_validation; None = off)
        self._pt = None                     # pseudo-time stepping (set_pseudo_time; None = off)
        self._ff = None                     # frozen Fourier-feature first layer (set_fourier_features; None = off)
        self._mon = None                    # convergence monitor (set_convergence_monitor; None = off)
        self._snap = None                   # training-state snapshots (save_training_state; buffers made at first use)
        self._visc = None                   # viscosity identification (set_viscosity_identification; None = off)
        self._rc = None                     # Reynolds-number continuation (set_reynolds_continuation; None = off)
        self._flow = None                   # flow diagnostics (set_flow_diagnostics; None = off)

    # ---- what the evaluations are made for ----
    @contextlib.contextmanager
    def _evaluating(self, mode):
        """Evaluate in `mode` (or the current one, where that holds more); the previous mode comes back on exit."""
        prev, self._mode = self._mode, max(self._mode, mode)
        try:
            yield
        finally:
            self._mode = prev

    # what the mode holds, option by option (read-only)
    _bal_frozen = _cfg_frozen = property(lambda self: self._mode == EVAL_LBFGS)
    _batch_frozen = _rba_frozen = property(lambda self: self._mode != EVAL_ADAM)

    def _rank(self):
        return torch.distributed.get_rank(self.pg) if self.world_size > 1 else 0

    def _w4(self):      # the weight of eq4 (the plain flavour has none)
        return self.eq4_weight if self.net_e is not None else 0.0

    def _options(self):
        """The training options that are on, in the order of _OPTIONS (for configuration, graph-key and checkpoint time:
        the step's path tests the attributes it needs directly)."""
        return [o for o in (getattr(self, attr) for attr, _ in _OPTIONS) if o is not None]

    def _option_header(self, part):
        """What the options add to part 0 / 1 / 2 (fingerprint / settings / host mirrors) of a training state's header:
        an option's header() where it is on, its class's `off` where it is not."""
        out = {}
        for attr, cls in _OPTIONS:
            o = getattr(self, attr)
            out.update((cls.off if o is None else o.header())[part])
        return out

    # ---- views into the exchange buffer ----
    @property
    def grads(self):
        return self.flat[:self.P]

    @property
    def grads_e(self):
        return self.flat[self.P:self.P + self.P1]

    @property
    def sums(self):
        return self.flat[self.P + self.P1:]

    # ---- data ----
    def set_collocation(self, x, y, weights=None, n_global=None, chunk_points=None):
        """chunk_points (or $NSFNET_CHUNK_POINTS): process the set in passes of that many points sharing
        one activation workspace (ChunkedResidual); default: one pass, everything resident."""
        if chunk_points is None and os.environ.get("NSFNET_CHUNK_POINTS"):
            chunk_points = int(os.environ["NSFNET_CHUNK_POINTS"])
        n = int(np.asarray(x).size)
        bt = self._batch
        chunked = bool(chunk_points) and n > int(chunk_points)
        for option in self._options():
            _refuse_chunked(option, chunked)
        if bt is not None and bt.B > n:
            raise ValueError("mini-batching: batch_points=%d exceeds the %d local collocation points" % (bt.B, n))
        self._graphs.clear()      # captured steps hold the old plan's pointers
        self.lbfgs_reset()
        if chunked:
            self.plan_f = ChunkedResidual(self.net, x, y, weights, chunk_points)
        else:
            self.plan_f = ResidualPlan(self.net, x, y, weights, **({} if self._pt is None else dict(pseudo_time=True)))
        self.n_f_global = int(n_global if n_global is not None else self.plan_f.n)
        if self._visc is not None:
            self._attach_viscosity(self.plan_f)
        if self._rc is not None:
            self._attach_continuation(self.plan_f)
        if self.net_e is not None:
            self.plan_e = ValuePlan(self.net_e, x, y)
            self.init_vis_t()
        self._eval_batch = False
        if self._rba is not None:
            self._attach_attention()        # the new set starts at lam = init; its weights are the new s
        if bt is not None:
            self._make_batch_plans(bt)      # the store may have gained or lost its weights; the draw counter carries on
        if self._pt is not None:
            self._attach_pseudo_time()      # the new set starts anchored at the field of the current weights

    # ---- residual-based attention weights on the collocation points ----
    def set_residual_attention(self, eta=0.0, gamma=0.999, init=1.0):
        """eta > 0: residual-based attention (RBA; Anagnostopoulos, Toscano, Stergiopulos & Karniadakis 2024).  Every
        local collocation point i carries a multiplier lam_i, and the weight the residual kernels read becomes
        w_i = s_i lam_i^2 with s the static weights given to set_collocation (1 without).  After every evaluation
        made for Adam (step(), and loss_and_grad() followed by adam_step()), from its unweighted residual planes:
            r_j = sqrt(eq1^2 + eq2^2 + eq3^2 + eq4_weight eq4^2),  rmax = max r_j over the points of ALL ranks,
            lam_i <- gamma lam_i + eta r_j / rmax,  w_i <- s_i lam_i^2          (fp64, rounded to fp32 on store)
        so lam stays within [0, max(init, eta / (1 - gamma))].  An rmax that is 0 or not finite skips the update
        (attention_info()['skipped']).  The weights evaluation k uses are those made after evaluation k - 1 - one
        evaluation of lag, like vis_t_minus - because the fused forward + reverse sweep needs w before the residual
        exists; w is a constant to the reverse sweep, as RBA prescribes.  With mini-batching the statistics are the
        batch's and only the drawn points change.  Evaluations of lbfgs_step and with full_batch=True do not update:
        the L-BFGS objective uses the current weights throughout.  resample() renormalises s and restarts lam at
        init.  loss_terms() keeps returning the WEIGHTED terms Adam minimises; attention_info() has the unweighted
        ones.  lam is not part of a save() checkpoint: a run restored from one restarts it at init (a training state,
        save_training_state, carries it).

        eta = 0: off (plan_f.w is s again and every path launches what it launches without the feature).  A call
        restarts lam at init; so does set_collocation.  Refused: a chunked store, gamma outside (0, 1], eta < 0,
        init < 0 (ValueError), a call before set_collocation (RuntimeError) and, in loss_and_grad, loss mode 'L2'."""
        eta, gamma, init = float(eta), float(gamma), float(init)
        if not (math.isfinite(eta) and eta >= 0.0):
            raise ValueError("residual attention: eta must be finite and >= 0")
        if not (0.0 < gamma <= 1.0):
            raise ValueError("residual attention: gamma must be in (0, 1]")
        if not (math.isfinite(init) and init >= 0.0):
            raise ValueError("residual attention: init must be finite and >= 0")
        if eta > 0.0:
            if self.plan_f is None:
                raise RuntimeError("set_residual_attention() needs set_collocation() first")
            _refuse_chunked(_Attention, isinstance(self.plan_f, ChunkedResidual))
        self._graphs.clear()        # captured steps hold the other weight buffer and gamma / eta
        old = self._rba
        if old is not None:
            self.plan_f.w = old.s   # the static weights again (None: the set had none)
            self._rba = None
        if eta > 0.0:
            self._rba = _Attention(eta, gamma, init)
            self._attach_attention()
        if self._batch is not None and (old is not None or eta > 0.0):
            self._make_batch_plans(self._batch)      # the store may have gained or lost its weight buffer

    def _attach_attention(self):
        """Take plan_f's weights as s, allocate lam and the effective-weight buffer, make it plan_f.w and fill."""
        a, f = self._rba, self.plan_f
        a.s = f.w
        a.lam = torch.zeros(f.n, dtype=torch.float32, device=self.device)
        a.w = torch.zeros(f.n, dtype=torch.float32, device=self.device)
        a.scratch = rba_scratch(f.n, self.device)
        a.rec = torch.zeros(RBA_RECORD, dtype=torch.float64, device=self.device)
        a.n_eval = 0
        f.w = a.w
        rba_fill(a.init, a.s, a.lam, a.w)

    def _static_w(self):
        """The static weights of the resident collocation set (what set_collocation was given), or None."""
        return self._rba.s if self._rba is not None else self.plan_f.w

    def attention(self):
        """Device fp32 tensor [N]: the attention multipliers lam of the local collocation points (updated in place);
        None when the feature is off."""
        return None if self._rba is None else self._rba.lam

    def attention_info(self):
        """The device record of the last attention update (one host read), or None when the feature is off: rmax,
        lam_min / lam_mean / lam_max of the multipliers that update wrote, the UNWEIGHTED loss_eq1..4 and loss_e of
        the evaluation it followed (this rank's points), updates, skipped, and the settings."""
        a = self._rba
        if a is None:
            return None
        r = a.rec.cpu().tolist()
        out = dict(rmax=r[0], lam_min=r[5], lam_max=r[6], lam_mean=r[7] / r[8] if r[8] > 0 else float("nan"),
                   updates=int(r[9]), skipped=int(r[10]), eta=a.eta, gamma=a.gamma, init=a.init)
        n = max(a.n_eval, 1)
        for k in range(4):
            out["loss_eq%d" % (k + 1)] = r[1 + k] / n
        out["loss_e"] = (r[1] + r[2] + r[3] + (self.eq4_weight * r[4] if self.net_e is not None else 0.0)) / n
        return out

    def _attention_update(self, f, bt):
        """One attention update from the residual planes the collocation pass just wrote on plan f (the batch plan
        when bt is given: its points are the store's bt.idx).  Two launches; between them, multi-rank, the MAX
        all-reduce of the one rmax word - as int64: the kernel stores a NaN as the positive quiet NaN, so the
        integer order of non-negative doubles is their NaN-propagating order."""
        a, w4 = self._rba, self._w4()
        rba_stats(f, w4, a.scratch)
        if self.world_size > 1:
            torch.distributed.all_reduce(a.scratch[:1].view(torch.int64), op=torch.distributed.ReduceOp.MAX,
                                         group=self.pg)
        rba_apply(f, w4, a.gamma, a.eta, None if bt is None else bt.idx, a.s, a.lam, a.w, a.scratch, a.rec)
        a.n_eval = f.n

    # ---- stochastic mini-batching of the collocation term ----
    def set_batching(self, batch_points=0, seed=0):
        """batch_points = B > 0: every evaluation made for Adam (step(), and loss_and_grad() followed by adam_step())
        runs the collocation term on a fresh random batch of B of the N local collocation points, which stay
        resident as the store.  Each evaluation (1) draws B ascending, distinct store indices on the device,
        stratified with one point per stratum [floor(j N / B), floor((j + 1) N / B)) (Philox4x32-10, counter
        (slot j, draw number t), key (seed, rank); t lives in device memory and advances by one per draw, so a
        captured step draws a new batch on every replay), (2) gathers x, y, w and vis_t_minus of those points into the
        batch plan's buffers, (3) runs the usual step on the batch plan with the collocation normalisation
        B * world_size instead of n_f_global, and (4), ev flavour, scatters the batch's updated vis_t_minus back to
        the store, so a point's lagged viscosity is alpha_evm |e| at its last visit.

        The weights are used as gathered, without renormalising them per batch.  When B divides N every point is
        drawn with probability B / N and the batch loss is an unbiased estimate of the full weighted mean; when it
        does not, the strata differ by one point, and so do the inclusion probabilities (1 / floor(N / B) against
        1 / ceil(N / B)): the estimate is biased by that much.  B = N draws the identity: the step is the full one,
        bit for bit.  The boundary and supervised terms always use their full sets.  Multi-rank: B is per rank and
        must be the same on all ranks; every rank draws from its own shard.

        lbfgs_step, resample, init_vis_t and collocation_points keep using the store.  batch_points = 0: off.  A call
        restarts the draw counter at 0 (set_collocation and resample do not).  Refused with ValueError: B > N, a
        chunked store, and (in loss_and_grad) the loss mode 'L2'."""
        B, seed = int(batch_points), int(seed)
        if B < 0:
            raise ValueError("mini-batching: batch_points must be >= 0")
        if B > 0 and self._pt is not None:
            raise ValueError("mini-batching is not available with pseudo-time stepping: the anchors live with the "
                             "evaluated plan (store-level anchors and a gather are a follow-up)")
        if B > 0:
            if self.plan_f is None:
                raise RuntimeError("set_batching() needs set_collocation() first")
            _refuse_chunked(_Batching, isinstance(self.plan_f, ChunkedResidual))
            if B > self.plan_f.n:
                raise ValueError("mini-batching: batch_points=%d exceeds the %d local collocation points"
                                 % (B, self.plan_f.n))
        self._graphs.clear()        # captured steps hold the other plan's pointers
        self._eval_batch = False
        if B == 0:
            self._batch = None
            return
        bt = _Batching(B, seed, self._rank())
        bt.idx = torch.zeros(B, dtype=torch.int64, device=self.device)
        bt.counter = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._make_batch_plans(bt)
        self._batch = bt

    def _make_batch_plans(self, bt):
        """The batch plan(s) of bt.B points for the current store; the buffers are filled by every draw."""
        z = lambda: np.zeros(bt.B, dtype=np.float32)       # one array per buffer: a host tensor may alias its source
        bt.f = ResidualPlan(self.net, z(), z(), None if self.plan_f.w is None else z())
        if self._visc is not None:
            self._attach_viscosity(bt.f)
        if self._rc is not None:
            self._attach_continuation(bt.f)
        bt.e = None
        if self.net_e is not None:
            bt.f.vis_t_minus = torch.zeros(bt.B, dtype=torch.float32, device=self.device)
            bt.e = ValuePlan(self.net_e, z(), z())
            bt.e.x, bt.e.y = bt.f.x, bt.f.y         # one gather serves both nets

    def batch_indices(self):
        """Device int64 tensor [B]: the store indices of the last drawn batch (ascending, distinct); None when
        batching is off.  It is rewritten in place by the next draw."""
        return None if self._batch is None else self._batch.idx

    def batch_info(self):
        """dict(batch_points, store_points, seed, draws) (one host read of the device draw counter), or None when
        batching is off."""
        bt = self._batch
        if bt is None:
            return None
        return dict(batch_points=bt.B, store_points=self.plan_f.n, seed=bt.seed, draws=int(bt.counter[0].item()))

    def _batching_on(self):
        return self._batch is not None and self._mode == EVAL_ADAM

    def _colloc(self):
        """(collocation plan, entropy-net plan, global point count of the normalisation) of the next evaluation: the
        batch plans when batching is on, else the store."""
        if self._batching_on():
            bt = self._batch
            return bt.f, bt.e, bt.B * self.world_size
        return self.plan_f, self.plan_e, self.n_f_global

    @property
    def evaluated_batch(self):
        """True when the last evaluation ran on a drawn batch (its loss terms are the batch's)."""
        return self._eval_batch and self._batch is not None

    def eval_plans(self):
        """(collocation plan, entropy-net plan) the last evaluation ran on: their fields, vis_t and pred are what the
        solvers publish."""
        if self.evaluated_batch:
            return self._batch.f, self._batch.e
        return self.plan_f, self.plan_e

    def set_boundary(self, x, y, u, v, n_global=None):
        self._graphs.clear()      # captured steps hold the old plan's pointers
        self.lbfgs_reset()
        self.plan_b = ValuePlan(self.net, x, y, targets=[u, v, None])
        self.n_b_global = int(n_global if n_global is not None else self.plan_b.n)

    def set_supervised(self, x, y, u, v, p=None, n_global=None):
        """Supervised samples of THIS rank (ev-NSFnet/pinn_solver.py:202-251).  A rank's share may be
        empty (np.array_split with fewer samples than ranks, :219-221; the reference then skips the
        branch on that rank, :400): it contributes zero sums and no gradient but still takes part in
        the step's all-reduce and divides by the global counts."""
        self._graphs.clear()      # captured steps hold the old plan's pointers
        self.lbfgs_reset()
        self._n_p_valid = None
        self.sums[S_SUP:S_SUP + NLOSS].zero_()
        self._sup_stale = False
        if x is None:
            self.plan_s, self.n_s_global, self._n_p_local = None, 0, 0
            return
        n_local = int(np.asarray(x).size)
        self.n_s_global = int(n_global if n_global is not None else n_local)
        if n_local == 0:
            self.plan_s, self._n_p_local = None, 0
            return
        self.plan_s = ValuePlan(self.net, x, y, targets=[u, v, p])
        self._n_p_local = 0 if p is None else int(np.isfinite(np.asarray(p, dtype=np.float64)).sum())

    def init_vis_t(self):
        """vis_t_minus = alpha_evm*|e(x_f)|   (ev-NSFnet/pinn_solver.py:138-140)"""
        self.plan_e.forward(save=False)
        fresh = (self.alpha_evm * self.plan_e.pred[0].abs()).contiguous()
        passes = _passes(self.plan_f)
        if all(p.vis_t_minus is not None and p.vis_t_minus.shape == (hi - lo,) for (lo, hi), p in passes):
            for (lo, hi), p in passes:      # in place: a captured hipGraph keeps reading / writing these allocations
                p.vis_t_minus.copy_(fresh[lo:hi])
        else:
            self._graphs.clear()
            self.plan_f.vis_t_minus = fresh

    # ---- residual-based resampling of the collocation points ----
    def set_resample_pool(self, x, y, weights=None):
        """Candidate points of THIS rank for resample(): a forward-only residual plan over them (and, for the ev
        flavour, a forward-only plan of the entropy net).  `weights` (pool SDF weights) must be given exactly when
        the live collocation set has weights.  A new pool does not restart the draws: the call counter that goes into
        resample()'s seed keeps counting, so refreshing the pool every stage with one seed gives fresh U values."""
        if self.plan_f is not None and (weights is None) != (self._static_w() is None):
            raise ValueError("pool weights must be given exactly when the collocation set has weights")
        pool = ResidualPlan(self.net, x, y, with_backward=False)
        if self._visc is not None:
            self._attach_viscosity(pool, with_lap=False)
        if self._rc is not None:
            self._attach_continuation(pool)
        w = None
        if weights is not None:
            w = torch.as_tensor(np.asarray(weights, dtype=np.float32).reshape(-1)).to(self.device).contiguous()
            if w.numel() != pool.n:
                raise ValueError("pool weights must have one entry per pool point")
        self._pool, self._pool_w = pool, w
        self._pool_e = ValuePlan(self.net_e, x, y, with_backward=False) if self.net_e is not None else None
        self._pool_scratch = resample_scratch(pool.n, self.device)

    def resample(self, k=1.0, c=1.0, seed=0):
        """Replace the live collocation points by plan_f.n points of the pool, drawn with density
        |r|^k / mean|r|^k + c (systematic resampling, pinn_resample_select) under the current parameters, Re, scale,
        vis_t0 and alpha_evm.  The live buffers are rewritten IN PLACE, so a captured step replays on the new points;
        parameters, Adam moments, the boundary / supervised plans and n_f_global are not touched.  Each rank draws from
        its own pool shard (per-rank stratification).  The weights are renormalised to mean 1 over the global selected
        set (with residual attention on: the static weights s, and lam restarts at init); the entropy-net state
        vis_t_minus of a new point is alpha_evm |e|, what init_vis_t gives it.  Stream-ordered after the last step; one
        8-byte host read.  Returns the int64 pool indices (ascending, may repeat)."""
        f, pool = self.plan_f, self._pool
        if self._pt is not None:
            raise ValueError("resample() is not available with pseudo-time stepping: new points invalidate the anchors")
        if pool is None or f is None:
            raise RuntimeError("resample() needs set_collocation() and set_resample_pool() first")
        rba = self._rba              # on: the gather and the renormalisation work on the static weights s
        if (self._pool_w is None) != (self._static_w() is None):
            raise ValueError("pool weights must be given exactly when the collocation set has weights")
        e = vtm0 = None
        if self.net_e is not None:
            self._pool_e.forward(save=False)
            e = self._pool_e.pred[0]
            vtm0 = (self.alpha_evm * e.abs()).contiguous()       # init_vis_t at the pool points
            pool.vis_t_minus = vtm0.clone()                        # (the forward overwrites its state argument)
        pool.forward(self.Re, e=e, vis_t0=self.vis_t0, alpha_evm=self.alpha_evm, scale=self.scale, save=False)
        u = np.random.default_rng([int(seed), self._resample_calls, self._rank()]).random()     # (calls counted per engine)
        self._resample_calls += 1
        idx, S = resample_select(pool, self._w4(), k, c, u, f.n, self._pool_scratch)
        self.lbfgs_reset()                       # the objective changes: the history no longer describes it
        if self._batch is not None:
            self._graphs.clear()
        if not math.isfinite(S):
            raise FloatingPointError("resample: the pool's residual sum is %r (non-finite residual or coordinate in the "
                                     "pool); the collocation set is unchanged" % S)
        passes = _passes(f)
        src = dict(x=pool.x, y=pool.y, w=self._pool_w, vtm=vtm0)
        wts = [rba.s] if rba is not None else [ck.w for _, ck in passes]      # (attention: one resident pass)
        w_sums = torch.zeros(len(passes), dtype=torch.float64, device=self.device) if wts[0] is not None else None
        for j, ((lo, hi), ck) in enumerate(passes):
            dst = dict(x=ck.x, y=ck.y, w=wts[j], vtm=ck.vis_t_minus)
            resample_gather(idx, lo, hi, pool.n, src, dst, self._pool_scratch,
                            None if w_sums is None else w_sums[j:j + 1])
            if self.plan_e is not None:
                self.plan_e.x[lo:hi].copy_(ck.x)
                self.plan_e.y[lo:hi].copy_(ck.y)
        if w_sums is not None:
            total = 0.0
            for v in w_sums.cpu().tolist():          # pass order
                total += v
            if self.world_size > 1:
                t = torch.tensor([total], dtype=torch.float64, device=self.device)
                torch.distributed.all_reduce(t, group=self.pg)
                total = float(t.item())
            mean = total / self.n_f_global
            for wt in wts:                           # mean 1 over the global set (cavity_data._compute_sdf_weights)
                wt.copy_((wt.double() / mean).float())
        if rba is not None:                          # new points: lam = init, w = s init^2 (in place: graphs stay valid)
            rba_fill(rba.init, rba.s, rba.lam, rba.w)
        return idx

    def collocation_points(self):
        """(x, y, w) of the live collocation set as fresh device tensors (w None without weights; with residual
        attention on, w is the effective weight s lam^2)."""
        plans = [p for _, p in _passes(self.plan_f)]
        return tuple(None if getattr(plans[0], k) is None else torch.cat([getattr(p, k) for p in plans])
                     for k in ("x", "y", "w"))

    # ---- adaptive loss-weight balancing ----
    def set_loss_balancing(self, every=0, beta=0.1):
        """every > 0: balance the boundary (and supervised) weight by the learning-rate-annealing rule (Wang, Teng &
        Perdikaris 2021): on Adam update n of the main net with n % every == 0 (updates counted from this call on,
        by step() and adam_step()), lambda_t <- (1 - beta) lambda_t + beta max|g_r| / mean|g_t| from the global
        per-term gradients, in the first evaluation for that update.  The weights live on the device and start at
        alpha_b / alpha_s; the gradient Adam sees is g_r + lambda_b g_b + lambda_s g_s.  every = 0: off (the step
        launches what it launches without balancing).  A call restarts the weights and the update count."""
        every, beta = int(every), float(beta)
        if every < 0:
            raise ValueError("loss balancing: every must be >= 0")
        if every > 0 and not (0.0 < beta <= 1.0):
            raise ValueError("loss balancing: beta must be in (0, 1]")
        if every > 0 and self._cfg is not None:
            raise ValueError("loss balancing and conflict-free gradients both decide how the term gradients are "
                             "combined: switch set_conflict_free_gradients off first")
        self._graphs.clear()        # captured steps hold the seeds and buffers of the other mode
        if every == 0:
            self._bal = None
            return
        self._bal = _Balance(self, every, beta)

    def loss_weights(self):
        """Device tensor [lambda_b, lambda_s] (fp32) of the weights the gradient uses (the configured ones when
        balancing is off)."""
        if self._bal is not None:
            return self._bal.lam
        return torch.tensor([self.alpha_b, self.alpha_s], dtype=torch.float32).to(self.device)

    def balance_info(self):
        """The device record of the last balance step (one host read), or None when balancing is off."""
        b = self._bal
        if b is None:
            return None
        r = b.rec.cpu().tolist()
        names = ("max_r", "mean_r", "max_b", "mean_b", "lambda_hat_b", "max_s", "mean_s", "lambda_hat_s", "skipped",
                 "lambda_b", "lambda_s", "updates")
        out = dict(zip(names, r))
        out["skipped"], out["updates"] = int(out["skipped"]), int(out["updates"])
        out.update(every=b.every, beta=b.beta, adam_updates=b.n)
        return out

    def _balance_due(self):
        """True for the first evaluation of a balance update (n % every == 0), which it claims."""
        b = self._bal
        if b is None or self._mode == EVAL_LBFGS or b.n % b.every != 0 or b.done == b.n:
            return False
        b.done = b.n
        return True

    def _sup_on(self):
        return self.n_s_global > 0 and self.alpha_s != 0.0

    # ---- conflict-free combination of the per-term gradients ----
    def set_conflict_free_gradients(self, enabled=True):
        """enabled: every evaluation on the Adam path combines the global per-term gradients g_r (collocation), g_b
        (boundary) and - with the supervised loss active - g_s by the ConFIG rule (Liu, Chu & Thuerey 2025): the
        direction with equal positive projection on every term's unit gradient, as long as the sum of the terms'
        projections on it; for two terms g = (|g_r| + |g_b|) / 2 (g_r / |g_r| + g_b / |g_b|).  The terms keep the
        configured alpha_e, alpha_b and alpha_s; the rule has no state, so no weight can drift, and loss_terms() stays
        the alpha-weighted sum.  Per step and rank this is the term-split assembly (which also writes the Gram
        statistics), a one-workgroup coefficient kernel and a combine; several ranks all-reduce the term vectors
        [grads | grads_e | sums | g_b (| g_s)] in one message every step, since the rule is not linear.  Parallel,
        anti-parallel or non-finite terms fall back to the plain sum (conflict_info() counts them).  lbfgs_step
        evaluates with the plain sum: the combined direction is not the gradient of an objective.  Not together with
        set_loss_balancing or the L2 loss mode.  Off (the default): the step launches what it launches without the
        feature.  A call restarts the counters."""
        if enabled and self._bal is not None:
            raise ValueError("conflict-free gradients and loss balancing both decide how the term gradients are "
                             "combined: switch set_loss_balancing off first")
        if enabled and self._visc is not None:
            raise ValueError("conflict-free gradients are not available with viscosity identification "
                             "(set_viscosity_identification): the combined direction is not the gradient of the loss "
                             "whose d / d nu the scalar follows")
        self._graphs.clear()        # captured steps hold the launches and buffers of the other mode
        if not enabled:
            self._cfg = None
            return
        self._cfg = _ConflictFree(self)

    def conflict_info(self):
        """The device record of the last conflict-free combination (one host read), or None when the feature is
        off: the term norms n_*, their cosines, the coefficients k_* of g = sum k_t g_t, |g|, and the counters
        steps, fallbacks (plain-sum steps) and dropped (zero-norm terms left out)."""
        c = self._cfg
        if c is None:
            return None
        names = ("n_r", "n_b", "n_s", "cos_rb", "cos_rs", "cos_bs", "k_r", "k_b", "k_s", "norm", "steps", "fallbacks",
                 "dropped")
        out = dict(zip(names, c.rec.cpu().tolist()))
        for k in ("steps", "fallbacks", "dropped"):
            out[k] = int(out[k])
        return out

    # ---- one loss + gradient evaluation ----
    def loss_and_grad(self, mode="MSE", full_batch=False):
        """mode 'MSE' (every script of the reference) or 'L2': 2-norms of the residual / boundary-misfit vectors
        (NSFnet/pinn_solver.py:202-204, 214-217; plain NSFnet, one GPU).  The same kernels run: only the adjoint
        coefficients change, from 2 alpha / N to alpha / ||r_k||, and the norms have to be known first - one host read
        of the forward sums per evaluation (no hipGraph in this mode).  Refusals come before any stream switch.
        full_batch: evaluate the whole store although mini-batching is on (what lbfgs_step's evaluations do)."""
        if mode not in ("MSE", "L2"):
            raise ValueError("loss mode must be 'MSE' or 'L2' (got %r)" % (mode,))
        l2 = mode == "L2"
        for option in self._options() if l2 else ():
            if option.mse is not None:
                raise ValueError("%s the MSE loss (loss mode %r)" % (option.mse, mode))
        if l2 and (self.net_e is not None or self.world_size > 1 or self._sup_on() or len(_passes(self.plan_f)) > 1):
            raise NotImplementedError("loss mode 'L2' exists for the plain NSFnet flavour on one GPU (NSFnet/pinn_solver.py:202-217)")
        with self._evaluating(EVAL_FULL_BATCH) if full_batch else _SAME_MODE:
            self._loss_and_grad(self._balance_due(), l2)

    def _loss_and_grad(self, update=False, l2=False):
        b = self.plan_b
        f, plan_e, n_f = self._colloc()
        bt = self._batch if self._batching_on() else None
        self._eval_batch = bt is not None
        comb = self._bal        # the rule that combines the term gradients; None: the plain sum
        if comb is None and self._mode != EVAL_LBFGS:       # (never both; the L-BFGS objective has its own gradient)
            comb = self._cfg
        sums = self.sums
        sup_on = self._sup_on()
        s = self.plan_s if sup_on else None             # None also on a rank whose supervised share is empty
        n_p = self._n_p_valid_global() if sup_on else 0
        if s is None and self._sup_stale:
            # the supervised block is all-reduced in place with everything else: what an earlier step left
            # there (this rank's own sums, or - on a rank with an empty share - the global sums) would be
            # added again, and multiplied by world_size, every step
            sums[S_SUP:S_SUP + NLOSS].zero_()
            self._sup_stale = False
        if sup_on:
            self._sup_stale = True
        # The value-mode chains (boundary / supervised points: a few thousand points, latency-bound
        # kernels) are independent of the collocation chain until the gradient assembly: they run on a
        # second HIP stream beside it.
        main = side = None
        if self.device.type == "cuda" and self._overlap:
            main = torch.cuda.current_stream(self.device)
            side = self._side_stream(main)
            side.wait_stream(main)
            torch.cuda.set_stream(side)
        try:
            wb, ws = (1.0, 1.0) if comb is not None and comb.unit_seeds else (self.alpha_b, self.alpha_s)
            cb = 2.0 * wb / self.n_b_global
            if l2:      # norms first (2052 boundary points: a forward-only pass), then the adjoints alpha_b (u - u_b) / ||u - u_b||
                b.forward(coef=(0.0, 0.0, 0.0), save=False, sums_out=sums[S_BC:S_BC + NLOSS])
                nb = torch.sqrt(sums[S_BC:S_BC + 2]).cpu().numpy().astype(np.float64)
                b.forward(coef=(self.alpha_b / max(nb[0], 1e-30), self.alpha_b / max(nb[1], 1e-30), 0.0), save=True,
                          sums_out=sums[S_BC:S_BC + NLOSS])
            else:
                b.forward(coef=(cb, cb, 0.0), save=True, sums_out=sums[S_BC:S_BC + NLOSS])
            b.backward()
            if s is not None:
                # per-output means: u,v over all supervised points, p over its finite targets (ev:399-411)
                cs = 2.0 * ws / self.n_s_global
                s.forward(coef=(cs, cs, (2.0 * ws / n_p) if n_p > 0 else 0.0), save=True,
                          sums_out=sums[S_SUP:S_SUP + NLOSS])
                s.backward()
        finally:
            if side is not None:
                torch.cuda.set_stream(main)
        if bt is not None:      # draw + gather: the batch buffers are rewritten in place, the device counter advances
            st = self.plan_f
            batch_draw(dict(x=st.x, y=st.y, w=st.w, vtm=st.vis_t_minus),
                       dict(x=f.x, y=f.y, w=f.w, vtm=f.vis_t_minus), bt.idx, st.n, bt.B, bt.seed, bt.rank, bt.counter)
        e = None
        if self.net_e is not None:
            plan_e.forward(save=self.e_trainable)
            e = plan_e.pred[0]
        c = 2.0 * self.alpha_e / n_f
        coef_eq = (c, c, c, c * self._w4())
        # one pass per plan (several: chunks sharing one workspace, gradients and sums accumulate); every pass but
        # the last is reduced here, the last one together with the value plans below
        passes = _passes(f)
        many = len(passes) > 1
        eq_sums = sums[S_EQ:S_EQ + NLOSS]
        if many:
            eq_sums.zero_()
        for k, ((lo, hi), p) in enumerate(passes):
            ek = e[lo:hi] if e is not None and many else e
            out = f.tmp_sums if many else eq_sums
            if not l2 and hasattr(p, "forward_backward"):      # MSE seeds: one call, the sweeps fused where the plan allows
                p.forward_backward(self.Re, coef_eq, e=ek, vis_t0=self.vis_t0, alpha_evm=self.alpha_evm,
                                   scale=self.scale, want_ebar=self.e_trainable, sums_out=out)
            else:
                p.forward(self.Re, e=ek, vis_t0=self.vis_t0, alpha_evm=self.alpha_evm, scale=self.scale, save=True,
                          sums_out=out)
                if l2:      # d ||eq_k|| / d theta = sum eq_k d eq_k / ||eq_k||: the reverse sweep's seeds with alpha_e / ||eq_k||
                    ne = torch.sqrt(out[:3]).cpu().numpy().astype(np.float64)
                    coef_eq = tuple(self.alpha_e / max(v, 1e-30) for v in ne) + (0.0,)
                p.backward(self.Re, coef_eq, e=ek, scale=self.scale, want_ebar=self.e_trainable)
            if many:
                eq_sums += f.tmp_sums
            if k < len(passes) - 1:
                if comb is None:
                    grad_reduce(self.net, [p], self.grads, accumulate=k > 0)
                else:
                    grad_reduce_terms(self.net, [[p], [], []], [self.grads, None, None], acc_mask=1 if k > 0 else 0)
        if bt is not None and f.vis_t_minus is not None:      # the forward left alpha_evm |e| of the batch points there
            batch_scatter(bt.idx, bt.B, self.plan_f.n, f.vis_t_minus, self.plan_f.vis_t_minus)
        vs = self._visc
        if vs is not None:
            # after the loss-sum launch of the pass, before the attention update below rewrites the weights the sweep
            # read, and before the exchange, which makes the sum global in the message that is sent anyway.  An evaluation that
            # is not made for Adam (L-BFGS, full_batch) leaves the slot at the 0 the loss-sum launch wrote, and holds nu
            vs.fresh, vs.n_eq = self._mode == EVAL_ADAM, n_f
            if vs.fresh:
                visc_grad(f, self._w4(), eq_sums[VISC_SLOT:], vs.scratch)
        if self._rba is not None and self._mode == EVAL_ADAM:      # the weights of the NEXT evaluation
            self._attention_update(f, bt)
        mon = self._mon
        if mon is not None and self.net_e is not None and self._mode != EVAL_LBFGS:
            # after the loss-sum launch of the pass (which zeroes the slot) and before the exchange below, which makes
            # the sum global in the message that is sent anyway: every rank then observes the same bits
            monitor_vis_stats(f.vis_t, f.n, self.vis_t0, eq_sums[MON_VIS_SLOT:], mon.info, mon.scratch)
        if side is not None:
            main.wait_stream(side)
        last = passes[-1][1]
        if comb is None:
            grad_reduce(self.net, [last, b] + ([] if s is None else [s]), self.grads, accumulate=many)
        else:       # g_r into grads, g_b / g_s behind the exchange buffer
            grad_reduce_terms(self.net, [[last], [b], [] if s is None else [s]],
                              [self.grads, comb.gb, comb.gs if sup_on else None], acc_mask=1 if many else 0,
                              **comb.assembly(self, update))
        if self.net_e is not None:
            if self.e_trainable:
                plan_e.backward(out_adj=f.ebar)
                grad_reduce(self.net_e, [plan_e], self.grads_e)
            else:
                self.grads_e.zero_()
        if comb is not None:
            comb.finish(self, update, sup_on)
        elif self.world_size > 1:
            torch.distributed.all_reduce(self.flat, group=self.pg)

    def _side_stream(self, main):
        """The stream the value-mode chains run on.  Inside a graph capture it must be a stream that is
        not already capturing something else; one persistent stream per engine serves both cases."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def _n_p_valid_global(self):
        if self._n_p_valid is None:
            n = int(self._n_p_local)
            if self.world_size > 1:
                tt = torch.tensor([n], dtype=torch.int64, device=self.device)
                torch.distributed.all_reduce(tt, group=self.pg)
                n = int(tt.item())
            self._n_p_valid = n
        return self._n_p_valid

    def loss_terms(self, mode="MSE"):
        """Device tensors (no sync): dict of loss_eq1..4, loss_e, loss_b, loss_s, loss of the sums of the last
        evaluation, in the loss mode it ran with.  The equation terms carry the per-point weights the evaluation
        used - with residual attention on, the effective weights s lam^2: they are what Adam minimises
        (attention_info() has the unweighted ones).  With pseudo-time stepping on, loss_e (and loss_eq1..3) is the
        minimised term, of the residuals q_k; loss_e_steady is the same sum over the steady residuals and drift is
        (sum w ((u-u*)^2 + (v-v*)^2) + sum w (p-p*)^2) / N, both from the record the advance after the last update left,
        in the normalisation of loss_e.  The record is per rank - nothing new is all-reduced - so with several ranks
        these two are THIS rank's share of the global mean; before the first update they are those of the attached
        weights: the steady term, and a drift of 0."""
        s = self.sums
        if mode == "L2":      # NSFnet/pinn_solver.py:202-204, 214-217
            eq = torch.sqrt(s[S_EQ:S_EQ + 4])
            loss_e = eq[0] + eq[1] + eq[2]
            loss_b = torch.sqrt(s[S_BC]) + torch.sqrt(s[S_BC + 1])
            return dict(loss_eq1=eq[0], loss_eq2=eq[1], loss_eq3=eq[2], loss_eq4=eq[3], loss_e=loss_e, loss_b=loss_b,
                        loss_s=torch.zeros((), device=self.device), loss=self.alpha_b * loss_b + self.alpha_e * loss_e)
        eq = s[S_EQ:S_EQ + 4] / (self._batch.B * self.world_size if self._eval_batch else self.n_f_global)
        loss_e = eq[0] + eq[1] + eq[2] + (self.eq4_weight * eq[3] if self.net_e is not None else 0.0)
        loss_b = (s[S_BC] + s[S_BC + 1]) / self.n_b_global
        out = dict(loss_eq1=eq[0], loss_eq2=eq[1], loss_eq3=eq[2], loss_eq4=eq[3], loss_e=loss_e, loss_b=loss_b)
        loss_s = torch.zeros((), device=self.device)
        if self._sup_on():
            n_p = self._n_p_valid_global()
            loss_s = (s[S_SUP] + s[S_SUP + 1]) / self.n_s_global + (s[S_SUP + 2] / n_p if n_p > 0 else 0.0)
        out["loss_s"] = loss_s
        if self._pt is not None:        # this rank's record of the last update (nothing new is all-reduced)
            r = self._pt.record
            out["loss_e_steady"] = (r[0] + r[1] + r[2]) / self.n_f_global + (
                self.eq4_weight * eq[3].double() if self.net_e is not None else 0.0)
            out["drift"] = (r[3] + r[4]) / self.n_f_global
        if self._bal is not None:
            lam = self._bal.lam
            out["loss"] = lam[0] * loss_b + self.alpha_e * loss_e + lam[1] * loss_s
            out["lambda_b"], out["lambda_s"] = lam[0], lam[1]
            return out
        out["loss"] = self.alpha_b * loss_b + self.alpha_e * loss_e + self.alpha_s * loss_s
        return out

    def adam_step(self, lr, validate=None, diagnose=None):
        """Adam on the gradient of the last evaluation.  With a device schedule or clipping on, lr is the schedule's
        base rate lr0; every trainable net uses the lr_e and the clipping coefficient of the same epoch.  With
        set_validation on, the update that is due by its cadence is followed by a validation (validate: step()'s
        decision for a captured sequence; None = by the count); set_flow_diagnostics and `diagnose` likewise."""
        o = self._opt
        with_e = self.net_e is not None and self.e_trainable
        g, ge = self.grads, self.grads_e
        if self._rwf is not None:       # the chain rule from the effective gradient (all-reduced, combined) to d theta
            g = self.net.rwf_grad(g)
            if with_e:
                ge = self.net_e.rwf_grad(ge)
        if o is None:
            self.net.adam_step(g, lr)
            if with_e:
                self.net_e.adam_step(ge, lr)
        else:
            if o.max_norm > 0.0:        # the gradient Adam consumes: all-reduced, combined (, transformed)
                grad_sqnorm(g, ge if with_e else None, o.scratch)
            if with_e:
                self.net_e.adam_step_sched(ge, lr, o, advance=False)
            self.net.adam_step_sched(g, lr, o, advance=True)        # last: it moves the epoch on
        vs = self._visc
        if vs is not None and vs.fresh:     # the scalar's own Adam, from the exchanged slot of the evaluation just used
            visc_update(self.sums[S_EQ + VISC_SLOT:], -2.0 * self.alpha_e / vs.n_eq, vs.lr, vs.betas, vs.eps,
                        vs.theta_bounds, vs.state, vs.nu)
        rc = self._rc
        if rc is not None:      # the ramp moves on by one update: nu (and the cap) of the NEXT evaluation
            visc_schedule_step(rc.cstruct, rc.pos, rc.nu, rc.cap, rc.rec)
        if self._bal is not None:
            self._bal.n += 1
        self._updated(validate, diagnose=diagnose)

    def _count_updates(self, d):
        """Move the host mirrors of the update count (what adam_step advances) by d = +1 / -1."""
        self.net.adam_t += d
        if self.net_e is not None and self.e_trainable:
            self.net_e.adam_t += d
        if self._bal is not None:
            self._bal.n += d
        if self._val is not None:
            self._val.n += d
        if self._flow is not None:
            self._flow.n += d

    # ---- random weight factorization of the dense layers ----
    def _nets(self):
        return [("net", self.net)] + ([("net_e", self.net_e)] if self.net_e is not None else [])

    def set_weight_factorization(self, mean=0.5, std=0.1, seed=0, factors=None):
        """Random weight factorization (RWF; Wang, Wang, Sankaran & Perdikaris 2022): every Linear layer of every net
        - the first and the output layer included, on the ev flavour both nets - gets its weight as
        W = diag(exp(s)) V with s (one fp32 scale factor per row) and V both trainable.  The optimizers then act on
        theta = [params with V where W stands | s] with d loss / d theta: Adam's moments, the clipping norm and the
        L-BFGS vectors all have theta's size.  Per Adam update and trainable net this costs two small launches, both
        captured in the step graph: the chain rule from the effective gradient (after the all-reduce and the
        loss-balancing combine, whose statistics stay those of the effective term gradients) and the compose that
        rebuilds `params`, which prepare, state_dict, predict and every plan keep reading.

        s ~ Normal(mean, std), drawn on the host from np.random.Generator(np.random.Philox(key=seed)): the main net
        first, layers ascending and rows ascending, then the entropy net from the same generator.  The global numpy
        and torch generators are not consumed, and every rank draws the same s.  factors: the s to use instead of a
        draw, as weight_factors() returns them (per net a list of per-layer tensors, or one flat vector).  V = W / g
        by one fp32 division; `params` is not rewritten before the first update, so the first evaluation is
        bit-identical to the one without the feature.

        mean = None: off; `params` stays as composed.  Every call re-creates Adam (t = 0, zero moments), forgets the
        L-BFGS history and clears the captured graphs; the schedule position is left alone.  load_state_dict with
        the feature on sets `params` exactly and re-splits with the current s."""
        self._graphs.clear()        # captured steps hold the other vectors' pointers
        self._lbfgs = None          # the history is sized on the trainable vector
        self.lbfgs_reset()
        if mean is None and factors is None:
            self._rwf = None
            for _, net in self._nets():
                net.set_factorization(None)
            self._validation_reset()
            return
        given = {}
        if factors is not None:
            for name, net in self._nets():
                if name not in factors:
                    raise ValueError("weight factorization: factors has no entry %r" % name)
                f = factors[name]
                if isinstance(f, (list, tuple)):
                    f = torch.cat([torch.as_tensor(a, dtype=torch.float32).reshape(-1).cpu() for a in f])
                given[name] = torch.as_tensor(f, dtype=torch.float32).reshape(-1)
            mean = std = seed = None
        else:
            mean, std, seed = float(mean), float(std), int(seed)
            if not (math.isfinite(mean) and math.isfinite(std) and std >= 0.0):
                raise ValueError("weight factorization: mean must be finite, std finite and >= 0")
            rng = np.random.Generator(np.random.Philox(key=seed))
            for name, net in self._nets():
                given[name] = torch.from_numpy(rng.normal(mean, std, size=net.rwf_rows).astype(np.float32))
        for name, net in self._nets():
            net.set_factorization(given[name])
        self._rwf = dict(mean=mean, std=std, seed=seed)
        self._validation_reset()

    def weight_factors(self):
        """dict(net=[s_0, ..., s_L][, net_e=[...]]): the per-layer scale factors s as fp32 device tensors, views of
        theta that the updates rewrite in place; None when the feature is off."""
        if self._rwf is None:
            return None
        return {name: net.factors() for name, net in self._nets()}

    def factorization_info(self):
        """One host read: dict(n_train=[per net], layers={net name: [dict(min, max, mean) of g = fp32(exp(s)) per
        layer]}, mean, std, seed); None when the feature is off."""
        if self._rwf is None:
            return None
        nets = self._nets()
        s = torch.cat([net.theta[net.num_params:] for _, net in nets]).cpu().numpy()
        out = dict(self._rwf, n_train=[net.num_train for _, net in nets], layers={})
        off = 0
        for name, net in nets:
            rows = []
            for r, _ in layer_shapes(net.n_out, net.n_hidden, net.hidden):
                g = np.exp(s[off:off + r].astype(np.float64)).astype(np.float32)
                rows.append(dict(min=float(g.min()), max=float(g.max()), mean=float(g.astype(np.float64).mean())))
                off += r
            out["layers"][name] = rows
        return out

    # ---- frozen Fourier-feature first layer ----
    def set_fourier_features(self, sigma=1.0, seed=0, frequencies=None):
        """Random Fourier features (Tancik et al. 2020; Wang, Wang & Perdikaris 2021) as the main net's first layer:
        gamma(x) = [cos(2 pi B x), sin(2 pi B x)] with B of shape (hidden / 2, 2), followed by the tanh layers 1 .. L-1.
        That is this net with layer 0 on sin instead of tanh and frozen: rows 2k and 2k + 1 of W0 are both
        fp32(2 pi B_k), their biases fp32(pi / 2) (the cosine) and 0 (the sine).  The call writes them into the flat
        parameters - state_dict keeps its keys and shapes, every other layer the values it had - and sets the net's
        first-layer kind, so every plan of the main net (collocation passes, batch, pool, boundary, supervised,
        validation, predict) evaluates the same function.  The entropy net of the ev flavour keeps tanh.

        B ~ Normal(0, sigma^2), drawn in fp64 from a torch.Generator of its own seeded with `seed`: the global
        generators are not consumed and every rank draws the same B.  frequencies: the B to use instead of a draw.
        sigma's default 1.0 is a guess; no value has been compared in training.

        Layer 0 is not trained: its 3 * hidden entries lead every gradient vector as +0.0 (grads, the term vectors of
        balancing and ConFIG, the L-BFGS gradient), so Adam, clipping and L-BFGS leave it where it is.  By default the
        plans run the 8-wave kernel families and store layer 0.  With PINN_FF_SPLIT=1 in the environment when a residual
        plan is created it keeps the role-split, fused and wide role-split sweeps the other switches choose, in their
        frozen-sine variants, whose reverse sweep ends at layer 1; where either sweep would not be a role-split one the
        whole plan is the default one (fourier_info()["kernels"] names what the collocation plan launches).  Needs an
        even hidden width and at least 2 hidden layers; not available together
        with hard walls or pseudo-time.  Must be called before any point set is attached (ValueError otherwise).
        sigma = None without frequencies: off (layer 0 is tanh again and trainable; its weights stay as they are)."""
        if any(p is not None for p in (self.plan_f, self.plan_b, self.plan_s, self._pool, self._val, self._flow)):
            raise ValueError("fourier features: call set_fourier_features before any point set is attached")
        net = self.net
        if sigma is None and frequencies is None:
            net.set_first_layer(0)
            self._ff = None
            return
        if net.hard_bc is not None or self._pt is not None:
            raise ValueError("fourier features: not available together with hard walls or pseudo-time")
        H = net.hidden
        if H % 2:
            raise ValueError("fourier features: the hidden width must be even (got %d)" % H)
        if net.n_hidden < 2:
            raise ValueError("fourier features: at least 2 hidden layers are needed (got %d)" % net.n_hidden)
        if frequencies is not None:
            B = torch.as_tensor(np.asarray(frequencies, dtype=np.float64))
            if tuple(B.shape) != (H // 2, 2):
                raise ValueError("fourier features: frequencies must have shape (%d, 2), got %s" % (H // 2, tuple(B.shape)))
            sigma = seed = None
        else:
            sigma, seed = float(sigma), int(seed)
            if not (math.isfinite(sigma) and sigma > 0.0):
                raise ValueError("fourier features: sigma must be finite and > 0 (got %r)" % (sigma,))
            gen = torch.Generator(device="cpu")
            gen.manual_seed(seed)
            B = sigma * torch.randn(H // 2, 2, generator=gen, dtype=torch.float64)
        if not bool(torch.isfinite(B).all()):
            raise ValueError("fourier features: frequencies must be finite")
        w0, b0 = fourier_first_layer(B)
        flat = net.params.detach().cpu().clone()
        flat[:2 * H] = w0.reshape(-1)
        flat[2 * H:3 * H] = b0
        net.set_first_layer(1)
        net.set_flat(flat)
        self._ff = dict(sigma=sigma, seed=seed, frequencies=B.clone())

    def fourier_info(self):
        """dict(kind="sine", sigma, seed, frequencies=B as an fp64 (hidden / 2, 2) tensor, kernels, split) of
        set_fourier_features (sigma and seed None where B was given); None when the option is off.  kernels: the three
        names the collocation plan launches (None before one is attached); split: $PINN_FF_SPLIT as plan creation reads
        it now (an integer, 0 when unset)."""
        if self._ff is None:
            return None
        try:
            split = int(os.environ.get("PINN_FF_SPLIT", "0"))
        except ValueError:
            split = 0
        names = getattr(self.plan_f, "kernel_names", None)      # (a stand-in plan of the CPU tests has no kernels)
        return dict(kind="sine", sigma=self._ff["sigma"], seed=self._ff["seed"], frequencies=self._ff["frequencies"].clone(),
                    kernels=None if names is None else names(), split=split)

    # ---- hard wall conditions by an output transform ----
    def set_hard_boundary(self, enabled=True, lift_power=2, lid_sharpness=10.0, origin=(0.0, 0.0), inv_len=1.0):
        """enabled: the no-slip walls and the lid of the lid-driven unit cavity hold exactly, by construction:
        u = g + D N_u, v = D N_v, p = N_p with N the main net's outputs, D = 16 X(1-X) Y(1-Y) zero on the four walls and
        g = l(X) Y^lift_power the lift of the regularised lid l = 1 - cosh(lid_sharpness (X - 1/2)) / cosh(lid_sharpness / 2)
        (cavity_data.py's profile at its default 10).  X = (x - origin[0]) inv_len, Y = (y - origin[1]) inv_len place the
        unit cavity in the net's input coordinates: origin (0, 0) and inv_len 1 without a coordinate map, origin (-1, -1)
        and inv_len 1/2 with ev-NSFnet's; coord_scale * inv_len must be 1.  lift_power (an integer, 1..8) decides how
        fast the lid's influence decays into the cavity; the default 2 is a guess, not a measured optimum.

        Every ResidualPlan / ValuePlan of the main net created from here on is constrained (the entropy net's never are):
        collocation passes and chunks, the batch plan, the resample pool, boundary, supervised, validation and predict.
        Field planes, losses, predictions and gradients are those of the constrained field.  The boundary term keeps
        running: its misfit is rounding-size and its gradient exactly zero (D = 0 at wall points), which makes loss_b a
        live check of the constraint.  A constrained plan runs the 8-wave kernel families; the role-split and fused
        sweeps have no constrained variant yet.

        Must be called before any point set is attached (ValueError otherwise).  enabled=False: off."""
        if any(p is not None for p in (self.plan_f, self.plan_b, self.plan_s, self._pool, self._val, self._flow)):
            raise ValueError("hard boundary: call set_hard_boundary before any point set is attached")
        if not enabled:
            self.net.hard_bc = None
            return
        if self.net.first_layer:
            raise ValueError("hard boundary: not available together with fourier features")
        m = int(lift_power)
        if m != lift_power or not 1 <= m <= 8:
            raise ValueError("hard boundary: lift_power must be an integer in 1..8 (got %r)" % (lift_power,))
        x0, y0 = (float(c) for c in origin)
        r, il = float(lid_sharpness), float(inv_len)
        if not all(math.isfinite(c) for c in (x0, y0, r, il)):
            raise ValueError("hard boundary: origin, inv_len and lid_sharpness must be finite")
        if not il > 0.0:
            raise ValueError("hard boundary: inv_len must be > 0 (got %r)" % (inv_len,))
        if abs(r) > 150.0:
            raise ValueError("hard boundary: |lid_sharpness| must be <= 150 (got %r)" % (lid_sharpness,))
        if abs(self.scale * il - 1.0) > 1e-6:
            raise ValueError("hard boundary: coord_scale * inv_len must be 1 (coord_scale %g, inv_len %g)" % (self.scale, il))
        self.net.hard_bc = _lib.HardBcStruct(1, m, x0, y0, il, r)

    def hard_boundary_info(self):
        """dict(lift_power, lid_sharpness, origin=(x0, y0), inv_len) of set_hard_boundary; None when it is off."""
        bc = self.net.hard_bc
        if bc is None:
            return None
        return dict(lift_power=int(bc.lift_power), lid_sharpness=float(bc.lid_sharpness),
                    origin=(float(bc.x0), float(bc.y0)), inv_len=float(bc.inv_len))

    # ---- pseudo-time stepping of the residual loss ----
    def set_pseudo_time(self, dtau=None, every=0, pressure_dtau=None):
        """dtau > 0 and every >= 1: pseudo-time stepping of the collocation term.  Every local collocation point carries
        an anchor (u*, v*, p*) in device memory, the field there when the anchors were last refreshed, and the
        residuals the term minimises become, with sigma = 1 / dtau and sigma_p = 1 / pressure_dtau (0 when None:
        no artificial compressibility),
            q1 = eq1 + sigma (u - u*),  q2 = eq2 + sigma (v - v*),  q3 = eq3 + sigma_p (p - p*),
            loss_e = alpha_e / N sum_i w_i (q1^2 + q2^2 + q3^2 + eq4_weight eq4^2)
        with eq4 (ev flavour) on the steady eq1, eq2 as before.  For fixed anchors that is one backward-Euler step of
        the pseudo-transient equations; at u = u* it is the steady loss, so the steady solution is a fixed point.  The
        field planes keep the steady residuals and the fields: resampling pools, residual attention, validation,
        logging and the eq*_pred views read what they read without the feature.  With hard walls u, v are the
        constrained fields.

        After every optimiser update (an Adam step, or one lbfgs_step call; line-search evaluations never count) one
        launch records, from the planes of the evaluation that update used, the steady sums, the drift
        sum w ((u - u*)^2 + (v - v*)^2), sum w (p - p*)^2 and max(|u - u*|, |v - v*|), and on every `every`-th update
        overwrites the anchors with those planes' U, V, P - the field one update old, the lag vis_t_minus has.  The
        cadence is device state: the launch is part of the captured step.  The first anchor is the field of the
        weights when set_collocation attaches the points; reset_pseudo_time() re-anchors at the current weights.
        Anchors are not part of a save() checkpoint (a training state, save_training_state, carries them).

        By default the collocation plan runs the 8-wave kernel families (as PINN_SCHED=0 PINN_WSPLIT=0 PINN_FUSE=0
        would).  With PINN_PTIME_SPLIT=1 in the environment when set_collocation creates the plan it keeps the
        role-split, wide role-split and fused sweeps the other switches choose, in their pseudo-time variants; the
        pipelined schedule has none, and a sweep that would run it runs the 8-wave kernel (pseudo_time_info()["kernels"]
        names what the plan launches).  dtau, every and pressure_dtau have no measured defaults: any value is a guess
        until the convergence runs exist.

        Must be called before set_collocation (ValueError otherwise).  dtau None or every 0: off.  Refused with
        ValueError: mini-batching, resample(), a chunked collocation set and the loss mode 'L2'."""
        if self.plan_f is not None:
            raise ValueError("pseudo-time stepping: call set_pseudo_time before set_collocation")
        if dtau is None or not every:
            if pressure_dtau is not None and dtau is None:
                raise ValueError("pseudo-time stepping: pressure_dtau needs dtau")
            self._pt = None
            return
        ev = int(every)
        if ev != every or ev < 1:
            raise ValueError("pseudo-time stepping: every must be an integer >= 0 (got %r)" % (every,))
        for name, v in (("dtau", dtau), ("pressure_dtau", pressure_dtau)):
            if v is not None and not (math.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError("pseudo-time stepping: %s must be finite and > 0 (got %r)" % (name, v))
        if self._batch is not None:
            raise ValueError("pseudo-time stepping is not available with mini-batching: the anchors live with the "
                             "evaluated plan (store-level anchors and a gather are a follow-up)")
        if self._visc is not None:
            raise ValueError("pseudo-time stepping is not available with viscosity identification "
                             "(set_viscosity_identification): switch it off first")
        self._pt = _PseudoTime(float(dtau), ev, None if pressure_dtau is None else float(pressure_dtau))

    def _attach_pseudo_time(self):
        """Scratch and record for the new collocation plan, and its first anchors."""
        pt, f = self._pt, self.plan_f
        pt.scratch = ptime_scratch(f.n, self.device)
        pt.record = torch.zeros(PTIME_RECORD, dtype=torch.float64, device=self.device)
        self.reset_pseudo_time()
        pt.record[3:6].zero_()      # (the forced advance measured the drift from the zero-initialised planes)

    def reset_pseudo_time(self):
        """Re-anchor at the current weights: one forward of the collocation plan with the rates at 0 (the fields do not
        depend on the entropy net or the lagged viscosity: neither is read or advanced), then a forced advance.  The
        record's refresh count goes up by one, its update count restarts at 0."""
        pt, f = self._pt, self.plan_f
        if pt is None or f is None:
            raise RuntimeError("pseudo-time stepping is off, or no collocation set is attached")
        f.set_pseudo_time(0.0, 0.0)
        vtm, f.vis_t_minus = f.vis_t_minus, None
        try:
            f.forward(self.Re, scale=self.scale, save=False)
        finally:
            f.vis_t_minus = vtm
        ptime_advance(f, pt.every, True, pt.scratch, pt.record)
        f.set_pseudo_time(pt.sigma, pt.sigma_p)

    def pseudo_time_info(self):
        """dict(dtau, pressure_dtau, sigma, sigma_p, every, kernels, and - one host read of this rank's record -
        steady_sums (sum w eq_k^2, k = 1..3), drift_uv, drift_p (sum w (u-u*)^2 + (v-v*)^2, sum w (p-p*)^2), max_drift,
        since_refresh, refreshes); None when it is off.  The record entries are None before a collocation set is
        attached."""
        pt = self._pt
        if pt is None:
            return None
        out = dict(dtau=pt.dtau, pressure_dtau=pt.pressure_dtau, sigma=pt.sigma, sigma_p=pt.sigma_p, every=pt.every,
                   kernels=None if self.plan_f is None else self.plan_f.kernel_names() + ("ptime_advance_kernel",),
                   steady_sums=None, drift_uv=None, drift_p=None, max_drift=None, since_refresh=None, refreshes=None)
        if pt.record is not None:
            r = pt.record.cpu().numpy()
            out.update(steady_sums=tuple(float(v) for v in r[:3]), drift_uv=float(r[3]), drift_p=float(r[4]),
                       max_drift=float(r[5]), since_refresh=int(r[6]), refreshes=int(r[7]))
        return out

    # ---- device learning-rate schedule and gradient clipping ----
    def set_lr_schedule(self, spec=None):
        """spec = an LrSchedule: the Adam updates of step() and adam_step(lr) use the rate lr_e = spec.value(lr, e) of a
        schedule position e kept in device memory (the update kernel computes it in fp64 from launch constants and
        rounds it to fp32 once) - lr is the base rate lr0, and e advances by one per update, so a captured step
        serves a whole stage.  e is not Adam's step count: reset_adam (the ev freeze schedule) leaves it alone, and
        so does lbfgs_step.  A call restarts e at 0; reset_lr_schedule(e) sets it.  None: off (with clipping off
        too, adam_step makes exactly the calls it makes without the feature)."""
        if spec is not None and not isinstance(spec, _schedule.LrSchedule):
            raise TypeError("set_lr_schedule: an LrSchedule or None (got %r)" % (spec,))
        self._graphs.clear()        # captured steps hold the other schedule's launch constants
        if spec is None and (self._opt is None or self._opt.max_norm == 0.0):
            self._opt = None
            return
        if self._opt is None:
            self._opt = _Optim(self.device)
        self._opt.set_spec(spec)
        self._opt.epoch.zero_()

    def reset_lr_schedule(self, e=0):
        """Set the schedule position to e (in place: captured steps stay valid)."""
        if int(e) < 0:
            raise ValueError("reset_lr_schedule: e must be >= 0")
        if self._opt is not None:
            self._opt.epoch.fill_(int(e))

    def set_grad_clipping(self, max_norm=0.0):
        """max_norm > 0: before every Adam update the gradient is scaled by min(1, max_norm / (||g|| + 1e-6)), the
        formula of torch.nn.utils.clip_grad_norm_, with ||g|| the 2-norm over all trainable nets of the gradient Adam
        is about to consume (after the all-reduce and the loss-balancing or conflict-free combine; every rank computes
        the same value).  One more launch per step, a fixed-order fp64 sum; the scaling happens inside the update, so
        `grads` stays the raw gradient.  A non-finite norm propagates into the parameters, as in torch.  0: off."""
        max_norm = float(max_norm)
        if not (max_norm >= 0.0 and math.isfinite(max_norm)):
            raise ValueError("gradient clipping: max_norm must be finite and >= 0")
        self._graphs.clear()
        if max_norm == 0.0 and (self._opt is None or self._opt.user_spec is None):
            self._opt = None
            return
        if self._opt is None:
            self._opt = _Optim(self.device)
        self._opt.max_norm = max_norm

    def optimizer_info(self):
        """The device record of the last scheduled / clipped update (one host read), or None with both off: epoch
        (the position e it used), lr (the fp32 lr_e), grad_norm and clip_coef (0 and 1 without clipping), clipped
        (updates with coef < 1 so far), updates, next_epoch, and the settings."""
        o = self._opt
        if o is None:
            return None
        r = torch.cat([o.rec, o.epoch.to(torch.float64)]).cpu().tolist()
        return dict(epoch=int(r[0]), lr=r[1], grad_norm=r[2], clip_coef=r[3], clipped=int(r[4]), updates=int(r[5]),
                    next_epoch=int(r[6]), schedule=o.user_spec, max_norm=o.max_norm)

    # ---- validation error on the device and the best weights ----
    def set_validation(self, x, y, u=None, v=None, p=None, every=1000, metric="uv", keep_best=True, history=4096):
        """Track the relative L2 error against the reference fields u, v (and p) at the points x, y on the device.
        After the every-th optimizer update since this call, and every every-th after that (Adam updates of step() and
        adam_step(), and each lbfgs_step call as one), three things follow the update on the main stream: a value
        forward of the main net on the validation points, one launch that folds the error sums in fixed-order fp64,
        writes the record [t, e_u, e_v, e_p, e_p0, metric, improved, n_p] into a history ring of `history` rows and
        updates the monitor state (best metric, its t, validations since the last improvement, non-finite count), and
        - keep_best - one launch that copies the trainable vector of every net into a snapshot when that validation
        improved strictly on the best so far.  Everything is device memory: the captured validating step serves the
        whole stage, and nothing synchronises.  e_c = ||c^ - c|| / ||c|| as a fraction; e_p0 is the pressure error
        after removing the mean of p^ - p and of p; metric: 'uv' (u and v together, the default), 'u', 'v', 'p' or
        'p0'.  A NaN target masks that point for its channel.  Record t is the number of updates since this call, and
        the record describes the parameters after that update.  Several ranks: every rank validates the whole set it
        is given; there is no communication (the parameters are identical, so the records are).

        every = 0 or x = None: off (the step launches what it launches without the feature).  A call restarts the
        state and drops the best; so does a change of the weight factorization."""
        every, history = int(every), int(history)
        if every < 0:
            raise ValueError("validation: every must be >= 0")
        self._graphs.clear()        # captured steps hold the other monitor's buffers and constants
        if every == 0 or x is None:
            self._val = None
            return
        if metric not in VAL_METRICS:
            raise ValueError("validation: metric must be one of %s (got %r)" % (sorted(VAL_METRICS), metric))
        if u is None or v is None:
            raise ValueError("validation: the targets u and v must be given")
        if metric in ("p", "p0") and p is None:
            raise ValueError("validation: metric %r needs pressure targets" % (metric,))
        if history < 1:
            raise ValueError("validation: history must be >= 1")
        m = _Validation(every, metric, bool(keep_best), history, p is not None)
        m.plan = ValuePlan(self.net, x, y, with_backward=False)
        n = m.plan.n
        m.pred, m.tgt = val_planes(n, self.device), val_planes(n, self.device)
        m.plan.pred = m.pred[:, :n]         # the forward writes rows that start 16-byte aligned
        for c, t in enumerate((u, v, p)):
            if t is None:
                continue
            t = torch.as_tensor(np.asarray(t, dtype=np.float32).reshape(-1))
            if t.numel() != n:
                raise ValueError("validation: target %d must have one entry per point" % c)
            m.tgt[c, :n].copy_(t)
        m.scratch = val_scratch(self.device)
        m.state = torch.zeros(VAL_STATE, dtype=torch.float64, device=self.device)
        m.ring = torch.zeros(history, VAL_RECORD, dtype=torch.float64, device=self.device)
        self._val = m
        self._validation_reset()

    def _validation_reset(self):
        """The state at its start, an empty ring and fresh snapshot vectors of the nets' trainable sizes."""
        m = self._val
        if m is None:
            return
        self._graphs.clear()
        m.n = 0
        start = torch.zeros(VAL_STATE, dtype=torch.float64)
        start[1] = float("inf")
        m.state.copy_(start)
        m.ring.zero_()
        m.snap = [torch.zeros_like(net.trainable) for _, net in self._nets()]

    def _validation_due(self):
        """True when the next optimizer update is one the cadence validates after."""
        m = self._val
        return m is not None and (m.n + 1) % m.every == 0

    def _updated(self, validate=None, observe=True, diagnose=None):
        """An optimizer update is in place: count it, let the convergence monitor observe it (observe False: an L-BFGS
        call, whose sums are a trial point's), and validate and diagnose the flow when the cadences (or the caller)
        say so."""
        if self._pt is not None:
            ptime_advance(self.plan_f, self._pt.every, False, self._pt.scratch, self._pt.record)
        if observe and self._mon is not None:
            self._observe()
        m = self._val
        if m is not None:
            due = self._validation_due() if validate is None else validate
            m.n += 1
            if due:
                self._validate(-1.0)
        d = self._flow
        if d is not None:
            due = self._flow_due() if diagnose is None else diagnose
            d.n += 1
            if due:
                self._diagnose(-1.0)

    def _validate(self, t):
        m = self._val
        m.plan.forward(save=False)
        val_stats(m.pred, m.tgt, m.plan.n, m.with_p, VAL_METRICS[m.metric], t, m.every, m.scratch, m.state, m.ring)
        if m.keep_best:
            val_keep([(net.trainable, snap) for (_, net), snap in zip(self._nets(), m.snap)], m.state)

    def _val_on(self):
        if self._val is None:
            raise RuntimeError("validation is off: call set_validation() first")
        return self._val

    def validate(self, t=None):
        """One validation now, of the current parameters, recorded with the explicit position t (default: the updates
        counted since set_validation).  It takes part in the best-so-far like any other.  Returns the row as a dict
        (one host read)."""
        m = self._val_on()
        t = float(m.n if t is None else t)
        if not (math.isfinite(t) and t >= 0.0):
            raise ValueError("validate: t must be finite and >= 0")
        self._validate(t)
        return self.validation_info()["last"]

    def validation_info(self):
        """The monitor state (one host read), or None when the feature is off: records, best_metric, best_t, stale,
        nonfinite, last (the newest row as a dict; None before the first), every, metric, points."""
        m = self._val
        if m is None:
            return None
        st = m.state.cpu().tolist()
        k = int(st[0])
        last = None
        if k > 0:
            last = dict(zip(VAL_ROW, m.ring[(k - 1) % m.capacity].cpu().tolist()))
        return dict(records=k, best_metric=st[1], best_t=st[2], stale=int(st[3]), nonfinite=int(st[4]), last=last,
                    every=m.every, metric=m.metric, points=m.plan.n)

    def validation_history(self):
        """fp64 numpy array [rows, VAL_RECORD] of the recorded rows in time order (the ring unwrapped: the newest
        `history` of them); one host read."""
        m = self._val_on()
        both = torch.cat([m.state, m.ring.reshape(-1)]).cpu().numpy()
        k, ring = int(both[0]), both[VAL_STATE:].reshape(m.capacity, VAL_RECORD)
        if k <= m.capacity:
            return ring[:k].copy()
        return np.concatenate([ring[k % m.capacity:], ring[:k % m.capacity]])

    def _has_best(self):
        m = self._val
        return m is not None and m.keep_best and math.isfinite(float(m.state[1].item()))

    def best_state_dict(self):
        """The main net's effective weights at the best validation so far, in the checkpoint format of state_dict();
        None before the first improvement (or with keep_best off)."""
        if not self._has_best():
            return None
        return self.net.flat_state_dict(self.net.composed(self._val.snap[0]))

    def best_state_dict_e(self):
        """best_state_dict() of the entropy net (ev flavour)."""
        if self.net_e is None or not self._has_best():
            return None
        return self.net_e.flat_state_dict(self.net_e.composed(self._val.snap[1]))

    def best_factors(self):
        """The scale factors inside the snapshot, shaped like weight_factors(); None without factorization or best."""
        if self._rwf is None or not self._has_best():
            return None
        out = {}
        for (name, net), snap in zip(self._nets(), self._val.snap):
            rows, off = [], net.num_params
            for r, _ in layer_shapes(net.n_out, net.n_hidden, net.hidden):
                rows.append(snap[off:off + r].clone())
                off += r
            out[name] = rows
        return out

    def restore_best(self):
        """Copy the snapshot back into the trainable vector of every net (in place: captured steps stay valid) and
        rebuild the effective weights.  Adam's moments and the monitor state are left alone.  RuntimeError without a
        best."""
        if not self._has_best():
            raise RuntimeError("restore_best: there is no best snapshot (validation off, keep_best off, or no "
                               "validation has improved yet)")
        for (_, net), snap in zip(self._nets(), self._val.snap):
            net.trainable.copy_(snap)
            net.update_params()
        self.lbfgs_reset()

    # ---- flow diagnostics: stream function, vorticity and vortices on the device ----
    def set_flow_diagnostics(self, nx=257, ny=257, every=1000, eps=1e-3, history=4096, xs=None, ys=None, domain=None):
        """Record which flow the net describes, on the device.  After the every-th optimizer update since this call,
        and every every-th after that (counted like set_validation's cadence: Adam updates, and each lbfgs_step call as
        one), four launches follow the update on the main stream, behind the pseudo-time advance, the monitor
        observation and the validation: a forward-only residual forward of the main net on the nx x ny tensor grid,
        whose field planes hold u, v and their exact first derivatives; the stream function psi = int u dy by the
        trapezoid rule from the bottom wall; and two launches that reduce psi and the planes in fixed-order fp64 to one
        row of a history ring of `history` rows (FLOW_ROW):
          t, x_c, y_c, psi_min, omega_c           the primary vortex: argmin psi, its centre refined inside the cell
          x, y, psi_max, area per quadrant        bl, br, tl, tr of the grid's midlines, the lid row left out: the
                                                  strongest counter-rotating node and the fraction of all nodes that
                                                  lie in the quadrant with psi > eps |psi_min|
          counter_area                            the four areas added: 0.06 for the DNS flow at Re 2000, 0.46 for
                                                  the other steady branch plain NSFnet can land on
          mass_defect, ke, enstrophy, div_rms, div_max, nonfinite
        with omega = v_x - u_y and div = u_x + v_y.  A field with a non-finite node records NaN for everything but t
        and nonfinite.  Everything is device memory: the captured diagnosing step serves the whole stage and nothing
        synchronises; the training is not changed by it.  Several ranks: every rank computes the same record.

        xs, ys: the grid's coordinates (strictly increasing, at least 3 each; they are held in fp32 like every
        point set) instead of nx / ny equidistant ones over domain = (x0, x1, y0, y1).  All three are in the net's
        input coordinates, as every point set is.  The domain defaults to where the cavity lies in them: the box of
        the hard walls when they are on, else the unit square at coordinate scale 1 and [-1, 1]^2 at scale 2 (the
        map 2 x - 1 of the ev data loader); any other scale without hard walls is refused.  The record is physical:
        the field planes hold physical derivatives (the sweeps multiply by the scale), so psi is integrated over, and
        every centre is given in, x = (xi - o) / scale with o the cavity's lower-left corner in input coordinates
        (the hard walls' origin, else (0, 0) or (-1, -1)); at scale 1 without hard walls that is xi itself.  The scale
        is the one in force at this call; a diagnostic after it has changed raises.  Area is a node fraction: an area
        only on a uniform grid.  The quadrant maxima are not connected regions: one that spans quadrants shows in several rows.
        Like every point set the grid must be attached after set_hard_boundary / set_fourier_features.

        every = 0: off (the step launches what it launches without the feature).  A call restarts the record."""
        every, history = int(every), int(history)
        if every < 0:
            raise ValueError("flow diagnostics: every must be >= 0")
        self._graphs.clear()        # captured steps hold the other grid's buffers and constants
        if every == 0:
            self._flow = None
            return
        eps = float(eps)
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError("flow diagnostics: eps must be finite and >= 0")
        if history < 1:
            raise ValueError("flow diagnostics: history must be >= 1")
        bc, scale = self.hard_boundary_info(), float(self.scale)
        if bc is not None:
            origin, side = bc["origin"], 1.0 / bc["inv_len"]
        elif scale in (1.0, 2.0):
            origin, side = ((0.0, 0.0), 1.0) if scale == 1.0 else ((-1.0, -1.0), 2.0)
        else:
            raise ValueError("flow diagnostics: coordinate scale %g is neither the plain cavity's nor the [-1, 1] map's, "
                             "and no hard walls say where the cavity lies" % scale)
        if domain is None:
            domain = (origin[0], origin[0] + side, origin[1], origin[1] + side)
        x0, x1, y0, y1 = (float(c) for c in domain)
        axes = []
        for name, given, count, lo, hi in (("xs", xs, nx, x0, x1), ("ys", ys, ny, y0, y1)):
            if given is None:
                count = int(count)
                if count < 3:
                    raise ValueError("flow diagnostics: n%s must be >= 3 (got %d)" % (name[0], count))
                if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
                    raise ValueError("flow diagnostics: domain must be finite with x0 < x1 and y0 < y1")
                given = np.linspace(lo, hi, count)
            c = np.asarray(given, dtype=np.float64).reshape(-1).astype(np.float32)
            if c.size < 3:
                raise ValueError("flow diagnostics: %s must have at least 3 entries (got %d)" % (name, c.size))
            if not (np.all(np.isfinite(c)) and np.all(np.diff(c) > 0)):
                raise ValueError("flow diagnostics: %s must be finite and strictly increasing in fp32" % name)
            axes.append(c)
        cx, cy = axes
        nx, ny = cx.size, cy.size
        if nx * ny > 1 << 30:
            raise ValueError("flow diagnostics: nx * ny must be at most 2^30 (got %d)" % (nx * ny))
        d = _FlowDiag(nx, ny, every, eps, history)
        d.plan = ResidualPlan(self.net, np.tile(cx, ny), np.repeat(cy, nx), with_backward=False)
        d.scale = scale
        # physical coordinates, fp64 from the fp32 ones the plan holds (at scale 1 and origin 0: those, widened)
        d.xs = torch.as_tensor((cx.astype(np.float64) - origin[0]) / scale).to(self.device)
        d.ys = torch.as_tensor((cy.astype(np.float64) - origin[1]) / scale).to(self.device)
        d.psi = torch.zeros(nx * ny, dtype=torch.float64, device=self.device)
        d.scratch = flow_scratch(self.device)
        d.state = torch.zeros(FLOW_STATE, dtype=torch.float64, device=self.device)
        d.ring = torch.zeros(history, FLOW_RECORD, dtype=torch.float64, device=self.device)
        self._flow = d

    def _flow_due(self):
        """True when the next optimizer update is one the cadence diagnoses after."""
        d = self._flow
        return d is not None and (d.n + 1) % d.every == 0

    def _flow_forward(self):
        d = self._flow
        if self.scale != d.scale:
            raise RuntimeError("flow diagnostics: the coordinate scale changed from %g to %g since set_flow_diagnostics; "
                               "call it again" % (d.scale, self.scale))
        d.plan.forward(self.Re, scale=self.scale, save=False)
        flow_stream_function(d.plan.fields, d.nx, d.ny, d.ys, d.psi)

    def _diagnose(self, t):
        d = self._flow
        self._flow_forward()
        flow_stats(d.plan.fields, d.nx, d.ny, d.xs, d.ys, d.psi, d.eps, t, d.every, d.scratch, d.state, d.ring)

    def _flow_on(self):
        if self._flow is None:
            raise RuntimeError("flow diagnostics are off: call set_flow_diagnostics() first")
        return self._flow

    def flow_diagnostics(self, t=None):
        """One record now, of the current parameters, with the explicit position t (default: the updates counted since
        set_flow_diagnostics).  Returns the row as a dict (one host read)."""
        d = self._flow_on()
        t = float(d.n if t is None else t)
        if not (math.isfinite(t) and t >= 0.0):
            raise ValueError("flow_diagnostics: t must be finite and >= 0")
        self._diagnose(t)
        return self.flow_info()["last"]

    def flow_info(self):
        """The state (one host read), or None when the feature is off: records, nonfinite (records of a field with
        non-finite nodes), last (the newest row as a dict; None before the first), every, eps, nx, ny."""
        d = self._flow
        if d is None:
            return None
        st = d.state.cpu().tolist()
        k = int(st[0])
        last = None
        if k > 0:
            last = dict(zip(FLOW_ROW, d.ring[(k - 1) % d.capacity].cpu().tolist()))
        return dict(records=k, nonfinite=int(st[2]), last=last, every=d.every, eps=d.eps, nx=d.nx, ny=d.ny)

    def flow_history(self):
        """fp64 numpy array [rows, FLOW_RECORD] of the recorded rows in time order (the ring unwrapped: the newest
        `history` of them; columns FLOW_ROW, then +0); one host read."""
        d = self._flow_on()
        both = torch.cat([d.state, d.ring.reshape(-1)]).cpu().numpy()
        k, ring = int(both[0]), both[FLOW_STATE:].reshape(d.capacity, FLOW_RECORD)
        if k <= d.capacity:
            return ring[:k].copy()
        return np.concatenate([ring[k % d.capacity:], ring[:k % d.capacity]])

    def flow_fields(self, refresh=True):
        """The streamline / vorticity data on the grid, as device tensors shaped [ny, nx]: psi (fp64) and u, v, p,
        omega, div (fp32), with the physical xs [nx] and ys [ny] (fp64).  refresh: evaluate the current parameters first (a forward
        and the stream function, no record); otherwise the planes are those of the last diagnostic.  psi, u, v and p
        are views that the next diagnostic rewrites."""
        d = self._flow_on()
        if refresh:
            self._flow_forward()
        n, shape = d.nx * d.ny, (d.ny, d.nx)
        f = lambda name: d.plan.fields[FLD[name], :n].view(shape)
        return dict(psi=d.psi.view(shape), u=f("u"), v=f("v"), p=f("p"), omega=f("v_x") - f("u_y"),
                    div=f("u_x") + f("v_y"), xs=d.xs, ys=d.ys)

    # ---- convergence monitor: a stage that has stopped making progress ----
    def set_convergence_monitor(self, every=1, window=1000, min_rel_improvement=1e-3, patience=3, re_eff_tol=None,
                                min_updates=0, quantity="loss", mode="any", history=4096):
        """Watch the loss terms (and, ev flavour, Re_eff = 1 / (1/Re + mean vis_t)) of every every-th Adam update on
        the device.  One launch after the update (between the pseudo-time advance and the validation) forms loss,
        loss_e, loss_b, loss_s, eq1..4, the global mean of vis_t and Re_eff in fp64 from the exchanged loss sums of the
        evaluation that produced the update, writes them as a row [t, loss, loss_e, loss_b, loss_s, eq1..eq4, vis_mean,
        Re_eff, stop code] into a ring of `history` rows and adds the monitored `quantity` ('loss' | 'loss_e' |
        'loss_b') and Re_eff to the sums of the current window of `window` observations.  A complete window's means are
        compared with the previous window's: (prev - mean) / |prev| < min_rel_improvement counts as stale, |mean_re -
        prev_re| / prev_re < re_eff_tol as settled (anything else restarts that count; the first window only sets the
        means); from update min_updates on, `patience` stale windows in a row set the sticky stop bit 'plateau',
        `patience` settled ones the bit 're_eff'.  A non-finite loss sets 'nonfinite' at once and stays out of the
        window.  A tolerance of None switches its criterion off.  The launch only sets bits: should_stop() - one host
        read, meant for log points - combines the two criteria by mode ('any': either; 'all': every criterion that is
        on), and 'nonfinite' always stops.  Window means, not moving averages: they ride over the loss jump where the ev
        schedule re-creates Adam, and have an exact numpy statement (tests/monitor_model.py).

        Ev flavour: one more launch per evaluation sums the vis_t plane of the plan that was evaluated (the batch plan
        under mini-batching) into slot 4 of the equation block of the loss sums, before the exchange - so the mean is
        global, and every rank takes the same decision from the same bits; this rank's own max and cap fraction are in
        monitor_info().  An lbfgs_step does not observe.  The loss terms are those of loss_terms(): with batching the
        batch's, with attention the weighted ones, with pseudo-time the minimised loss_e.  Everything is device memory
        allocated here once and rewritten in place: one captured step serves a whole stage, and monitor_history() is a
        full training curve without a synchronisation in between.  Refused: re_eff_tol on the plain flavour (no
        vis_t), chunked collocation passes, the 'L2' loss mode.  The defaults are guesses: no value has been compared
        in training.  every = 0: off (the step launches what it launches without the feature).  A call restarts the
        state."""
        every, window, patience, min_updates, history = (int(v) for v in (every, window, patience, min_updates, history))
        if every < 0:
            raise ValueError("convergence monitor: every must be >= 0")
        if every > 0 and self._visc is not None:
            raise ValueError("the convergence monitor is not available with viscosity identification "
                             "(set_viscosity_identification): its Re_eff is built on the configured Re")
        if every > 0 and self._rc is not None:
            raise ValueError("the convergence monitor is not available with Reynolds-number continuation "
                             "(set_reynolds_continuation): its Re_eff and plateau rule assume a fixed problem")
        self._graphs.clear()        # captured steps hold the other monitor's buffers and constants
        if every == 0:
            self._mon = None
            return
        if window < 1 or patience < 1 or history < 1 or min_updates < 0:
            raise ValueError("convergence monitor: window, patience and history must be >= 1, min_updates >= 0 (got "
                             "window=%d patience=%d history=%d min_updates=%d)" % (window, patience, history, min_updates))
        tol = {}
        for name, v in (("min_rel_improvement", min_rel_improvement), ("re_eff_tol", re_eff_tol)):
            tol[name] = None if v is None else float(v)
            if v is not None and not (math.isfinite(tol[name]) and tol[name] >= 0.0):
                raise ValueError("convergence monitor: %s must be finite and >= 0, or None (got %r)" % (name, v))
        if quantity not in MON_QUANTITIES:
            raise ValueError("convergence monitor: quantity must be one of %s (got %r)" % (sorted(MON_QUANTITIES), quantity))
        if mode not in ("any", "all"):
            raise ValueError("convergence monitor: mode must be 'any' or 'all' (got %r)" % (mode,))
        if tol["re_eff_tol"] is not None and self.net_e is None:
            raise ValueError("convergence monitor: re_eff_tol needs the ev flavour (the plain flavour has no vis_t)")
        _refuse_chunked(_Monitor, isinstance(self.plan_f, ChunkedResidual))
        m = _Monitor(every, window, tol["min_rel_improvement"], patience, tol["re_eff_tol"], min_updates, quantity, mode,
                     history)
        m.state = torch.zeros(MON_STATE, dtype=torch.float64, device=self.device)
        m.ring = torch.zeros(history, MON_RECORD, dtype=torch.float64, device=self.device)
        m.info = torch.zeros(MON_INFO, dtype=torch.float64, device=self.device)
        m.scratch = monitor_scratch(self.device) if self.net_e is not None else None
        self._mon = m

    def reset_convergence_monitor(self):
        """The state at its start and an empty ring (in place: captured steps stay valid)."""
        m = self._mon_on()
        m.state.zero_()
        m.ring.zero_()
        m.info.zero_()

    def _mon_on(self):
        if self._mon is None:
            raise RuntimeError("the convergence monitor is off: call set_convergence_monitor() first")
        return self._mon

    def _observe(self):
        """The observation of the update that is in place, from the sums of the evaluation that produced it."""
        m, s = self._mon, self.sums
        sup_on = self._sup_on()
        n_eq = self._batch.B * self.world_size if self._eval_batch else self.n_f_global
        monitor_observe(s[S_EQ:S_EQ + NLOSS], s[S_BC:S_BC + NLOSS], s[S_SUP:S_SUP + NLOSS] if sup_on else None,
                        None if self._bal is None else self._bal.lam, self.alpha_b, self.alpha_s, self.alpha_e,
                        self._w4(), n_eq, self.n_b_global, self.n_s_global if sup_on else 0,
                        self._n_p_valid_global() if sup_on else 0, self.Re, m.c_struct(self.net_e is not None), m.state,
                        m.ring)

    def _stop_reasons(self, code, m):
        """The names of the bits in `code`, and whether they end the stage under m.mode."""
        reasons = [k for k, bit in MON_STOP.items() if code & bit]
        on = [k for k, v in (("plateau", m.min_rel), ("re_eff", m.re_tol)) if v is not None]
        hit = [k in reasons for k in on]
        stop = "nonfinite" in reasons or (bool(on) and (any(hit) if m.mode == "any" else all(hit)))
        return reasons, stop

    def monitor_info(self):
        """The monitor state (one host read), or None when the feature is off: updates, observations, nonfinite,
        windows, window_mean / window_mean_re (of the last complete window), stale, settled, stop (the code), reasons
        (the names of its bits), should_stop, t_plateau / t_re_eff / t_nonfinite (the update that set each bit; 0:
        not set), last (the newest row as a dict; None before the first), and this rank's vis_t_max and cap_fraction
        (entries >= vis_t0; None on the plain flavour or before the first evaluation), with the settings."""
        m = self._mon
        if m is None:
            return None
        k = torch.remainder(m.state[1:2] - 1.0, float(m.capacity)).long()       # the newest row (device index: no sync)
        both = torch.cat([m.state, m.info, m.ring.index_select(0, k).reshape(-1)]).cpu().tolist()
        st, info, row = both[:MON_STATE], both[MON_STATE:MON_STATE + MON_INFO], both[MON_STATE + MON_INFO:]
        out = dict(zip(MON_STATE_NAMES, st))
        for key in MON_STATE_NAMES:
            if key not in ("window_sum", "window_sum_re", "window_mean", "window_mean_re"):
                out[key] = int(out[key])
        out["reasons"], out["should_stop"] = self._stop_reasons(out["stop"], m)
        out["last"] = dict(zip(MON_ROW, row)) if out["observations"] > 0 else None
        seen = self.net_e is not None and info[3] > 0
        out["vis_t_max"] = info[0] if seen else None
        out["cap_fraction"] = info[1] / info[3] if seen else None
        out.update(every=m.every, window=m.window, min_rel_improvement=m.min_rel, patience=m.patience,
                   re_eff_tol=m.re_tol, min_updates=m.min_updates, quantity=m.quantity, mode=m.mode, history=m.capacity)
        return out

    def monitor_history(self):
        """fp64 numpy array [rows, MON_RECORD] of the observed rows in time order (the ring unwrapped: the newest
        `history` of them); one host read."""
        m = self._mon_on()
        both = torch.cat([m.state, m.ring.reshape(-1)]).cpu().numpy()
        k, ring = int(both[1]), both[MON_STATE:].reshape(m.capacity, MON_RECORD)
        if k <= m.capacity:
            return ring[:k].copy()
        return np.concatenate([ring[k % m.capacity:], ring[:k % m.capacity]])

    def should_stop(self):
        """True when the stop bits end the stage under the configured mode (one host read; False with the monitor
        off).  Every rank reads the same bits."""
        m = self._mon
        if m is None:
            return False
        return self._stop_reasons(int(m.state[11].item()), m)[1]

    # ---- identification of the viscosity from data ----
    def set_viscosity_identification(self, re0=None, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, re_bounds=(1e-2, 1e6),
                                     enabled=True):
        """Make the molecular viscosity nu = 1 / Re a trainable scalar (the inverse problem of Raissi, Perdikaris &
        Karniadakis 2019: with measurements attached by set_supervised, the flow's Reynolds number is identified along
        with the field).  nu lives in device memory as one fp32 that every residual launch of the engine's plans reads
        in place of 1 / Re - the collocation plan, the batch plan, the resampling pool - and the evaluated plan's
        forward also leaves Lap u, Lap v.  Every evaluation made for Adam is followed by one streaming launch that forms
        S = sum_i w_i ((eq1 + w4 eq4 (u - 1/2)) Lap u + (eq2 + w4 eq4 (v - 1/2)) Lap v) in fp64 with a fixed order and
        puts it into slot 5 of the equation block of the loss sums, before the exchange: with several ranks the sum is
        global in the message that is sent anyway, and every rank updates from the same bits.  adam_step then runs, after
        the nets' updates, one launch of torch-Adam in fp64 on theta = ln nu with d loss / d theta = nu (-(2 alpha_e / N) S)
        (N: the global collocation count, or batch_points x world size under mini-batching), its own rate `lr`, betas and
        eps, theta clamped to ln(1 / re_bounds[1]) .. ln(1 / re_bounds[0]).  Both launches are part of the captured step.
        The nets' schedule and clipping do not see the scalar.

        re0: the starting estimate (None: the engine's Re).  The engine's Re itself stays what it was configured: with
        the ev flavour vis_t0 = vis_t0_factor / Re keeps its configured value.  nu is held fixed during lbfgs_step and
        by loss_and_grad(full_batch=True).  viscosity_info() reads the estimate.

        Refused with ValueError, each way round: pseudo-time stepping, conflict-free gradients, the convergence monitor
        (whose Re_eff is built on the configured Re), chunked collocation passes and the loss mode 'L2'.  lr None or
        enabled False: off - the plans carry no pointer and the step launches what it launches without the feature.
        A call restarts the scalar's optimiser at re0."""
        self._graphs.clear()        # captured steps hold the other mode's launches and pointers
        if not enabled or lr is None:
            if self._visc is not None:
                self._visc = None
                for plan, _ in self._visc_plans():
                    plan.set_viscosity(None)
            return
        if self._rc is not None:
            raise ValueError("viscosity identification is not available with Reynolds-number continuation "
                             "(set_reynolds_continuation): both own nu - switch it off first")
        re0 = self.Re if re0 is None else float(re0)
        lr, eps, betas = float(lr), float(eps), (float(betas[0]), float(betas[1]))
        re_bounds = (float(re_bounds[0]), float(re_bounds[1]))
        if not (math.isfinite(lr) and lr >= 0.0 and math.isfinite(eps) and eps > 0.0):
            raise ValueError("viscosity identification: lr must be finite and >= 0, eps finite and > 0 (got lr=%r eps=%r)"
                             % (lr, eps))
        if not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError("viscosity identification: betas must lie in [0, 1) (got %r)" % (betas,))
        if not (0.0 < re_bounds[0] <= re_bounds[1] and math.isfinite(re_bounds[1])):
            raise ValueError("viscosity identification: re_bounds must be 0 < re_min <= re_max < inf (got %r)" % (re_bounds,))
        if not (math.isfinite(re0) and re_bounds[0] <= re0 <= re_bounds[1]):
            raise ValueError("viscosity identification: re0 must lie inside re_bounds (got re0=%r, bounds %r)"
                             % (re0, re_bounds))
        for state, what in ((self._pt, "pseudo-time stepping (set_pseudo_time)"),
                            (self._cfg, "conflict-free gradients (set_conflict_free_gradients)"),
                            (self._mon, "the convergence monitor (set_convergence_monitor), whose Re_eff is built on "
                                        "the configured Re")):
            if state is not None:
                raise ValueError("viscosity identification is not available with %s: switch it off first" % what)
        _refuse_chunked(_Viscosity, isinstance(self.plan_f, ChunkedResidual))
        vs = _Viscosity(re0, lr, betas, eps, re_bounds)
        vs.state = torch.zeros(VISC_STATE, dtype=torch.float64, device=self.device)
        vs.nu = torch.zeros(1, dtype=torch.float32, device=self.device)
        vs.start()
        self._visc = vs
        for plan, with_lap in self._visc_plans():
            self._attach_viscosity(plan, with_lap)

    def _visc_plans(self):
        """[(residual plan, it is evaluated for a gradient)] of every residual plan the engine owns."""
        bt = self._batch
        return [(p, lap) for p, lap in ((self.plan_f, True), (None if bt is None else bt.f, True), (self._pool, False))
                if p is not None]

    def _attach_viscosity(self, plan, with_lap=True):
        vs = self._visc
        plan.set_viscosity(vs.nu, with_lap)
        if with_lap:
            s = visc_scratch(plan.n, self.device)
            if vs.scratch is None or s.numel() > vs.scratch.numel():
                vs.scratch = s

    def viscosity_info(self):
        """dict(Re, nu, theta, grad (the last d loss / d nu), updates, skipped (updates left out for a non-finite sum),
        m, v, and the settings re0, lr, betas, eps, re_bounds) - one host read; None when the feature is off."""
        vs = self._visc
        if vs is None:
            return None
        both = torch.cat([vs.state, vs.nu.double()]).cpu().tolist()
        out = dict(zip(VISC_STATE_NAMES, both[:VISC_STATE]))
        nu = both[VISC_STATE]
        out.update(nu=nu, Re=1.0 / nu if nu > 0.0 else float("inf"), updates=int(out["updates"]), skipped=int(out["skipped"]),
                   re0=vs.re0, lr=vs.lr, betas=vs.betas, eps=vs.eps, re_bounds=vs.re_bounds)
        return out

    # ---- continuation in the Reynolds number ----
    def set_reynolds_continuation(self, re_start, updates, hold=0, shape="geometric", stairs=0, follow_vis_t0=True,
                                  enabled=True):
        """Ramp the molecular viscosity nu = 1 / Re from 1 / re_start to that of the engine's configured Re while
        training, so that a steady high-Re solve follows the solution branch from a viscous, easy problem instead of
        searching for it.  nu lives in device memory as one fp32 that every residual launch of the engine's plans reads
        in place of 1 / Re - the collocation plan, the batch plan, the resampling pool - and, ev flavour with
        follow_vis_t0, so does the cap vis_t0 = vis_t0_factor / Re of the artificial viscosity: the ramp then is a
        continuation of one problem.  A position counter in device memory counts Adam updates; adam_step runs, after
        the nets' updates, one one-workgroup launch that moves it on and rewrites nu, the cap and a record for
        continuation_info().  The launch is part of the captured step: one hipGraph serves the whole ramp.

        With t updates made, s = clamp((t - hold) / updates, 0, 1); stairs = K > 0 lowers s to floor(s K) / K (s = 1
        stays).  shape 'geometric' (ln nu linear in s; the default: Re spans a decade), 'linear_re' (Re linear in s) or
        'linear_nu'; fp64, rounded once to fp32.  At s = 0 and s = 1 the launch writes the fp32 values the residual
        launches would form from Re = re_start and from the configured Re (and vis_t0) as constants: a finished ramp
        computes what a plain engine at Re computes, bit for bit.

        nu is held during lbfgs_step and by evaluations alone (loss_and_grad without adam_step); the position is not
        an optimiser's state and survives reset_adam.  Refused with ValueError, each way round: viscosity
        identification (both own nu), the convergence monitor (its Re_eff and plateau rule assume a fixed problem),
        chunked collocation passes and the loss mode 'L2'.  enabled False: off - the plans carry no pointer and the
        step launches what it launches without the feature.  A call restarts the ramp at position 0.

        The ends are fixed by the call: the engine's Re and vis_t0 as they stand then (cap = vis_t0 Re / Re_t, which is
        vis_t0_factor unless vis_t0 was assigned since construction).  While the ramp is on the residual launches read
        the scalars, so an engine.Re or engine.vis_t0 assigned afterwards does not reach them: call again."""
        self._graphs.clear()        # captured steps hold the other mode's launches and pointers
        if not enabled:
            if self._rc is not None:
                self._rc = None
                for plan, _ in self._visc_plans():
                    plan.set_viscosity(None)
            return
        re_start = float(re_start)
        if not (math.isfinite(re_start) and re_start > 0.0):
            raise ValueError("Reynolds-number continuation: re_start must be finite and > 0 (got %r)" % (re_start,))
        if int(updates) != updates or int(hold) != hold or int(stairs) != stairs:
            raise ValueError("Reynolds-number continuation: updates, hold and stairs must be integers (got %r, %r, %r)"
                             % (updates, hold, stairs))
        updates, hold, stairs = int(updates), int(hold), int(stairs)
        if updates <= 0 or hold < 0 or stairs < 0:
            raise ValueError("Reynolds-number continuation: updates must be > 0, hold and stairs >= 0 (got updates=%d "
                             "hold=%d stairs=%d)" % (updates, hold, stairs))
        if shape not in RAMP_SHAPES:
            raise ValueError("Reynolds-number continuation: shape must be one of %s (got %r)" % (sorted(RAMP_SHAPES), shape))
        for state, what in ((self._visc, "viscosity identification (set_viscosity_identification): both own nu"),
                            (self._mon, "the convergence monitor (set_convergence_monitor), whose Re_eff and plateau "
                                        "rule assume a fixed problem")):
            if state is not None:
                raise ValueError("Reynolds-number continuation is not available with %s - switch it off first" % what)
        _refuse_chunked(_Continuation, isinstance(self.plan_f, ChunkedResidual))
        rc = _Continuation(self, re_start, updates, hold, shape, stairs, bool(follow_vis_t0))
        rc.place(0)
        self._rc = rc
        for plan, _ in self._visc_plans():
            self._attach_continuation(plan)

    def _attach_continuation(self, plan):
        """The scalars onto a residual plan: no Laplacian planes (nothing differentiates by nu)."""
        plan.set_viscosity(self._rc.nu, with_lap=False)
        if self._rc.cap is not None:
            plan.set_viscosity_cap(self._rc.cap)

    def _rc_on(self):
        if self._rc is None:
            raise RuntimeError("Reynolds-number continuation is off: call set_reynolds_continuation() first")
        return self._rc

    def reset_reynolds_continuation(self, t=0):
        """Put the ramp at position t (Adam updates made): nu, the cap and the record become those of t, in place -
        captured steps stay valid.  The values come from the host's evaluation of the schedule: for 'geometric' a placed
        position inside the ramp may differ from a stepped one in the last bit of the fp32 (the next step rewrites them
        from the position alone)."""
        if int(t) != t or int(t) < 0:
            raise ValueError("Reynolds-number continuation: the position must be an integer >= 0 (got %r)" % (t,))
        self._rc_on().place(int(t))

    def continuation_info(self):
        """dict(t, s, Re_t, nu_t, cap_t (None without a cap), done, and the settings re_start, re_end, updates, hold,
        shape, stairs, follow_vis_t0) of the ramp - one host read; None when the feature is off."""
        rc = self._rc
        if rc is None:
            return None
        out = dict(zip(RAMP_RECORD_NAMES, rc.rec.cpu().tolist()))
        out.update(t=int(out["t"]), done=bool(out["done"]), cap_t=out["cap_t"] if rc.cap is not None else None,
                   re_start=rc.re_start, re_end=self.Re, updates=rc.updates, hold=rc.hold, shape=rc.shape,
                   stairs=rc.stairs, follow_vis_t0=rc.follow)
        return out

    # ---- L-BFGS ----
    def lbfgs_reset(self):
        """Forget the L-BFGS history: the next lbfgs_step starts like a fresh torch.optim.LBFGS."""
        self._lbfgs_state = _lbfgs.LbfgsState()

    def lbfgs_step(self, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9,
                   history_size=100, line_search_fn=None, owner=None):
        """torch.optim.LBFGS.step(closure) on the full-batch MSE loss of the main net (every rank computes the same
        direction from the all-reduced gradient).  The state persists across calls.  Ev flavour: the entropy net is
        frozen for the whole call and vis_t_minus is refreshed from it first (init_vis_t), so every evaluation sees
        the same viscosity.  Adam's moments and step counters are not touched.  Returns the loss at entry.

        The state belongs to `owner` (the solvers pass their torch.optim.LBFGS object): a call with another owner
        than the previous one starts fresh, as a new torch.optim.LBFGS does.  With the same owner the state carries
        on across calls - also across Adam steps or changed loss weights in between, exactly as the state of one
        torch.optim.LBFGS object does."""
        _lbfgs.check_knobs(lr, max_iter, max_eval, history_size, line_search_fn)
        if self._lbfgs is None or self._lbfgs.history_size != int(history_size):
            self._lbfgs = LbfgsHistory(self.net.num_train, int(history_size), self.device)
            self.lbfgs_reset()
        if self._lbfgs_owner is _RESTORED:      # load_training_state: the restored state is this owner's from here on
            self._lbfgs_owner = owner
        if owner is not self._lbfgs_owner:
            self.lbfgs_reset()
            self._lbfgs_owner = owner
        e_trainable = self.e_trainable
        if self.net_e is not None:
            self.e_trainable = False
            self.init_vis_t()
        space = _EngineSpace(self, self._lbfgs)
        try:
            with self._evaluating(EVAL_LBFGS):      # the objective: one set of points, weights and terms throughout
                loss, info = _lbfgs.step(space, self._lbfgs_state, lr=float(lr), max_iter=int(max_iter),
                                         max_eval=max_eval, tolerance_grad=float(tolerance_grad),
                                         tolerance_change=float(tolerance_change), line_search_fn=line_search_fn)
        finally:
            self.e_trainable = e_trainable
        self.lbfgs_info = info
        self._updated(observe=False)     # one call = one update; the accepted point is in place
        return loss

    def step(self, lr):
        """loss + gradient + (all-reduce) + Adam.  With NSFNET_GRAPH=1 the launch sequence is captured
        once per (lr, schedule state) in a hipGraph and replayed.  Opt-in: measured on MI355X the eager
        launch sequence (~14 launches, all asynchronous) already keeps the GPU busy down to the 4x50 /
        10 k-point step (0.12 ms), and replay is 0-6 % slower; it pays only when the host is contended."""
        if not self._graphs_enabled():
            self.loss_and_grad()
            self.adam_step(lr)
            return
        # with balancing on, a balance step and a plain step are separate graphs (the weights are device state)
        update = self._balance_due()
        validate = self._validation_due()       # a validating step and a plain one are separate graphs, too
        diagnose = self._flow_due()             # and so are a diagnosing step and one that does both
        key = self._graph_key(lr, update, validate, diagnose)
        g = self._graphs.get(key)
        if g is None:
            # first use of this configuration: run it eagerly once (lazy host-side setup such as the
            # supervised-target census happens here), then capture
            self._loss_and_grad(update)
            self.adam_step(lr, validate, diagnose)
            if len(self._graphs) >= 8:
                self._graphs.clear()
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    self._loss_and_grad(update)
                    self.adam_step(lr, validate, diagnose)
            torch.cuda.current_stream(self.device).wait_stream(side)
            self._count_updates(-1)      # the capture itself does not execute
            self._graphs[key] = graph
            return
        g.replay()
        self._eval_batch = self._batching_on()
        self._count_updates(1)

    def _graph_key(self, lr, update, validate=False, diagnose=False):
        """What a captured step depends on besides device memory: the launch constants of the engine and of every
        option that is on (lr is the base rate lr0 under a schedule: the rate of each update is device state).  The
        head holds balancing, batching, attention, the schedule and the factorization (which lives on the nets)."""
        bt, a, o = self._batch, self._rba, self._opt
        key = (float(lr), self.e_trainable, self.alpha_evm, self.alpha_b, self.alpha_e, self.alpha_s, self.scale,
               self.n_f_global, self.n_b_global, self.n_s_global, self.Re, self.vis_t0, self.eq4_weight,
               self._bal is not None, update, 0 if bt is None else bt.B,
               (False, 0.0, 0.0) if a is None else (True, a.gamma, a.eta))
        key += () if o is None else (o.spec.key(), o.max_norm)
        key += () if self._rwf is None else ("rwf",)
        for option in self._options():
            key += option.graph_key()
        v = self._val
        key += ("diagnose",) if diagnose else ()        # (the grid, the cadence and eps: the option's graph_key)
        return key + (("validate", v.every, v.metric, v.keep_best, v.plan.n, v.with_p) if validate else ())

    def _graphs_enabled(self):
        flag = os.environ.get("NSFNET_GRAPH")
        return flag is not None and flag not in ("0", "", "false", "False") and self.device.type == "cuda"

    # ---- training-state snapshots that resume bit for bit ----
    def _state_segments(self, lbfgs=None):
        """[(name, tensor, stored)]: everything in device memory that a step reads and an earlier step wrote, in the
        file's fixed order - per net (net, net_e) trainable, m, v, adam_t; per collocation pass x, y, w (the static
        weights), vis_t_minus; plan_e x, y; what every option that is on names as `stored`, in the order of _OPTIONS
        (opt epoch, rec; bal lam, rec; cfg coef, rec; batch counter, idx; rba lam, w, rec; val state, ring; monitor
        state, ring; visc state, nu); ptime anchor, record; val snap per net; lbfgs ws, d, x0 - and then, digested but
        not stored (stored False), the sets a resume must attach again unchanged: boundary, supervised, validation,
        resample pool."""
        segs = []

        def add(name, t, stored=True):
            if t is not None:
                segs.append((name, t, stored))

        for name, net in self._nets():
            for key, t in (("trainable", net.trainable), ("m", net.m), ("v", net.v), ("adam_t", net.adam_t_dev)):
                add("%s.%s" % (name, key), t)
        if self.plan_f is not None:
            for i, (_, p) in enumerate(_passes(self.plan_f)):
                add("colloc.%d.x" % i, p.x)
                add("colloc.%d.y" % i, p.y)
                add("colloc.%d.w" % i, self._rba.s if self._rba is not None else p.w)
                add("colloc.%d.vis_t_minus" % i, p.vis_t_minus)
        if self.plan_e is not None:
            add("plan_e.x", self.plan_e.x)
            add("plan_e.y", self.plan_e.y)
        for option in self._options():
            for key in option.stored[1:]:
                add("%s.%s" % (option.stored[0], key), getattr(option, key))
        # the file's order has two special cases: the pseudo-time anchors (they live on the plan) and record come
        # behind every option's `stored` tensors, and the validation snapshots behind those
        if self._pt is not None and self.plan_f is not None:
            add("ptime.anchor", self.plan_f.anchor)
            add("ptime.record", self._pt.record)
        if self._val is not None:
            for i, t in enumerate(self._val.snap):
                add("val.snap.%d" % i, t)
        lbfgs = lbfgs if lbfgs is not None else self._lbfgs     # (a load hands in the workspace it is about to adopt)
        if lbfgs is not None:
            for key in ("ws", "d", "x0"):
                add("lbfgs.%s" % key, getattr(lbfgs, key))
        for name, plan in (("boundary", self.plan_b), ("supervised", self.plan_s),
                           ("val", None if self._val is None else self._val.plan), ("pool", self._pool)):
            if plan is not None:
                add("%s.x" % name, plan.x, False)
                add("%s.y" % name, plan.y, False)
                for c, t in enumerate(getattr(plan, "targets", ())):
                    add("%s.target%d" % (name, c), t, False)
        if self._val is not None:
            add("val.tgt", self._val.tgt, False)
        add("pool.w", self._pool_w, False)
        if self._flow is not None:
            add("flow.xs", self._flow.xs, False)
            add("flow.ys", self._flow.ys, False)
        return segs

    def _state_fingerprint(self):
        """The structure a file must share with the engine that loads it."""
        shape = lambda net: None if net is None else [net.n_out, net.n_hidden, net.hidden]
        count = lambda plan, g: None if plan is None else [plan.n, int(g)]
        f = self.plan_f
        return dict(
            self._option_header(0), flavour=self.flavour, net=shape(self.net), net_e=shape(self.net_e),
            points_colloc=count(f, self.n_f_global), points_boundary=count(self.plan_b, self.n_b_global),
            points_supervised=[0 if self.plan_s is None else self.plan_s.n, int(self.n_s_global)],
            points_pool=None if self._pool is None else self._pool.n,
            points_colloc_passes=None if f is None else [[int(a), int(b)] for (a, b), _ in _passes(f)],
            colloc_weights=f is not None and self._static_w() is not None,
            lbfgs_history=None if self._lbfgs is None else self._lbfgs.history_size, rwf=self._rwf is not None,
            hard_bc=None if self.hard_boundary_info() is None else
            {k: list(x) if isinstance(x, tuple) else x for k, x in self.hard_boundary_info().items()},
            world_size=self.world_size, rank=self._rank(), first_layer="sine" if self.net.first_layer else None)

    def _state_info(self):
        """What a file records beside the structure; load_training_state reports the keys that differ."""
        kernels = getattr(self.plan_f, "kernel_names", None)
        return dict(
            self._option_header(1), precision=[list(getattr(net, "precision", ())) for _, net in self._nets()],
            kernels=None if kernels is None else list(kernels()), Re=self.Re, alpha_b=self.alpha_b, alpha_e=self.alpha_e,
            alpha_s=self.alpha_s, alpha_evm=self.alpha_evm, scale=self.scale, vis_t0=self.vis_t0, eq4_weight=self._w4())

    def _state_host(self):
        """The host mirrors of the device state."""
        ls = self._lbfgs_state
        return dict(self._option_header(2), adam_t=[net.adam_t for _, net in self._nets()],
                    e_trainable=bool(self.e_trainable), resample_calls=self._resample_calls,
                    lbfgs=None if self._lbfgs is None else [ls.n_iter, ls.func_evals, ls.t, ls.prev_loss])

    def _state_path(self, path):
        return path if self.world_size == 1 else path + ".rank%d" % self._rank()

    def _state_join(self):
        """Wait for the snapshot in flight, if any; an error of its writer is raised here."""
        sn = self._snap
        if sn is None or sn.thread is None:
            return
        sn.thread.join()
        sn.thread = None
        err, sn.error = sn.error, None
        if err is not None:
            raise err

    def __del__(self):
        try:
            self._state_join()
        except Exception:
            pass

    def save_training_state(self, path, extra=None, wait=True):
        """Write everything a later step reads that an earlier step wrote (_state_segments, and the host mirrors) to
        `path` (several ranks: path + '.rank%d', every rank its own file, no collective), so that a fresh process that
        builds the same engine, attaches the same data and options and calls load_training_state continues bit for bit.
        One launch (per 64 segments) on the current stream packs the state into a staging buffer that is allocated
        once; a side stream then copies it to pinned host memory, so the stream the steps run on waits for the pack
        alone.  wait=False: a host thread waits for that copy, writes path + '.tmp' and renames it over path - a job
        killed meanwhile leaves the previous file whole - and the call returns at once; the file then holds the state
        of the moment of the call, whatever steps follow.  At most one snapshot is in flight: the next call, wait=True
        and the engine's teardown join it.  extra: a JSON-able dict kept in the header (the solvers' loop position)."""
        self._state_join()
        segs = self._state_segments()
        cuda = self.device.type == "cuda"
        sn = self._snap = self._snap or _Snapshot()
        sig = [(name, t.numel() * t.element_size(), stored) for name, t, stored in segs]
        if sig != sn.sig:
            offs, sn.total = _state_file.layout([b if stored else 0 for _, b, stored in sig])
            sn.offsets = [o if stored else -1 for o, (_, _, stored) in zip(offs, sig)]
            sn.staging = torch.zeros(max(sn.total, 256), dtype=torch.uint8, device=self.device)
            sn.digests = torch.zeros(len(segs), 2, dtype=torch.int64, device=self.device)
            sn.host = torch.zeros(max(sn.total, 256), dtype=torch.uint8, pin_memory=cuda)
            sn.digests_host = torch.zeros(len(segs), 2, dtype=torch.int64, pin_memory=cuda)
            sn.scratch = sn.scratch if sn.scratch is not None else state_scratch(self.device)
            sn.sig = sig
        header = dict(fingerprint=self._state_fingerprint(), info=self._state_info(), host=self._state_host(),
                      extra={} if extra is None else extra,
                      segments=[dict(name=name, dtype=str(t.dtype).replace("torch.", ""), shape=list(t.shape), bytes=b,
                                     offset=o) for (name, t, _), (_, b, _), o in zip(segs, sig, sn.offsets)])
        path = self._state_path(path)
        t0 = time.perf_counter()
        if cuda:
            if sn.stream is None:
                sn.stream = torch.cuda.Stream(device=self.device)
                sn.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] + [torch.cuda.Event()]
            main = torch.cuda.current_stream(self.device)
            sn.ev[0].record(main)
            state_pack([t for _, t, _ in segs], sn.offsets, sn.staging, sn.digests, sn.scratch)
            sn.ev[1].record(main)
            with torch.cuda.stream(sn.stream):
                sn.stream.wait_event(sn.ev[1])
                sn.host.copy_(sn.staging, non_blocking=True)
                sn.digests_host.copy_(sn.digests, non_blocking=True)
                sn.ev[2].record(sn.stream)
        else:
            state_pack([t for _, t, _ in segs], sn.offsets, sn.staging, sn.digests, sn.scratch)
            sn.host.copy_(sn.staging)
            sn.digests_host.copy_(sn.digests)

        def finish():
            if cuda:
                sn.ev[2].synchronize()
            dig = sn.digests_host.numpy().view(np.uint64)
            for seg, d in zip(header["segments"], dig):
                seg["digest"] = [int(d[0]), int(d[1])]
            _state_file.write(path, header, sn.host.numpy()[:sn.total])
            sn.info = dict(path=path, bytes=sn.total, segments=[name for name, _, _ in segs],
                           stream_ms=sn.ev[0].elapsed_time(sn.ev[1]) if cuda else None,
                           wall_s=time.perf_counter() - t0)

        if wait:
            finish()
            return

        def run():
            try:
                finish()
            except BaseException as e:      # raised by the call that joins
                sn.error = e

        sn.thread = threading.Thread(target=run, name="nsfnet-state-writer")
        sn.thread.start()

    def training_state_info(self):
        """dict(path, bytes, segments, stream_ms, wall_s) of the last finished snapshot (stream_ms: the pack, between two
        events on the stream of the steps; wall_s: from the call to the renamed file); None before the first.  Joins
        the snapshot in flight."""
        self._state_join()
        return None if self._snap is None else self._snap.info

    def load_training_state(self, path, strict=True):
        """Continue from a file of save_training_state.  The engine must be built as the saving one was, with the same
        point sets and options attached (the file's fingerprint: a difference raises ValueError naming the first key that
        differs - another world size, rank or point count, an option on here and off there).  Every stored segment is
        verified against its digest on the host before anything is uploaded: a short or damaged file raises
        StateFileError and the engine is untouched.  strict: the boundary, supervised, validation and pool sets, which
        are not stored, must digest to what the file recorded (ValueError); strict=False skips only that.  Then one
        host-to-device copy and an unpack IN PLACE into the existing tensors - captured hipGraphs stay valid -, `prep`
        of every net rebuilt (compose under the weight factorization, then prepare), the host mirrors restored and the
        digests the unpack wrote compared with the header's.  An L-BFGS history in the file is adopted by the next
        lbfgs_step, whatever `owner` it is given.  loss_terms() and the field planes are not state: after a load they
        are those of the NEXT evaluation.  (With the factorization on, `params` comes back as compose(theta), which is
        what every update leaves; only a file saved before the first update could differ from the saving engine in
        the rounding of that product.)  Returns dict(extra=the caller's dict, changed=[info keys that differ])."""
        self._state_join()
        header, payload = _state_file.read(self._state_path(path))
        fp_file, fp = header["fingerprint"], self._state_fingerprint()
        adopt = fp_file.get("lbfgs_history") if self._lbfgs is None else None
        if adopt is not None:
            fp["lbfgs_history"] = adopt                 # the workspace is made below, once nothing can refuse any more
        if fp_file.get("lbfgs_history") is None:
            fp["lbfgs_history"] = None                  # nothing to restore: the engine's own history restarts
        fp, fp_file = json.loads(json.dumps(fp)), dict(fp_file)
        for key in sorted(set(fp) | set(fp_file)):
            if fp.get(key) != fp_file.get(key):
                raise ValueError("training state %s: fingerprint key %r differs: the file has %r, this engine %r"
                                 % (path, key, fp_file.get(key), fp.get(key)))
        made = None
        if adopt is not None:
            made = LbfgsHistory(self.net.num_train, int(adopt), self.device)
        segs = self._state_segments(lbfgs=made)
        if fp_file.get("lbfgs_history") is None:
            segs = [s for s in segs if not s[0].startswith("lbfgs.")]
        mine = [(name, t.numel() * t.element_size(), stored) for name, t, stored in segs]
        theirs = [(s["name"], s["bytes"], s["offset"] >= 0) for s in header["segments"]]
        if mine != theirs:
            bad = next((a, b) for a, b in zip(mine + [None], theirs + [None]) if a != b)
            raise ValueError("training state %s: the segments differ: this engine has %r, the file %r" % ((path,) + bad))
        sn = self._snap = self._snap or _Snapshot()
        if sn.scratch is None:
            sn.scratch = state_scratch(self.device)
        digests = torch.zeros(len(segs), 2, dtype=torch.int64, device=self.device)
        want = [[int(v) for v in s["digest"]] for s in header["segments"]]
        got = lambda: [[int(v) for v in row] for row in digests.cpu().numpy().view(np.uint64)]
        loose = [k for k, (_, _, stored) in enumerate(segs) if not stored]
        if strict and loose:                            # before anything is written
            state_pack([segs[k][1] for k in loose], [-1] * len(loose), None, digests[:len(loose)], sn.scratch)
            for k, d in zip(loose, got()):
                if d != want[k]:
                    raise ValueError("training state %s: %r is not what the saving run had attached (digest %s, the file "
                                     "has %s)" % (path, segs[k][0], d, want[k]))
        staging = torch.from_numpy(payload).to(self.device) if payload.size else None
        offsets = [s["offset"] for s in header["segments"]]
        if made is not None:
            self._lbfgs = made
        state_unpack(staging, offsets, [t for _, t, _ in segs], digests, sn.scratch)
        for _, net in self._nets():
            net.update_params()
        host = header["host"]
        for (_, net), t in zip(self._nets(), host["adam_t"]):
            net.adam_t = int(t)
        self.e_trainable, self._resample_calls = bool(host["e_trainable"]), int(host["resample_calls"])
        for option in self._options():
            option.restore_host(host)
        self.lbfgs_reset()
        if host["lbfgs"] is not None:
            ls = self._lbfgs_state
            ls.n_iter, ls.func_evals, ls.t, ls.prev_loss = host["lbfgs"]
            self._lbfgs_owner = _RESTORED
        self._eval_batch = False
        for k, d in enumerate(got()):
            if (strict or segs[k][2]) and d != want[k]:
                raise StateFileError("training state %s: segment %r arrived with digest %s, the file has %s"
                                     % (path, segs[k][0], d, want[k]))
        info = json.loads(json.dumps(self._state_info()))
        changed = sorted(k for k in set(info) | set(header["info"]) if info.get(k) != header["info"].get(k))
        return dict(extra=header["extra"], changed=changed)

    # ---- inference (evaluate / test / predict) ----
    def predict(self, x, y, with_e=False):
        plan = ValuePlan(self.net, x, y, with_backward=False)
        plan.forward(save=False)
        out = [plan.pred[0], plan.pred[1], plan.pred[2]]
        if with_e and self.net_e is not None:
            pe = ValuePlan(self.net_e, x, y, with_backward=False)
            pe.forward(save=False)
            out.append(pe.pred[0])
        return out
