"""fp64 model of the frozen Fourier-feature first layer (TEST INFRASTRUCTURE).

Two independent statements of the net whose layer 0 is a = sin(W0 x + b0) and whose layers 1 .. L-1 are tanh:
  * SineFirstNet is a torch module over oracle.autograd_ref.RefFCNet's parameters whose first activation is torch.sin,
    so fields, residuals, loss and the parameter gradient come from autograd (step, through hardbc_model's statement of
    the engine's loss, which takes any module);
  * layer0_streams is the closed-form forward-mode map of layer 0 in numpy - the four streams (a, a_x, a_y, a_D) as
    include/nsfnet_pinn.h states them - and forward4 / backward4 / pde_loss_and_grad compose it with
    oracle.fwdmode_ref's sweep for the remaining layers (the same operations, layer by layer, as fwdmode_ref.forward4 /
    backward4 from layer 1 on), in passes where the point count asks for it.
Layer 0 is frozen: both statements return +0.0 for its 3 H gradient entries.
"""
import numpy as np
import torch

import hardbc_model as hm
from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr


def first_layer(B, dtype=np.float32):
    """(W0 [2m, 2], b0 [2m]) of the embedding with frequencies B [m, 2], rounded to `dtype` as the engine rounds them:
    rows 2k and 2k + 1 are 2 pi B_k, the biases pi / 2 (the cosine) and 0 (the sine)."""
    B = np.asarray(B, dtype=np.float64)
    w0 = np.repeat((2.0 * np.pi * B).astype(dtype), 2, axis=0)
    b0 = np.zeros(2 * B.shape[0], dtype=dtype)
    b0[0::2] = dtype(np.pi / 2.0)
    return w0, b0


def with_first_layer(flat, H, B):
    """A copy of the flat parameter vector (state_dict order) with layer 0 replaced by the embedding of B."""
    flat = np.array(flat, dtype=np.float32)
    w0, b0 = first_layer(B)
    flat[:2 * H] = w0.reshape(-1)
    flat[2 * H:3 * H] = b0
    return flat


# ---- statement 1: torch, autograd ----
class SineFirstNet(torch.nn.Module):
    """RefFCNet's Linear modules with torch.sin after layer_0 and tanh after the other hidden layers; parameters()
    are the wrapped net's, in its order."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, X):
        lin = [m for m in self.net.layers if isinstance(m, torch.nn.Linear)]
        a = torch.sin(lin[0](X))
        for m in lin[1:-1]:
            a = torch.tanh(m(a))
        return lin[-1](a)


def sine_net(flat, L, H, n_out=3, dtype=torch.float64):
    """SineFirstNet over a RefFCNet(2, n_out, L, H) of `dtype` holding the flat parameter vector."""
    net = ar.RefFCNet(2, n_out, L, H).to(dtype)
    torch.nn.utils.vector_to_parameters(torch.as_tensor(np.asarray(flat), dtype=dtype), net.parameters())
    return SineFirstNet(net)


def tanh_net(flat, L, H, n_out=1, dtype=torch.float64):
    """The plain RefFCNet (the entropy net keeps tanh)."""
    net = ar.RefFCNet(2, n_out, L, H).to(dtype)
    torch.nn.utils.vector_to_parameters(torch.as_tensor(np.asarray(flat), dtype=dtype), net.parameters())
    return net


def freeze(grad, H):
    """The gradient with layer 0's 3 H entries set to +0.0 (layer 0 is not trained)."""
    g = np.array(grad, dtype=np.float64)
    g[:3 * H] = 0.0
    return g


def step(model, H, x, y, Re, xb, yb, ub, vb, **kw):
    """hardbc_model.constrained_step on the sine net (it takes any module), with the frozen gradient."""
    r = hm.constrained_step(model, x, y, Re, xb, yb, ub, vb, **kw)
    r["grad"] = freeze(r["grad"], H)
    return r


# ---- statement 2: numpy, forward mode ----
def layer0_streams(W0, b0, x, y):
    """(a, a_x, a_y, a_D), each (N, H): z = w0x x + w0y y + b0, a = sin z, a_x = cos z w0x, a_y = cos z w0y,
    a_D = -sin z (w0x^2 + w0y^2)."""
    x = np.asarray(x).reshape(-1)
    y = np.asarray(y).reshape(-1)
    z = np.outer(x, W0[:, 0]) + np.outer(y, W0[:, 1]) + b0
    s, c = np.sin(z), np.cos(z)
    return s, c * W0[:, 0], c * W0[:, 1], -s * (W0[:, 0] ** 2 + W0[:, 1] ** 2)


def _tanh_streams(saved):
    t, zx, zy, zd = saved
    d1 = 1.0 - t * t
    d2 = -2.0 * t * d1
    return t, d1 * zx, d1 * zy, d2 * (zx * zx + zy * zy) + d1 * zd


def forward4(params, x, y):
    """fwdmode_ref.forward4 with layer 0 by layer0_streams: out (N, n_out, 4) and saved, whose entry 0 holds layer 0's
    a-streams themselves and whose entries l >= 1 hold (t, z_x, z_y, z_D) as before - what an FF plan saves."""
    a = layer0_streams(params[0][0], params[0][1], x, y)
    saved = [a]
    for l in range(1, len(params)):
        W, b = params[l]
        z = (a[0] @ W.T + b, a[1] @ W.T, a[2] @ W.T, a[3] @ W.T)
        if l == len(params) - 1:
            return np.stack(z, axis=2), saved
        saved.append((np.tanh(z[0]), z[1], z[2], z[3]))
        a = _tanh_streams(saved[-1])


def backward4(params, saved, out_adj):
    """fwdmode_ref.backward4 down to layer 1, whose weight gradient takes layer 0's a-streams as saved; layer 0's own
    gradient is +0.0.  Returns the flat parameter gradient."""
    n_lin = len(params)
    grads = [None] * n_lin
    grads[0] = (np.zeros_like(params[0][0]), np.zeros_like(params[0][1]))
    a = _tanh_streams(saved[-1])
    grads[-1] = (sum(out_adj[:, :, s].T @ a[s] for s in range(4)), out_adj[:, :, 0].sum(axis=0))
    g = [out_adj[:, :, s] @ params[-1][0] for s in range(4)]
    for l in range(n_lin - 2, 0, -1):
        t, zx, zy, zd = saved[l]
        d1 = 1.0 - t * t
        d2 = -2.0 * t * d1
        d3 = -2.0 * d1 * (1.0 - 3.0 * t * t)
        ga, gx, gy, gd = g
        zbs = (d1 * ga + d2 * (zx * gx + zy * gy) + (d3 * (zx * zx + zy * zy) + d2 * zd) * gd,
               d1 * gx + 2.0 * d2 * zx * gd, d1 * gy + 2.0 * d2 * zy * gd, d1 * gd)
        ap = saved[0] if l == 1 else _tanh_streams(saved[l - 1])
        grads[l] = (sum(zbs[s].T @ ap[s] for s in range(4)), zbs[0].sum(axis=0))
        g = [zbs[s] @ params[l][0] for s in range(4)]
    return fr.flatten(grads)


def pde_loss_and_grad(params, x, y, Re, alpha_e=1.0, scale=1.0, w=None, chunk=4096):
    """The plain flavour's collocation term by the forward-mode sweep, in passes of <= chunk points normalised by the
    global N: dict(out (N, 3, 4), eqs, sums, grad).  The output adjoints are fwdmode_ref.pde_loss_and_grad's."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N = x.size
    outs, eqs_all, sums, grad = [], [], np.zeros(3), None
    for lo in range(0, N, int(chunk)):
        hi = min(N, lo + int(chunk))
        out, saved = forward4(params, x[lo:hi], y[lo:hi])
        eqs = fr.residuals(out, Re, None, None, scale)
        ww = np.ones(hi - lo) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)[lo:hi]
        sums += [float(np.sum(ww * q * q)) for q in eqs]
        g = [2.0 * alpha_e * ww * q / N for q in eqs]
        s, s2 = scale, scale * scale
        u, v = out[:, 0, 0], out[:, 1, 0]
        u_x, u_y, v_x, v_y = out[:, 0, 1] * s, out[:, 0, 2] * s, out[:, 1, 1] * s, out[:, 1, 2] * s
        nu = 1.0 / Re
        adj = np.zeros_like(out)
        adj[:, 0, 0] = g[0] * u_x + g[1] * v_x
        adj[:, 1, 0] = g[0] * u_y + g[1] * v_y
        adj[:, 0, 1] = (g[0] * u + g[2]) * s
        adj[:, 0, 2] = (g[0] * v) * s
        adj[:, 1, 1] = (g[1] * u) * s
        adj[:, 1, 2] = (g[1] * v + g[2]) * s
        adj[:, 2, 1] = g[0] * s
        adj[:, 2, 2] = g[1] * s
        adj[:, 0, 3] = -nu * g[0] * s2
        adj[:, 1, 3] = -nu * g[1] * s2
        gr = backward4(params, saved, adj)
        grad = gr if grad is None else grad + gr
        outs.append(out)
        eqs_all.append(eqs)
    return dict(out=np.concatenate(outs), eqs=[np.concatenate([q[k] for q in eqs_all]) for k in range(3)],
                sums=[float(s) for s in sums], grad=grad)


def forward1(params, x, y):
    """Value mode: (pred (N, n_out), saved activations), layer 0 on sin."""
    X = np.stack([np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)], axis=1)
    a, saved = X, []
    for l, (W, b) in enumerate(params):
        z = a @ W.T + b
        if l == len(params) - 1:
            return z, saved
        a = np.sin(z) if l == 0 else np.tanh(z)
        saved.append(a)


def backward1(params, saved, out_adj):
    """Value mode's parameter gradient, layer 0 frozen."""
    n_lin = len(params)
    grads = [None] * n_lin
    grads[0] = (np.zeros_like(params[0][0]), np.zeros_like(params[0][1]))
    g = out_adj
    for l in range(n_lin - 1, 0, -1):
        if l < n_lin - 1:
            g = g * (1.0 - saved[l] * saved[l])
        grads[l] = (g.T @ saved[l - 1], g.sum(axis=0))
        g = g @ params[l][0]
    return fr.flatten(grads)


def bc_loss_and_grad(params, xb, yb, ub, vb, alpha_b=1.0):
    """fwdmode_ref.bc_loss_and_grad on the sine net."""
    out, saved = forward1(params, xb, yb)
    N = out.shape[0]
    du = out[:, 0] - np.asarray(ub, dtype=np.float64).reshape(-1)
    dv = out[:, 1] - np.asarray(vb, dtype=np.float64).reshape(-1)
    adj = np.zeros_like(out)
    adj[:, 0] = 2.0 * alpha_b * du / N
    adj[:, 1] = 2.0 * alpha_b * dv / N
    return dict(pred=out, sums=[float(np.sum(du * du)), float(np.sum(dv * dv))], grad=backward1(params, saved, adj))
