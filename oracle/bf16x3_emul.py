"""What bf16x3 arithmetic gives for the residual term, in numpy (TEST INFRASTRUCTURE).

An emulation of the bf16x3 residual kernels' number formats that follows fwdmode_ref.forward4 / backward4 step by
step; it is NOT the kernels' summation order, tiling or instruction selection.  It exists to tell "the kernel computes
what its number format gives" from "the kernel is wrong" where a bar is at stake: its error against the fp64 oracle is
the format's own.  As in nsfnet_amd/csrc/bf16_util.h and split_phases.h:
  * every hidden-to-hidden GEMM operand (a-streams and weights forward, z-adjoints and weights in reverse, z-adjoints
    and a-streams in dW) is split x = hi + lo, both bf16 rounded to nearest even; a product keeps
    hi*hi + hi*lo + lo*hi and accumulates in fp32;
  * layer 0, the output layer, the last hidden layer's a-adjoints, the bias gradients and all chain-rule arithmetic
    are fp32;
  * the saved (t, z_x, z_y, z_D) of layers >= 1 and every z-adjoint that dW reads go through the 24-bit spill (sign,
    exponent, 15 mantissa bits, round half up in magnitude); layer 0 is recomputed, not spilled.
"""
import numpy as np

from . import fwdmode_ref as fr

F = np.float32


def bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return r.view(F)


def split(x):
    hi = bf16(x)
    return hi, bf16(np.asarray(x, F) - hi)


def round24(x):
    """The 24-bit spill: add 0x80 to the integer image, drop the low byte (spill_io.h pack24)."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    return ((u + np.uint32(0x80)) & np.uint32(0xFFFFFF00)).view(F)


def mm3(a, b):
    """a @ b on bf16x3: three bf16 products, fp32 accumulation."""
    ah, al = split(a)
    bh, bl = split(b)
    return (ah @ bh + (ah @ bl + al @ bh)).astype(F)


def _a_streams(t, zx, zy, zd):
    d1 = F(1) - t * t
    d2 = F(-2) * t * d1
    return t, d1 * zx, d1 * zy, d2 * (zx * zx + zy * zy) + d1 * zd


def residual_loss_and_grad(flat, x, y, Re, n_hidden, hidden, coef=None):
    """The plain-flavour residual term (unit weights, scale 1) at float32 inputs: eqs, sums and the parameter gradient
    of sum_k coef * sum eq_k^2 / 2 (coef defaults to 2 / N, the engine's alpha_e = 1)."""
    P = [(W.astype(F), b.astype(F)) for W, b in fr.unflatten(np.asarray(flat, F), 2, 3, n_hidden, hidden)]
    x, y = np.asarray(x, F).reshape(-1), np.asarray(y, F).reshape(-1)
    n, L = x.size, n_hidden
    c = F(2.0 / n if coef is None else coef)
    W0, b0 = P[0]
    z = np.outer(x, W0[:, 0]) + (np.outer(y, W0[:, 1]) + b0)
    zx = np.broadcast_to(W0[:, 0], z.shape).copy()
    zy = np.broadcast_to(W0[:, 1], z.shape).copy()
    zd = np.zeros_like(z)
    saved = []
    for l in range(L):
        t = np.tanh(z.astype(np.float64)).astype(F)
        s = (t, zx, zy, zd)
        saved.append(s if l == 0 else tuple(round24(q) for q in s))
        a = _a_streams(*s)
        W, b = P[l + 1]
        if l < L - 1:
            z, zx, zy, zd = mm3(a[0], W.T) + b, mm3(a[1], W.T), mm3(a[2], W.T), mm3(a[3], W.T)
        else:
            z, zx, zy, zd = a[0] @ W.T + b, a[1] @ W.T, a[2] @ W.T, a[3] @ W.T
    out = np.stack([z, zx, zy, zd], axis=2).astype(F)
    nu = F(1.0 / Re)
    u, v = out[:, 0, 0], out[:, 1, 0]
    eq1 = (u * out[:, 0, 1] + v * out[:, 0, 2]) + out[:, 2, 1] - nu * out[:, 0, 3]
    eq2 = (u * out[:, 1, 1] + v * out[:, 1, 2]) + out[:, 2, 2] - nu * out[:, 1, 3]
    eq3 = out[:, 0, 1] + out[:, 1, 2]
    eqs = [eq1, eq2, eq3]
    r1, r2, r3 = c * eq1, c * eq2, c * eq3
    adj = np.zeros_like(out)
    adj[:, 0, 0] = r1 * out[:, 0, 1] + r2 * out[:, 1, 1]
    adj[:, 1, 0] = r1 * out[:, 0, 2] + r2 * out[:, 1, 2]
    adj[:, 0, 1], adj[:, 0, 2] = r1 * u + r3, r1 * v
    adj[:, 1, 1], adj[:, 1, 2] = r2 * u, r2 * v + r3
    adj[:, 2, 1], adj[:, 2, 2] = r1, r2
    adj[:, 0, 3], adj[:, 1, 3] = -nu * r1, -nu * r2
    # reverse
    grads = [None] * (L + 1)
    Wout = P[-1][0]
    a = _a_streams(*saved[-1])
    grads[-1] = (sum(adj[:, :, s].T @ a[s] for s in range(4)).astype(F), adj[:, :, 0].sum(axis=0))
    g = [adj[:, :, s] @ Wout for s in range(4)]
    for l in range(L - 1, -1, -1):
        t, zx, zy, zd = saved[l]
        d1 = F(1) - t * t
        d2 = F(-2) * t * d1
        d3 = F(-2) * d1 * (F(1) - F(3) * t * t)
        ga, gx, gy, gd = g
        zz = zx * zx + zy * zy
        zb = (d1 * ga + d2 * (zx * gx + zy * gy) + (d3 * zz + d2 * zd) * gd, d1 * gx + F(2) * d2 * zx * gd,
              d1 * gy + F(2) * d2 * zy * gd, d1 * gd)
        if l == 0:
            gW0 = np.stack([x @ zb[0] + zb[1].sum(axis=0), y @ zb[0] + zb[2].sum(axis=0)], axis=1)
            grads[0] = (gW0.astype(F), zb[0].sum(axis=0))
        else:
            ap = _a_streams(*saved[l - 1])
            zs = [round24(q) for q in zb]
            grads[l] = (sum(mm3(zs[s].T, ap[s]) for s in range(4)).astype(F), zb[0].sum(axis=0))
            g = [mm3(zb[s], P[l][0]) for s in range(4)]
    return dict(eqs=[q.astype(np.float64) for q in eqs], sums=[float(np.sum(q.astype(np.float64) ** 2)) for q in eqs],
                grad=fr.flatten(grads).astype(np.float64))
