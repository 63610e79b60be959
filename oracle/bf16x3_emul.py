"""What bf16x3 and plain-bf16 arithmetic give for the residual and the value term, in numpy (TEST INFRASTRUCTURE).

An emulation of the bf16 kernels' number formats that follows fwdmode_ref.forward4 / backward4 (residual_loss_and_grad)
and forward1 / backward1 / bc_loss_and_grad (value_loss_and_grad) step by step; it is NOT the kernels' summation order,
tiling or instruction selection.  It exists to tell "the kernel computes what its number format gives" from "the kernel
is wrong" where a bar is at stake: its error against the fp64 oracle is the format's own.  As in
nsfnet_amd/csrc/bf16_util.h, wave8_bodies.h and split_phases.h:
  * every hidden-to-hidden GEMM operand (a-streams and weights forward, z-adjoints and weights in reverse, z-adjoints
    and a-streams in dW) is split x = hi + lo, both bf16 rounded to nearest even; a bf16x3 product keeps
    hi*hi + hi*lo + lo*hi, a plain-bf16 product hi*hi alone, and both accumulate in fp32;
  * layer 0, the output layer, the last hidden layer's a-adjoints, the bias gradients and all chain-rule arithmetic
    are fp32;
  * the saved (t, z_x, z_y, z_D) of layers >= 1 and every z-adjoint that dW reads go through the 24-bit spill (sign,
    exponent, 15 mantissa bits, round half up in magnitude); layer 0 is recomputed, not spilled.

The keyword options restate what a plan may choose differently (defaults: the all-bf16x3 plan on the 24-bit spill):
  prec   (fwd, bwd, dw), each "fp32" | "bf16x3" | "bf16": the product of the forward hidden GEMMs, of the reverse
         a-adjoint GEMMs and of the dW GEMMs - the three roles pinn_net_set_precision takes.  "fp32" is a plain fp32
         matmul.  One name stands for all three roles.
  spill  "p24" | "f32": whether the saved quads and dW's z-adjoints pass through round24 (csrc/spill.h: SPILL_P24_* of
         the role-split sweeps and of the wide all-bf16 plans) or stay fp32 planes (SPILL_CLASSIC / SPILL_SKIP0: the
         narrow 8-wave family, the pipelined sweeps, every plan with an fp32 member, every value plan).
  acc    "fp32" | "fp64" | "k16": how the emulated products are summed - numpy's fp32 order, fp64 (rounded to fp32
         once), or fp32 over k in blocks of 16 (one MFMA's depth) added one after the other.  The three are equally
         legitimate; their spread is the summation-order noise of the format.
  spill0 "none" | "dw" | "all": who reads layer 0's saved quad through a "p24" spill.  The role-split sweeps at hidden
         256 and dw_bf16 behind them recompute it from the point ("none", SPILL_P24_COMPACT); in SPILL_P24_WIDE the
         forward sweep spills it: behind the wide role-split sweeps only dw_bf16_wide reads it back ("dw"), behind
         the wide 8-wave sweeps bwd_bf16_wide does too ("all").
  out    "fp32" | "image": the output layer's input.  The pipelined and role-split sweeps multiply the fp32 a-streams
         ("fp32"); the 8-wave sweeps fwd_bf16 / fwd_bf16_wide read them back from the LDS image of MFMA operands
         ("image": hi + lo in bf16x3, hi alone in plain bf16 - the output layer's weights stay fp32 either way).
  layer0 "plain" | "fma": layer 0's pre-activation as x * w0x + (y * w0y + b0) with every product rounded, or as the
         kernels' fmaf(w0x, x, fmaf(w0y, y, b0)) (spill_io.h layer0_z: one rounding per fmaf).
  tanh   "libm" | "fast": tanh rounded from fp64, or 1 - 2 / (exp2(z * 2.88539...) + 1) in fp32 as fast_tanh of
         bf16_util.h states it (the bf16 kernels' forward; the fp32 kernels call tanhf).
  point_map  None, or a pair of callables (forward, transpose) applied in fp32 after the output layer and before the
         reverse sweep: forward takes the net's output streams (N, 3, 4) - value mode: the predictions (N, n_out) - to
         the fields the loss is taken of, transpose takes the adjoints of those fields back to the net's outputs.  What
         the constrained point stages of csrc/point_stage.h do (the hard wall conditions); the caller states the map.
  fault  None, or a deliberate error for the sensitivity controls of tests/test_bf16_fast_mode.py: "trunc" truncates
         GEMM operands to bf16 instead of rounding them; ("stream", s, f) scales a-stream s of every hidden layer's
         forward GEMM input by f.
"""
import numpy as np

from . import fwdmode_ref as fr

F = np.float32
PRECS = ("fp32", "bf16x3", "bf16")


def bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return r.view(F)


def bf16_trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (a fault, not a format of the kernels)."""
    return (np.ascontiguousarray(x, dtype=F).view(np.uint32) & np.uint32(0xFFFF0000)).view(F)


def split(x, rnd=bf16):
    hi = rnd(x)
    return hi, rnd(np.asarray(x, F) - hi)


def round24(x):
    """The 24-bit spill: add 0x80 to the integer image, drop the low byte (spill_io.h pack24)."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    return ((u + np.uint32(0x80)) & np.uint32(0xFFFFFF00)).view(F)


def mm3(a, b):
    """a @ b on bf16x3: three bf16 products, fp32 accumulation."""
    ah, al = split(a)
    bh, bl = split(b)
    return (ah @ bh + (ah @ bl + al @ bh)).astype(F)


def _dot(a, b, acc):
    """a @ b of fp32 arrays, summed as `acc` says, as fp32."""
    if acc == "fp32":
        return (a @ b).astype(F)
    if acc == "fp64":
        return (a.astype(np.float64) @ b.astype(np.float64)).astype(F)
    assert acc == "k16", acc
    out = np.zeros((a.shape[0], b.shape[1]), F)
    for k in range(0, a.shape[1], 16):
        out = out + (a[:, k:k + 16] @ b[k:k + 16]).astype(F)
    return out


def mm(a, b, prec="bf16x3", acc="fp32", rnd=bf16):
    """a @ b in one of PRECS.  mm(a, b) is mm3(a, b)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if prec == "fp32":
        return _dot(a, b, acc)
    if prec == "bf16":
        return _dot(rnd(a), rnd(b), acc)
    assert prec == "bf16x3", prec
    if acc == "fp32" and rnd is bf16:
        return mm3(a, b)
    ah, al = split(a, rnd)
    bh, bl = split(b, rnd)
    if acc == "fp64":
        d = lambda p, q: p.astype(np.float64) @ q.astype(np.float64)
        return (d(ah, bh) + (d(ah, bl) + d(al, bh))).astype(F)
    return (_dot(ah, bh, acc) + (_dot(ah, bl, acc) + _dot(al, bh, acc))).astype(F)


def fast_tanh(z):
    """fast_tanh of bf16_util.h on fp32 (numpy's exp2 and divide for the device's 1-ulp v_exp_f32 and v_rcp_f32)."""
    with np.errstate(over="ignore"):
        e = np.exp2(np.asarray(z, F) * F(2.8853900817779268)).astype(F)
        return (F(1) - F(2) * (F(1) / (e + F(1)))).astype(F)


def _tanh(z, how):
    if how == "fast":
        return fast_tanh(z)
    assert how == "libm", how
    return np.tanh(z.astype(np.float64)).astype(F)


def _options(prec, spill, acc, tanh, fault, spill0="none", out="fp32"):
    prec = (prec,) * 3 if isinstance(prec, str) else tuple(prec)
    assert len(prec) == 3 and all(p in PRECS for p in prec), prec
    assert spill in ("p24", "f32") and acc in ("fp32", "fp64", "k16") and tanh in ("libm", "fast"), (spill, acc, tanh)
    assert spill0 in ("none", "dw", "all") and out in ("fp32", "image"), (spill0, out)
    assert fault is None or fault == "trunc" or (len(fault) == 3 and fault[0] == "stream"), fault
    rnd = bf16_trunc if fault == "trunc" else bf16
    gemm = lambda role: (lambda a, b: mm(a, b, prec[role], acc, rnd))
    scale = None if fault is None or fault == "trunc" else (int(fault[1]), F(fault[2]))
    return gemm(0), gemm(1), gemm(2), (round24 if spill == "p24" else (lambda q: q)), scale, _image(prec[0], out, rnd)


def _image(prec_fwd, out, rnd):
    """What the output layer reads of an a-stream: the stream, or its image as an operand of the forward GEMMs."""
    if out == "fp32" or prec_fwd == "fp32":
        return lambda q: q
    if prec_fwd == "bf16":
        return rnd
    return lambda q: (lambda hi, lo: hi + lo)(*split(q, rnd))


def _layer0(x, y, W0, b0, how):
    if how == "plain":
        return np.outer(x, W0[:, 0]) + (np.outer(y, W0[:, 1]) + b0)
    assert how == "fma", how
    d = np.float64      # (an fp32 product is exact in fp64; the sum's second rounding is below 2^-29 of an fp32 ulp)
    inner = (np.outer(y.astype(d), W0[:, 1].astype(d)) + b0.astype(d)).astype(F)
    return (np.outer(x.astype(d), W0[:, 0].astype(d)) + inner.astype(d)).astype(F)


def _a_streams(t, zx, zy, zd):
    d1 = F(1) - t * t
    d2 = F(-2) * t * d1
    return t, d1 * zx, d1 * zy, d2 * (zx * zx + zy * zy) + d1 * zd


def residual_loss_and_grad(flat, x, y, Re, n_hidden, hidden, coef=None, prec="bf16x3", spill="p24", acc="fp32",
                           tanh="libm", fault=None, spill0="none", out="fp32", layer0="plain", point_map=None):
    """The plain-flavour residual term (unit weights, scale 1) at float32 inputs: eqs, sums and the parameter gradient
    of sum_k coef * sum eq_k^2 / 2 (coef defaults to 2 / N, the engine's alpha_e = 1).  Options: see the module."""
    mm_f, mm_b, mm_d, sp, scale, img = _options(prec, spill, acc, tanh, fault, spill0, out)
    P = [(W.astype(F), b.astype(F)) for W, b in fr.unflatten(np.asarray(flat, F), 2, 3, n_hidden, hidden)]
    x, y = np.asarray(x, F).reshape(-1), np.asarray(y, F).reshape(-1)
    n, L = x.size, n_hidden
    c = F(2.0 / n if coef is None else coef)
    W0, b0 = P[0]
    z = _layer0(x, y, W0, b0, layer0)
    zx = np.broadcast_to(W0[:, 0], z.shape).copy()
    zy = np.broadcast_to(W0[:, 1], z.shape).copy()
    zd = np.zeros_like(z)
    saved = []
    for l in range(L):
        t = _tanh(z, tanh)
        s = (t, zx, zy, zd)
        saved.append(tuple(sp(q) for q in s) if l > 0 or spill0 == "all" else s)
        if l == 0:
            saved0_dw = saved[0] if spill0 == "none" else tuple(sp(q) for q in s)
        a = _a_streams(*s)
        W, b = P[l + 1]
        if l < L - 1:
            if scale is not None:
                a = tuple(q * scale[1] if k == scale[0] else q for k, q in enumerate(a))
            z, zx, zy, zd = mm_f(a[0], W.T) + b, mm_f(a[1], W.T), mm_f(a[2], W.T), mm_f(a[3], W.T)
        else:
            z, zx, zy, zd = img(a[0]) @ W.T + b, img(a[1]) @ W.T, img(a[2]) @ W.T, img(a[3]) @ W.T
    out = np.stack([z, zx, zy, zd], axis=2).astype(F)
    if point_map is not None:
        out = np.asarray(point_map[0](out), F)
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
    if point_map is not None:
        adj = np.asarray(point_map[1](adj), F)
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
            ap = _a_streams(*(saved[l - 1] if l > 1 else saved0_dw))
            zs = [sp(q) for q in zb]
            grads[l] = (sum(mm_d(zs[s].T, ap[s]) for s in range(4)).astype(F), zb[0].sum(axis=0))
            g = [mm_b(zb[s], P[l][0]) for s in range(4)]
    return dict(eqs=[q.astype(np.float64) for q in eqs], sums=[float(np.sum(q.astype(np.float64) ** 2)) for q in eqs],
                grad=fr.flatten(grads).astype(np.float64))


def value_loss_and_grad(flat, x_b, y_b, u_b, v_b, n_hidden, hidden, coef=None, n_out=3, prec="bf16", acc="fp32",
                        tanh="libm", fault=None, out="image", layer0="plain", point_map=None):
    """The value-mode (one-stream) boundary term at float32 inputs, after fwdmode_ref.forward1 / backward1 /
    bc_loss_and_grad: predictions (N, n_out), the two sums of squared errors and the parameter gradient of
    coef * (sum (u - u_b)^2 + sum (v - v_b)^2) / 2 (coef defaults to 2 / N).  As in the value branches of fwd_bf16.hip /
    bwd_bf16.hip (and their _wide twins) and in dw_bf16.hip:
      * the hidden-to-hidden GEMMs take bf16 operands in the role's precision - activations and weights forward,
        z-adjoints and weights in reverse, z-adjoints and activations in dW - and accumulate in fp32;
      * the output layer reads the last activations from the LDS image of MFMA operands (out="image": every value plan
        runs the 8-wave sweeps), with fp32 weights;
      * layer 0 (two FMAs of the point), the output layer's arithmetic, the last hidden layer's a-adjoints (a rank-3
        update), the gradients of layer 0 and of the output layer, the bias gradients and z-bar = (1 - t^2) * g are
        fp32;
      * every value plan is SPILL_CLASSIC: the saved t and the z-adjoints dW reads are fp32 planes, never rounded."""
    mm_f, mm_b, mm_d, _, scale, img = _options(prec, "f32", acc, tanh, fault, "none", out)
    P = [(W.astype(F), b.astype(F)) for W, b in fr.unflatten(np.asarray(flat, F), 2, n_out, n_hidden, hidden)]
    x, y = np.asarray(x_b, F).reshape(-1), np.asarray(y_b, F).reshape(-1)
    n, L = x.size, n_hidden
    c = F(2.0 / n if coef is None else coef)
    W0, b0 = P[0]
    z = _layer0(x, y, W0, b0, layer0)
    saved = []
    for l in range(L):
        t = _tanh(z, tanh)
        saved.append(t)
        W, b = P[l + 1]
        if l < L - 1:
            z = mm_f(t * scale[1] if scale is not None else t, W.T) + b
        else:
            pred = (img(t) @ W.T + b).astype(F)
    if point_map is not None:
        pred = np.asarray(point_map[0](pred), F)
    du, dv = pred[:, 0] - np.asarray(u_b, F).reshape(-1), pred[:, 1] - np.asarray(v_b, F).reshape(-1)
    adj = np.zeros_like(pred)
    adj[:, 0], adj[:, 1] = c * du, c * dv
    if point_map is not None:
        adj = np.asarray(point_map[1](adj), F)
    grads = [None] * (L + 1)
    grads[-1] = ((adj.T @ saved[-1]).astype(F), adj.sum(axis=0))
    g = adj @ P[-1][0]
    for l in range(L - 1, -1, -1):
        t = saved[l]
        zb = (F(1) - t * t) * g
        if l == 0:
            grads[0] = (np.stack([x @ zb, y @ zb], axis=1).astype(F), zb.sum(axis=0))
        else:
            grads[l] = (mm_d(zb.T, saved[l - 1]), zb.sum(axis=0))
            g = mm_b(zb, P[l][0])
    return dict(pred=pred.astype(np.float64), grad=fr.flatten(grads).astype(np.float64),
                sums=[float(np.sum(du.astype(np.float64) ** 2)), float(np.sum(dv.astype(np.float64) ** 2))])
