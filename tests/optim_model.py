"""fp64 model of the device learning-rate schedule and gradient clipping of csrc/optim.hip / pinn_lr_schedule_value,
pinn_grad_sqnorm and pinn_adam_step_sched (TEST INFRASTRUCTURE; numpy and math only).  The definition
(include/nsfnet_pinn.h):

    lr_e   = closed form of the schedule kind at epoch e, times the linear warm-up factor      fp64
    sq     = sum of g_i^2 over all entries of all vectors                                      fp64 (g fp32)
    coef   = fp32(min(1, max_norm / (sqrt(sq) + 1e-6)))                                        NaN propagates
    update = Adam (oracle/fwdmode_ref.adam_step) with lr = fp32(lr_e) on the gradient fp32(g_i coef)

Python evaluates every fp64 operation here as one correctly rounded operation in the order written."""
import math

import numpy as np

from oracle import fwdmode_ref as fr

RECORD = 6           # PINN_OPTIM_RECORD
R_EPOCH, R_LR, R_NORM, R_COEF, R_CLIPPED, R_UPDATES = range(6)
KINDS = ("constant", "multistep", "step", "exponential", "cosine")


def lr_e(lr0, e, kind="constant", milestones=(), gamma=0.1, step_size=1, t_max=1, eta_min=0.0, warmup_epochs=0,
         warmup_start=0.0):
    lr0, e = float(lr0), int(e)
    if kind == "constant":
        lr = lr0
    elif kind == "multistep":
        lr = lr0 * math.pow(gamma, float(sum(1 for m in milestones if m <= e)))
    elif kind == "step":
        lr = lr0 * math.pow(gamma, float(e // step_size))
    elif kind == "exponential":
        lr = lr0 * math.pow(gamma, float(e))
    elif kind == "cosine":
        lr = eta_min + (lr0 - eta_min) * (1.0 + math.cos(math.pi * float(e) / float(t_max))) / 2.0
    else:
        raise ValueError(kind)
    if warmup_epochs > 0:
        lr = lr * (warmup_start + (1.0 - warmup_start) * (float(min(e, warmup_epochs)) / float(warmup_epochs)))
    return lr


def sqnorm(*vecs):
    """The fp64 sum of squares of the fp32 vectors (each square is exact in fp64)."""
    with np.errstate(all="ignore"):
        return float(sum(np.sum(np.asarray(v, dtype=np.float32).astype(np.float64) ** 2) for v in vecs if v is not None))


def clip(sq, max_norm):
    """(total norm fp64, coef fp32) of the squared norm sq: the clip_grad_norm_ formula."""
    with np.errstate(all="ignore"):
        norm = math.sqrt(sq) if sq >= 0.0 else float("nan")
        c = float(max_norm) / (norm + 1e-6)
        return norm, np.float32(1.0 if c > 1.0 else c)


def scaled(g, coef):
    """fp32(g coef): one rounded fp32 multiply per entry; coef None = the gradient as it is."""
    g = np.asarray(g, dtype=np.float32)
    with np.errstate(all="ignore"):
        return g if coef is None else g * np.float32(coef)


def update(p, g, m, v, t, lr, coef=None, b1=0.9, b2=0.999, eps=1e-8):
    """(p, m, v) in fp64 after Adam update number t with the fp32 rate lr on the scaled gradient."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    return fr.adam_step(f(p), f(scaled(g, coef)), f(m), f(v), t, float(np.float32(lr)), b1, b2, eps)
