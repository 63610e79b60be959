"""fp64 numpy model of the adaptive loss-weight balancing: the block statistics, the
update rule with its guards, the combine and the cadence.  Shared by the CPU tests (through balance_fakes) and the
GPU tests (kernel checks)."""
import math

import numpy as np

import fold_model as fm

BLK = 64
RECORD = 12


def block_partials(vecs, n):
    """[nblk, 6] partials of three vectors (None = zeros): per 64-entry block max|v_t| (NaN-propagating), sum|v_t|,
    both in the kernel's order (wave_fold)."""
    nblk = (n + BLK - 1) // BLK
    out = np.zeros((nblk, 6))
    for t, v in enumerate(vecs):
        if v is None:
            continue
        a = np.zeros(nblk * BLK)
        a[:n] = np.abs(np.asarray(v, dtype=np.float64).reshape(-1)[:n])
        a = a.reshape(nblk, BLK)
        out[:, 2 * t] = fm.wave_fold(a, fm.NANMAX)
        out[:, 2 * t + 1] = fm.wave_fold(a, fm.SUM)
    return out


def initial_record(alpha_b, alpha_s):
    rec = np.zeros(RECORD)
    rec[9], rec[10] = alpha_b, alpha_s
    return rec


def update(partials, n, terms, beta, rec):
    """One balance update from [nblk, 6] partials; returns the new record (rec is not modified)."""
    rec = np.array(rec, dtype=np.float64)
    f = fm.strided_tree_fold(partials, [fm.NANMAX, fm.SUM] * 3)      # the update kernel's order
    mx, sm = [float(f[2 * t]) for t in range(3)], [float(f[2 * t + 1]) for t in range(3)]
    rec[0], rec[1] = mx[0], sm[0] / n
    for t in (1, 2):
        base = 2 + 3 * (t - 1)
        mean = sm[t] / n
        rec[base], rec[base + 1] = mx[t], mean
        if not (terms >> (t - 1)) & 1:
            rec[base + 2] = 0.0
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            lhat = float(np.float64(mx[0]) / np.float64(mean))
        rec[base + 2] = lhat
        if mean == 0.0 or not math.isfinite(lhat):
            rec[8] += 1
            continue
        rec[8 + t] = (1.0 - beta) * rec[8 + t] + beta * lhat
    rec[11] += 1
    return rec


def combine(gr, gb, gs, lam):
    """g = g_r + lam_b g_b (+ lam_s g_s) in fp64."""
    g = np.asarray(gr, dtype=np.float64) + float(lam[0]) * np.asarray(gb, dtype=np.float64)
    if gs is not None:
        g = g + float(lam[1]) * np.asarray(gs, dtype=np.float64)
    return g


class Cadence:
    """Which evaluations apply the rule: the first one for Adam update n with n % every == 0."""

    def __init__(self, every):
        self.every, self.n, self.done = every, 0, -1

    def evaluate(self, frozen=False):
        if self.every <= 0 or frozen or self.n % self.every or self.done == self.n:
            return False
        self.done = self.n
        return True

    def adam(self):
        self.n += 1
