"""fp64 numpy model of the conflict-free combination of the per-term gradients (ConFIG): the
Gram block partials and their sum in the kernels' order, the coefficients with the kernel's guards, the combine, and an
independent statement of the paper's definition through the pseudo-inverse.  Shared by the CPU tests (through
confgrad_fakes) and the GPU tests (kernel checks)."""
import math

import numpy as np

import fold_model as fm

BLK = 64
THREADS = 256
RECORD = 13
DET_MIN = 1e-10
PAIRS = ((0, 1), (0, 2), (1, 2))          # the terms of the cross entries rb, rs, bs


def block_partials(vecs, n):
    """[nblk, 6] partials rr, bb, ss, rb, rs, bs of three vectors (None = zeros) per 64-entry block: exact fp64
    products of the fp32 entries, summed in the kernel's order (wave_fold)."""
    nblk = (n + BLK - 1) // BLK
    v = np.zeros((3, nblk * BLK))
    for t, a in enumerate(vecs):
        if a is not None:
            v[t, :n] = np.asarray(a, dtype=np.float64).reshape(-1)[:n]
    v = v.reshape(3, nblk, BLK)
    cols = [(0, 0), (1, 1), (2, 2)] + list(PAIRS)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([fm.wave_fold(v[i] * v[j]) for i, j in cols], axis=1)


def sum_partials(partials):
    """The six sums in the coefficient kernel's order (strided_tree_fold)."""
    return fm.strided_tree_fold(partials, [fm.SUM] * 6, THREADS)


def coefficients(sums, nterms, rec=None):
    """One coefficient step from the six Gram sums; returns the new record (rec is not modified; None = zeros).
    [0..2] n_t  [3..5] cosines  [6..8] k_t  [9] |g|  [10] steps  [11] fallbacks  [12] dropped terms."""
    rec = np.zeros(RECORD) if rec is None else np.array(rec, dtype=np.float64)
    A, X = np.array(sums[:3], dtype=np.float64), np.array(sums[3:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = np.sqrt(A)
        sumsq = ((A[0] + A[1]) + A[2]) + 2.0 * ((X[0] + X[1]) + X[2])
        cs, k = np.zeros(3), np.ones(3)
        fallback, dropped = 0, 0
        if not (np.isfinite(A).all() and np.isfinite(X).all()):
            fallback, length = 1, np.sqrt(sumsq)
        else:
            on = [t < nterms and A[t] > 0.0 for t in range(3)]
            dropped = sum(1 for t in range(nterms) if not on[t])
            for q, (i, j) in enumerate(PAIRS):
                if on[i] and on[j]:
                    cs[q] = X[q] / (n[i] * n[j])
            if not any(on):
                k, length = np.zeros(3), 0.0
            else:
                a, b, c = cs
                det = ((1.0 + 2.0 * a * b * c) - a * a) - b * b - c * c
                c01, c02, c12 = b * c - a, a * c - b, a * b - c
                x = np.array([((1.0 - c * c) + c01) + c02, (c01 + (1.0 - b * b)) + c12, (c02 + c12) + (1.0 - a * a)])
                x = np.array([x[t] / det if on[t] else 0.0 for t in range(3)])
                sc = (x[0] + x[1]) + x[2]
                sn = 0.0
                for t in range(3):
                    if on[t]:
                        sn += n[t]
                if not (det > DET_MIN and np.isfinite(x).all() and sc > 0.0):
                    fallback, length = 1, math.sqrt(max(sumsq, 0.0))
                else:
                    scale = sn / sc
                    k = np.array([scale * x[t] / n[t] if on[t] else 0.0 for t in range(3)])
                    length = sn / math.sqrt(sc)
    rec[0:3], rec[3:6], rec[6:9], rec[9] = n, cs, k, length
    rec[10] += 1
    rec[11] += fallback
    rec[12] += dropped
    return rec


def combine(gr, gb, gs, k):
    """g = k_r g_r + k_b g_b (+ k_s g_s) in fp64."""
    g = float(k[0]) * np.asarray(gr, dtype=np.float64) + float(k[1]) * np.asarray(gb, dtype=np.float64)
    if gs is not None:
        g = g + float(k[2]) * np.asarray(gs, dtype=np.float64)
    return g


def step(vecs, rec=None):
    """The whole rule on term vectors [g_r, g_b, g_s or None]: (combined fp64 gradient with the coefficients rounded
    to fp32 as the device stores them, new record)."""
    n = np.asarray(vecs[0]).size
    rec = coefficients(sum_partials(block_partials(vecs, n)), 2 if vecs[2] is None else 3, rec)
    return combine(vecs[0], vecs[1], vecs[2], rec[6:9].astype(np.float32)), rec


def config_pinv(vecs):
    """The paper's definition, independent of the closed form: g_u = U(pinv([g_1^ .. g_m^]^T) 1),
    g = (sum_i g_i . g_u) g_u, with U(v) = v / |v| and g_t^ = U(g_t)."""
    G = np.stack([np.asarray(v, dtype=np.float64) for v in vecs if v is not None])
    units = G / np.linalg.norm(G, axis=1, keepdims=True)
    gu = np.linalg.pinv(units) @ np.ones(G.shape[0])
    gu = gu / np.linalg.norm(gu)
    return (G @ gu).sum() * gu
