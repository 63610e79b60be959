"""numpy replay of the collocation-point selection of pinn_resample_select (TEST INFRASTRUCTURE).

The math of include/nsfnet_pinn.h, written out sequentially.  The prefix sum C runs in extended precision
(np.longdouble), so the replay's C_i M / T + U is closer to the exact value than either fp64 order; a device
result may then differ from it only where that value lies within a rounding error of an integer.
"""
import numpy as np


def residual_sq(eq, w4):
    """e2 = eq1^2 + eq2^2 + eq3^2 + w4 eq4^2 in fp64 from the fp32 planes, summed in that order."""
    e = [np.asarray(q, dtype=np.float32).astype(np.float64) for q in eq]
    s = e[0] * e[0] + e[1] * e[1]
    s = s + e[2] * e[2]
    if w4 != 0.0:
        s = s + float(w4) * (e[3] * e[3])
    return s


def density(eq, w4, k, c):
    """(b, S): b_i = a_i + c S / N with a_i = e2_i^(k/2) (a_i = 1 when S == 0), S = sum a_i; at k = 0 a non-finite
    e2_i gives a_i = NaN."""
    e2 = residual_sq(eq, w4)
    n = e2.size
    if k == 0:
        a = np.where(e2 <= np.finfo(np.float64).max, 1.0, np.nan)     # a non-finite residual still reaches S
    elif k == 1:
        a = np.sqrt(e2)
    elif k == 2:
        a = e2
    else:
        a = e2 ** (0.5 * k)
    S = float(np.sum(a.astype(np.longdouble)))
    if S == 0.0:
        a = np.ones(n)
        S_eff = float(n)
    else:
        S_eff = S
    return a + c * S_eff / n, S


def offsets(eq, w4, k, c, u, m):
    """(o, v, S): o_i = min(m, floor(v_i)), v_i = C_i m / T + u, o_{N-1} = m; pool point i fills out[o_{i-1} .. o_i)."""
    b, S = density(eq, w4, k, c)
    C = np.cumsum(b.astype(np.longdouble))
    T = C[-1]
    v = (C * m / T + np.longdouble(u)).astype(np.float64)
    o = np.minimum(m, np.floor(v)).astype(np.int64)
    o[-1] = m
    return o, v, S


def select(eq, w4, k, c, u, m):
    """(idx, S): the m selected pool indices (ascending, repeats allowed) and S."""
    o, _, S = offsets(eq, w4, k, c, u, m)
    counts = np.diff(np.concatenate([[0], o]))
    return np.repeat(np.arange(o.size, dtype=np.int64), counts), S


def offsets_of(idx, n):
    """o recovered from a selection: o_i = number of selected slots holding an index <= i."""
    return np.cumsum(np.bincount(np.asarray(idx, dtype=np.int64), minlength=n))
