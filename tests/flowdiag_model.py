"""numpy statement of the flow diagnostics kernels of csrc/flowdiag.hip (TEST INFRASTRUCTURE),
operation for operation in fp64, so a record and a psi plane are meant to be compared bit for bit.  The three sums take
their order from tests/fold_model.py; the extrema need none (np.argmin / np.argmax return the lowest index on a tie,
which is the device's rule).  Node (i, j) of the nx x ny grid is point j nx + i; planes are [FLD_COUNT, >= n] fp32."""
import numpy as np

import fold_model as fm

RECORD, STATE = 32, 8
U, V, UX, UY, VX, VY = range(6)
ROW = ("t", "x_c", "y_c", "psi_min", "omega_c") + tuple(
    "%s_%s" % (k, q) for q in ("bl", "br", "tl", "tr") for k in ("x", "y", "psi_max", "area")) + (
    "counter_area", "mass_defect", "ke", "enstrophy", "div_rms", "div_max", "nonfinite")
S_RECORDS, S_CADENCE, S_NONFINITE = range(3)
THREADS, PER, MAX_BLOCKS = 256, 4, 512


def _wide(a):
    """fp64 of a plane: an fp32 plane widened as the kernels widen it; fp64 values (a reference field) as they are."""
    a = np.asarray(a)
    return a if a.dtype == np.float64 else a.astype(np.float32).astype(np.float64)


def blocks(n):
    return min(-(-n // (THREADS * PER)), MAX_BLOCKS)


def stream_function(u, ys, nx, ny):
    """psi [ny nx] fp64 of the plane u [>= ny nx]: sequential in j, (0.5 (u_j + u_j-1)) (ys_j - ys_j-1)."""
    u = _wide(u)[:nx * ny].reshape(ny, nx)
    ys = np.asarray(ys, np.float64)
    psi = np.zeros((ny, nx))
    with np.errstate(all="ignore"):
        for j in range(1, ny):
            psi[j] = psi[j - 1] + (0.5 * (u[j] + u[j - 1])) * (ys[j] - ys[j - 1])
    return psi.reshape(-1)


def _refine_axis(psi, at, stride, k, m, c):
    d = 0.0
    with np.errstate(all="ignore"):
        if 0 < k < m - 1:
            lo, b, hi = psi[at - stride], psi[at], psi[at + stride]
            den = (lo - 2.0 * b) + hi
            if den != 0.0:
                d = (0.5 * (lo - hi)) / den
                d = -0.5 if d < -0.5 else (0.5 if d > 0.5 else d)
        k2 = min(max(k + (1 if d > 0.0 else -1), 0), m - 1)
        return c[k] + abs(d) * (c[k2] - c[k])


def centre(psi, at, xs, ys):
    """The refined (x, y) of the extremum at point `at`."""
    nx, ny = len(xs), len(ys)
    j, i = divmod(int(at), nx)
    return _refine_axis(psi, at, 1, i, nx, xs), _refine_axis(psi, at, nx, j, ny, ys)


def quadrants(xs, ys):
    """[ny, nx] int: 0 BL, 1 BR, 2 TL, 3 TR, and -1 on the lid row."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    xm, ym = (xs[0] + xs[-1]) * 0.5, (ys[0] + ys[-1]) * 0.5
    q = (xs >= xm).astype(int)[None, :] + 2 * (ys >= ym).astype(int)[:, None]
    q[-1] = -1
    return q


def stats(fld, psi, xs, ys, eps, t, every, state, ring):
    """One pinn_flow_stats: writes its row into ring [capacity, RECORD] and updates state [STATE], both in place
    (t = -1: the cadence position from the state).  Returns the row."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    nx, ny = len(xs), len(ys)
    n = nx * ny
    f = [_wide(fld[c])[:n] for c in range(6)]
    psi = np.asarray(psi, np.float64)[:n]
    nb = blocks(n)
    with np.errstate(all="ignore"):
        w, dv = f[VX] - f[UY], f[UX] + f[VY]
        sums = [fm.grid_fold(v, nb) for v in (f[U] * f[U] + f[V] * f[V], w * w, dv * dv)]
        nonfinite = float(np.count_nonzero(~(np.isfinite(psi) & np.isfinite(w) & np.isfinite(dv))))
    k = int(state[S_RECORDS])
    if t < 0:
        t = (state[S_CADENCE] + 1.0) * every
        state[S_CADENCE] += 1.0
    state[S_RECORDS] = k + 1.0
    row = np.zeros(RECORD)
    row[0], row[27] = t, nonfinite
    if nonfinite > 0:
        state[S_NONFINITE] += 1.0
        row[1:27] = np.nan
        ring[k % ring.shape[0]] = row
        return row
    at = int(np.argmin(psi))
    row[1], row[2] = centre(psi, at, xs, ys)
    row[3], row[4] = psi[at], w[at]
    thr = eps * abs(psi[at])
    quad = quadrants(xs, ys).reshape(-1)
    total = 0.0
    for q in range(4):
        m = quad == q
        e = row[5 + 4 * q:9 + 4 * q]
        if m.any():
            at = int(np.argmax(np.where(m, psi, -np.inf)))
            e[0], e[1] = centre(psi, at, xs, ys)
            e[2] = psi[at]
        else:
            e[:3] = np.nan
        e[3] = float(np.count_nonzero(m & (psi > thr))) / float(n)
        total = total + e[3]
    row[21] = total
    row[22] = np.abs(psi[n - nx:]).max()
    row[23], row[24], row[25] = sums[0] / float(n), sums[1] / float(n), np.sqrt(sums[2] / float(n))
    row[26] = np.abs(dv).max()
    ring[k % ring.shape[0]] = row
    return row


def diagnose(fld, xs, ys, eps=1e-3, t=0.0, every=1, state=None, ring=None):
    """stream_function + stats on fresh state: (row as a dict, psi)."""
    state = np.zeros(STATE) if state is None else state
    ring = np.zeros((1, RECORD)) if ring is None else ring
    psi = stream_function(fld[U], ys, len(xs), len(ys))
    return dict(zip(ROW, stats(fld, psi, xs, ys, eps, t, every, state, ring))), psi


def history(state, ring):
    """The rows in time order, the ring unwrapped."""
    k, cap = int(state[S_RECORDS]), ring.shape[0]
    if k <= cap:
        return ring[:k].copy()
    return np.concatenate([ring[k % cap:], ring[:k % cap]])
