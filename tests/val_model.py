"""fp64 numpy model of the device validation monitor (TEST INFRASTRUCTURE): the error sums of
pinn_val_stats, the record, the monitor-state update and the history ring.  The per-point values are formed exactly as
the kernel forms them (fp64 from the fp32 planes, one rounding per operation); the sums are exact (math.fsum), so a
comparison measures the kernel's summation error alone."""
import math

import numpy as np

RECORD, STATE = 8, 8
METRICS = dict(uv=0, u=1, v=2, p=3, p0=4)
# the sums, in the order of the kernel's scratch[1..11]
SUMS = ("D_u", "T_u", "n_u", "D_v", "T_v", "n_v", "D_p", "T_p", "n_p", "A", "B")
S_RECORDS, S_BEST, S_BEST_T, S_STALE, S_NONFINITE, S_IMPROVED, S_CADENCE = range(7)
R_T, R_EU, R_EV, R_EP, R_EP0, R_METRIC, R_IMPROVED, R_NP = range(8)


def new_state():
    st = np.zeros(STATE)
    st[S_BEST] = np.inf
    return st


def valid(t):
    """The finite-target rule of pinn_value_forward."""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore"):
        return (t == t) & (np.abs(t) <= np.float32(3.0e38))


def sums(pred, tgt):
    """pred, tgt: three fp32 arrays [n] each (the third pair None: no pressure).  The eleven sums, in SUMS order."""
    out = []
    for c in range(3):
        if pred[c] is None or tgt[c] is None:
            out += [0.0, 0.0, 0.0] + ([0.0, 0.0] if c == 2 else [])
            continue
        ok = valid(tgt[c])
        t = np.asarray(tgt[c], np.float32)[ok].astype(np.float64)
        d = np.asarray(pred[c], np.float32)[ok].astype(np.float64) - t
        out += [math.fsum(d * d), math.fsum(t * t), float(ok.sum())]
        if c == 2:
            out += [math.fsum(d), math.fsum(t)]
    return np.array(out)


def _ratio(a, b, cnt):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a) / np.float64(b))) if cnt > 0 else float("nan")


def errors(S, metric="uv"):
    """(e_u, e_v, e_p, e_p0, metric value) of the sums S."""
    S = [np.float64(v) for v in S]
    e_u, e_v, e_p = _ratio(S[0], S[1], S[2]), _ratio(S[3], S[4], S[5]), _ratio(S[6], S[7], S[8])
    e_p0 = float("nan")
    with np.errstate(all="ignore"):
        if S[8] > 0:
            num = S[6] - (S[9] * S[9]) / S[8]
            den = S[7] - (S[10] * S[10]) / S[8]
            if num < 0.0:
                num = np.float64(0.0)
            e_p0 = float(np.sqrt(num / den))
        uv = float(np.sqrt((S[0] + S[3]) / (S[1] + S[4]))) if S[2] > 0 and S[5] > 0 else float("nan")
    return e_u, e_v, e_p, e_p0, dict(uv=uv, u=e_u, v=e_v, p=e_p, p0=e_p0)[metric]


def record(S, metric, t, every, state, ring):
    """One validation with the sums S: writes its row into ring [capacity, RECORD] and updates state, both in place
    (t = -1: the cadence position from the state).  Returns the row."""
    e_u, e_v, e_p, e_p0, m = errors(S, metric)
    k = int(state[S_RECORDS])
    if t < 0:
        t = (state[S_CADENCE] + 1.0) * every
        state[S_CADENCE] += 1.0
    finite = math.isfinite(m)
    improved = finite and m < state[S_BEST]
    if improved:
        state[S_BEST], state[S_BEST_T], state[S_STALE] = m, t, 0.0
    else:
        state[S_STALE] += 1.0
    if not finite:
        state[S_NONFINITE] += 1.0
    state[S_IMPROVED] = 1.0 if improved else 0.0
    state[S_RECORDS] = k + 1.0
    row = np.array([t, e_u, e_v, e_p, e_p0, m, 1.0 if improved else 0.0, S[8]])
    ring[k % ring.shape[0]] = row
    return row


def validate(pred, tgt, metric, t, every, state, ring):
    """sums + record."""
    return record(sums(pred, tgt), metric, t, every, state, ring)


def history(state, ring):
    """The rows in time order, the ring unwrapped."""
    k, cap = int(state[S_RECORDS]), ring.shape[0]
    if k <= cap:
        return ring[:k].copy()
    return np.concatenate([ring[k % cap:], ring[:k % cap]])


def direct_errors(pred, tgt):
    """The definitions evaluated directly (np.linalg.norm, as the solvers' _errors does): e_u, e_v, e_p, e_p0, uv."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    out = []
    for c in range(3):
        if pred[c] is None:
            out.append(float("nan"))
            continue
        ok = valid(tgt[c])
        out.append(np.linalg.norm(f(pred[c])[ok] - f(tgt[c])[ok]) / np.linalg.norm(f(tgt[c])[ok]) if ok.any() else float("nan"))
    e_p0 = float("nan")
    if pred[2] is not None and valid(tgt[2]).any():
        ok = valid(tgt[2])
        d, t = f(pred[2])[ok] - f(tgt[2])[ok], f(tgt[2])[ok]
        with np.errstate(all="ignore"):
            e_p0 = np.linalg.norm(d - d.mean()) / np.linalg.norm(t - t.mean())
    oku, okv = valid(tgt[0]), valid(tgt[1])
    num = np.sum((f(pred[0])[oku] - f(tgt[0])[oku]) ** 2) + np.sum((f(pred[1])[okv] - f(tgt[1])[okv]) ** 2)
    den = np.sum(f(tgt[0])[oku] ** 2) + np.sum(f(tgt[1])[okv] ** 2)
    return out[0], out[1], out[2], e_p0, float(np.sqrt(num / den))
