"""numpy statement of the convergence monitor's two launches (csrc/monitor.hip; TEST INFRASTRUCTURE): the vis_t
statistics in the kernel's fold order through tests/fold_model.py, and the observation with its window logic in the
order include/nsfnet_pinn.h states - every operation a correctly rounded fp64 one, so results are meant to be compared
bit for bit."""
import numpy as np

import fold_model as fm

RECORD, STATE, INFO = 12, 16, 4
STOP_PLATEAU, STOP_RE_EFF, STOP_NONFINITE = 1, 2, 4
QUANTITIES = dict(loss=0, loss_e=1, loss_b=2)
THREADS, PER, MAX_BLOCKS = 256, 4, 512
TILE = THREADS * PER
(S_UPDATES, S_OBS, S_NONFINITE, S_FILL, S_SUM_Q, S_SUM_RE, S_WINDOWS, S_PREV_Q, S_PREV_RE, S_STALE, S_SETTLED, S_STOP,
 S_T_PLATEAU, S_T_RE_EFF, S_T_NONFINITE) = range(15)
NLOSS = 8


def blocks(n):
    return min(-(-int(n) // TILE), MAX_BLOCKS)


def vis_stats(vis_t, vis_t0):
    """(the fp32 sum slot, info [max, count >= vis_t0, fp64 sum, n]) of the fp32 plane vis_t."""
    v = np.asarray(vis_t, dtype=np.float32).reshape(-1)
    nblk = blocks(v.size)
    with np.errstate(invalid="ignore"):
        cnt = (v >= np.float32(vis_t0)).astype(np.float64)
    v64 = v.astype(np.float64)
    parts = np.stack([fm.grid_partials(v64, nblk, fm.SUM, THREADS, PER),
                      fm.grid_partials(v64, nblk, fm.NANMAX, THREADS, PER),
                      fm.grid_partials(cnt, nblk, fm.SUM, THREADS, PER)], axis=1)
    s, mx, c = fm.strided_tree_fold(parts, [fm.SUM, fm.NANMAX, fm.SUM], THREADS)
    with np.errstate(over="ignore", invalid="ignore"):
        slot = np.float32(s)
    return slot, np.array([mx, c, s, float(v.size)])


class Config:
    def __init__(self, every=1, window=1000, min_rel_improvement=1e-3, patience=3, re_eff_tol=None, min_updates=0,
                 quantity="loss", capacity=4096, ev=False):
        self.every, self.window, self.patience, self.min_updates = int(every), int(window), int(patience), int(min_updates)
        self.min_rel, self.re_tol = min_rel_improvement, re_eff_tol
        self.quantity, self.capacity, self.ev = quantity, int(capacity), bool(ev)


def new_state():
    return np.zeros(STATE)


def new_ring(cfg):
    return np.zeros((cfg.capacity, RECORD))


def terms(eq, bc, sup, lam, alpha_b, alpha_s, alpha_e, w4, n_eq, n_b, n_s, n_p, Re, ev):
    """[loss, loss_e, loss_b, loss_s, eq_0..eq_3, vis_mean, Re_eff] in fp64 from the fp32 sums, in the header's order."""
    f = lambda v: np.float64(np.float32(v))
    with np.errstate(all="ignore"):
        n_eq, n_b, n_s, n_p, Re = (np.float64(v) for v in (n_eq, n_b, n_s, n_p, Re))
        e = [f(eq[k]) / n_eq for k in range(4)]
        loss_e = (e[0] + e[1]) + e[2]
        if ev:
            loss_e = loss_e + np.float64(w4) * e[3]
        loss_b = (f(bc[0]) + f(bc[1])) / n_b
        loss_s = np.float64(0.0)
        if sup is not None and n_s > 0:
            loss_s = (f(sup[0]) + f(sup[1])) / n_s
            if n_p > 0:
                loss_s = loss_s + f(sup[2]) / n_p
        w_b, w_s = (np.float64(alpha_b), np.float64(alpha_s)) if lam is None else (f(lam[0]), f(lam[1]))
        loss = ((w_b * loss_b) + (np.float64(alpha_e) * loss_e)) + (w_s * loss_s)
        vis = f(eq[4]) / n_eq if ev else np.float64(0.0)
        re_eff = np.float64(1.0) / (np.float64(1.0) / Re + vis)
    return [loss, loss_e, loss_b, loss_s] + e + [vis, re_eff]


def observe_terms(cfg, st, ring, tm):
    """One call of the observation launch on the terms tm (of `terms`): st and ring are updated in place.  Returns
    True when the update was observed."""
    t = st[S_UPDATES] + 1.0
    st[S_UPDATES] = t
    if int(t) % cfg.every != 0:
        return False
    loss, loss_e, loss_b = tm[0], tm[1], tm[2]
    re_eff = tm[9]
    nobs = st[S_OBS]
    st[S_OBS] = nobs + 1.0
    code = int(st[S_STOP])
    with np.errstate(all="ignore"):
        if not np.isfinite(loss):
            st[S_NONFINITE] += 1.0
            if not code & STOP_NONFINITE:
                code |= STOP_NONFINITE
                st[S_T_NONFINITE] = t
        else:
            q = (loss, loss_e, loss_b)[QUANTITIES[cfg.quantity]]
            st[S_FILL] += 1.0
            st[S_SUM_Q] = st[S_SUM_Q] + q
            st[S_SUM_RE] = st[S_SUM_RE] + re_eff
            if st[S_FILL] >= cfg.window:
                w = np.float64(cfg.window)
                mean, mean_re = st[S_SUM_Q] / w, st[S_SUM_RE] / w
                if st[S_WINDOWS] >= 1.0:
                    if cfg.min_rel is not None:
                        prev = st[S_PREV_Q]
                        stale = prev == 0.0 or bool((prev - mean) / np.abs(prev) < np.float64(cfg.min_rel))
                        st[S_STALE] = st[S_STALE] + 1.0 if stale else 0.0
                    if cfg.re_tol is not None:
                        prev = st[S_PREV_RE]
                        settled = bool(np.abs(mean_re - prev) / prev < np.float64(cfg.re_tol))
                        st[S_SETTLED] = st[S_SETTLED] + 1.0 if settled else 0.0
                st[S_PREV_Q], st[S_PREV_RE] = mean, mean_re
                st[S_WINDOWS] += 1.0
                st[S_FILL] = st[S_SUM_Q] = st[S_SUM_RE] = 0.0
    if t >= cfg.min_updates:
        if cfg.min_rel is not None and st[S_STALE] >= cfg.patience and not code & STOP_PLATEAU:
            code |= STOP_PLATEAU
            st[S_T_PLATEAU] = t
        if cfg.re_tol is not None and st[S_SETTLED] >= cfg.patience and not code & STOP_RE_EFF:
            code |= STOP_RE_EFF
            st[S_T_RE_EFF] = t
    st[S_STOP] = float(code)
    row = ring[int(nobs) % cfg.capacity]
    row[0] = t
    row[1:11] = tm
    row[11] = float(code)
    return True


def observe(cfg, st, ring, eq, bc, sup=None, lam=None, alpha_b=1.0, alpha_s=0.0, alpha_e=1.0, w4=0.1, n_eq=1.0, n_b=1.0,
            n_s=0.0, n_p=0.0, Re=100.0):
    """pinn_monitor_observe on the fp32 loss-sum blocks."""
    return observe_terms(cfg, st, ring, terms(eq, bc, sup, lam, alpha_b, alpha_s, alpha_e, w4, n_eq, n_b, n_s, n_p, Re,
                                              cfg.ev))


def observe_losses(cfg, st, ring, loss, re_eff=1.0):
    """An observation of a synthetic sequence: every term is `loss`."""
    return observe_terms(cfg, st, ring, [np.float64(loss)] * 4 + [np.float64(0.0)] * 4 + [np.float64(0.0),
                                                                                         np.float64(re_eff)])


def unwrap(st, ring):
    """The ring's rows in time order."""
    k, cap = int(st[S_OBS]), ring.shape[0]
    if k <= cap:
        return ring[:k].copy()
    return np.concatenate([ring[k % cap:], ring[:k % cap]])
