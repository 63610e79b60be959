"""fp64 model of the pseudo-time stepping of the residual loss (TEST INFRASTRUCTURE; numpy).

The formulation (include/nsfnet_pinn.h, "pseudo-time stepping"): with anchors (u*, v*, p*) per point and the rates
sigma, sigma_p >= 0

    q1 = eq1 + sigma (u - u*)     q2 = eq2 + sigma (v - v*)     q3 = eq3 + sigma_p (p - p*)
    eq4 = eq1 (u - 1/2) + eq2 (v - 1/2) - e                      (on the STEADY eq1, eq2)
    loss_e = alpha_e / N sum_i w_i (q1^2 + q2^2 + q3^2 + eq4_weight eq4^2)

  * residual_term composes oracle.fwdmode_ref's forward-mode sweeps (forward4 / backward4) with the seeds of the
    header, and with the output transform of tests/hardbc_model.py where the walls are hard: the term as the point
    stages compute it, in fp64, in passes like hardbc_model.constrained_fwdmode;
  * advance is pinn_ptime_advance: the record's sums and maximum in the kernel's fold order (tests/fold_model.py), so
    they are meant to be compared bit for bit, and the anchor refresh on its cadence.
"""
import numpy as np

import fold_model as fm
import hardbc_model as hm
from oracle import fwdmode_ref as fr

# field planes (csrc/kernels.h) and the record (PINN_PTIME_RECORD)
FLD_U, FLD_V, FLD_EQ1, FLD_EQ2, FLD_EQ3, FLD_P, FLD_COUNT = 0, 1, 6, 7, 8, 10, 11
RECORD = 8
R_STEADY, R_DRIFT_UV, R_DRIFT_P, R_MAX, R_SINCE, R_REFRESHES = 0, 3, 4, 5, 6, 7
THREADS, PER, MAX_BLOCKS = 256, 4, 512
# the places the pseudo-time term is written out in a point stage, each a separate place to go wrong (residual_term's
# `errors`): the drift sigma_k (c_k - c_k*) as it enters the loss sums (fwd_q*), as the reverse sweep rebuilds it for
# g_k (bwd_q*), the value seeds sigma g1, sigma g2, sigma_p g3 (seed_*), and eq4 built on q1, q2 (eq4_on_q, boolean)
FORWARD_TERMS = ("fwd_q1", "fwd_q2", "fwd_q3")
REVERSE_TERMS = ("bwd_q1", "bwd_q2", "bwd_q3")
SEED_TERMS = ("seed_u", "seed_v", "seed_p")
TERMS = FORWARD_TERMS + REVERSE_TERMS + SEED_TERMS + ("eq4_on_q",)


def residual_term(params, x, y, Re, anchor, sigma, sigma_p, alpha_e=1.0, vis_t=None, e=None, w=None, scale=1.0,
                  eq4_weight=0.1, bc=None, params_e=None, chunk=8192, errors=None):
    """The pseudo-time residual term and its gradient.  params: fr.unflatten's pairs; anchor [3, N] (u*, v*, p*); bc: a
    hardbc_model.HardBc (u, v are then the constrained fields) or None; params_e: the entropy net (e defaults to its
    output and grad_e is its gradient); the other arguments as fr.pde_loss_and_grad.  In passes of <= chunk points, each
    normalised by the global N.  errors: {term of TERMS: factor} - that term alone is multiplied by the factor (0 drops
    it, 1 + 2^-8 is one dropped bf16 term), or eq4_on_q=True: eq4 and its seeds on q1, q2, the mistake the header warns
    of; None changes no bit of any result.  q is always the exact one.  Returns dict(fields: u, v, p, u_x, u_y, v_x, v_y; eqs: the steady eq1..eq3[, eq4];
    q: q1..q3; sums: sum w q_k^2 (k = 1..3)[, sum w eq4^2]; steady_sums: sum w eq_k^2 (k = 1..3); loss_e; grad[,
    grad_e])."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    anchor = np.asarray(anchor, dtype=np.float64).reshape(3, -1)
    N, s, s2 = x.size, float(scale), float(scale) * float(scale)
    assert anchor.shape[1] == N
    opt = lambda a, lo, hi: None if a is None else np.asarray(a, dtype=np.float64).reshape(-1)[lo:hi]
    cw = [1.0, 1.0, 1.0, eq4_weight]
    rates = (float(sigma), float(sigma), float(sigma_p))
    er = {} if errors is None else dict(errors)
    assert set(er) <= set(TERMS), sorted(set(er) - set(TERMS))
    fac = lambda t: float(er.get(t, 1.0))
    on_q = bool(er.get("eq4_on_q", False))
    sums, steady, grad, grad_e, eqs_all, q_all, flds = None, None, None, None, [], [], []
    for lo in range(0, N, int(chunk)):
        hi = min(N, lo + int(chunk))
        xs, ys = x[lo:hi], y[lo:hi]
        ek, saved_e = opt(e, lo, hi), None
        if params_e is not None:
            ev, saved_e = fr.forward1(params_e, xs, ys)
            if ek is None:
                ek = ev[:, 0]
        out, saved = fr.forward4(params, xs, ys)
        con = out * np.array([1.0, s, s, s2])                   # derivatives in the physical coordinates
        if bc is not None:
            h = hm.point_factors(bc, xs, ys)
            phys = con.copy()
            for c, lift in ((0, True), (1, False)):
                con[:, c, :] = np.stack(hm.transform_streams(h, *(phys[:, c, k] for k in range(4)), lift=lift), axis=1)
        vt = opt(vis_t, lo, hi)
        eqs = fr.residuals(con, Re, vt, ek, 1.0)
        ww = np.ones(hi - lo) if w is None else opt(w, lo, hi)
        drift = [rates[k] * (con[:, k, 0] - anchor[k, lo:hi]) for k in range(3)]
        q = [eqs[k] + drift[k] for k in range(3)]
        u, v = con[:, 0, 0], con[:, 1, 0]
        if on_q and len(eqs) == 4:
            eqs[3] = q[0] * (u - 0.5) + q[1] * (v - 0.5) - np.asarray(ek).reshape(-1)
        mins = q + eqs[3:]                                      # what the loss squares
        mins_b = mins                                           # ... and what the reverse sweep rebuilds for g_k
        if er:
            mins = [eqs[k] + fac(FORWARD_TERMS[k]) * drift[k] for k in range(3)] + eqs[3:]
            mins_b = [eqs[k] + fac(REVERSE_TERMS[k]) * drift[k] for k in range(3)] + eqs[3:]
        ps = np.array([float(np.sum(ww * r * r)) for r in mins])
        st = np.array([float(np.sum(ww * r * r)) for r in eqs[:3]])
        g = [2.0 * alpha_e * cw[k] * ww * mins_b[k] / N for k in range(len(mins_b))]
        nu = 1.0 / Re + (0.0 if vt is None else vt)
        ev_on = len(eqs) == 4
        g4 = g[3] if ev_on else np.zeros(hi - lo)
        r1, r2, r3 = g[0] + g4 * (u - 0.5), g[1] + g4 * (v - 0.5), g[2]
        adj = np.zeros_like(con)
        e1, e2, s1, s2g = (q[0], q[1], r1, r2) if on_q else (eqs[0], eqs[1], g[0], g[1])
        seed = [rates[0] * s1, rates[1] * s2g, rates[2] * g[2]]
        if er:
            seed = [fac(SEED_TERMS[k]) * seed[k] for k in range(3)]
        adj[:, 0, 0] = r1 * con[:, 0, 1] + r2 * con[:, 1, 1] + (g4 * e1 if ev_on else 0.0) + seed[0]
        adj[:, 1, 0] = r1 * con[:, 0, 2] + r2 * con[:, 1, 2] + (g4 * e2 if ev_on else 0.0) + seed[1]
        adj[:, 2, 0] = seed[2]
        adj[:, 0, 1], adj[:, 0, 2], adj[:, 0, 3] = r1 * u + r3, r1 * v, -nu * r1
        adj[:, 1, 1], adj[:, 1, 2], adj[:, 1, 3] = r2 * u, r2 * v + r3, -nu * r2
        adj[:, 2, 1], adj[:, 2, 2] = r1, r2
        if bc is not None:
            for c in (0, 1):
                adj[:, c, :] = np.stack(hm.transpose_streams(h, *(adj[:, c, k] for k in range(4))), axis=1)
        gk, _ = fr.backward4(params, xs, ys, saved, adj * np.array([1.0, s, s, s2]))
        sums = ps if sums is None else sums + ps
        steady = st if steady is None else steady + st
        grad = gk if grad is None else grad + gk
        if params_e is not None:
            ge = fr.backward1(params_e, xs, ys, saved_e, (-g4).reshape(-1, 1))
            grad_e = ge if grad_e is None else grad_e + ge
        eqs_all.append(eqs)
        q_all.append(q)
        flds.append(con)
    con = np.concatenate(flds)
    cat = lambda parts: [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]
    res = dict(sums=[float(v) for v in sums], steady_sums=[float(v) for v in steady], grad=grad, eqs=cat(eqs_all),
               q=cat(q_all), loss_e=alpha_e * float(sum(cw[k] * sums[k] for k in range(len(sums)))) / N,
               fields=dict(u=con[:, 0, 0], v=con[:, 1, 0], p=con[:, 2, 0], u_x=con[:, 0, 1], u_y=con[:, 0, 2],
                           v_x=con[:, 1, 1], v_y=con[:, 1, 2]))
    if params_e is not None:
        res["grad_e"] = grad_e
    return res


def balanced_rates(r):
    """(sigma_bal, sigma_p_bal) of a residual_term result evaluated at any rates: the rates at which the pseudo-time
    terms weigh what the steady residuals do, sqrt(sum(eq1^2 + eq2^2) / sum((u-u*)^2 + (v-v*)^2)) and likewise from eq3
    and p - the drifts come back out of q - eq when the rates were not 0, so evaluate at (1, 1)."""
    e, q = r["eqs"], r["q"]
    d = [q[k] - e[k] for k in range(3)]
    return (float(np.sqrt(np.sum(e[0] ** 2 + e[1] ** 2) / np.sum(d[0] ** 2 + d[1] ** 2))),
            float(np.sqrt(np.sum(e[2] ** 2) / np.sum(d[2] ** 2))))


def amplification(r, anchor, sigma, sigma_p):
    """A = max_k (max|eq_k| + sigma_k max|c_k|) / max|q_k|, c = (u, v, p): the first-order growth of q's relative error
    over that of its parts, from the cancellation in eq + sigma (c - c*)."""
    f = r["fields"]
    c = (f["u"], f["v"], f["p"])
    rates = (sigma, sigma, sigma_p)
    return max((np.abs(r["eqs"][k]).max() + rates[k] * np.abs(c[k]).max()) / np.abs(r["q"][k]).max() for k in range(3))


def blocks(n):
    return min(-(-int(n) // (THREADS * PER)), MAX_BLOCKS)


def advance(fld, n, anchor, every, force=False, w=None, record=None):
    """pinn_ptime_advance.  fld [FLD_COUNT, npad] fp32 planes, anchor [3, npad] fp32, w [n] fp32 or None, record
    [RECORD] fp64 or None (zeros).  Returns (anchor, record) as new arrays: the sums of the record in the kernel's fold
    order; the refresh (record[6] + 1 >= every with every >= 1, or force) copies U, V, P into the anchors in whole quads
    of four points, up to the next multiple of 4 past n."""
    fld = np.asarray(fld, dtype=np.float32)
    anchor = np.array(anchor, dtype=np.float32)
    rec = np.zeros(RECORD) if record is None else np.array(record, dtype=np.float64)
    n = int(n)
    ww = np.ones(n) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)[:n]
    p64 = lambda k: fld[k, :n].astype(np.float64)
    nb = blocks(n)
    with np.errstate(all="ignore"):
        du, dv, dp = p64(FLD_U) - anchor[0, :n], p64(FLD_V) - anchor[1, :n], p64(FLD_P) - anchor[2, :n]
        vals = [ww * (p64(k) * p64(k)) for k in (FLD_EQ1, FLD_EQ2, FLD_EQ3)]
        vals += [ww * (du * du + dv * dv), ww * (dp * dp)]
        mx = fm.NANMAX[1](np.abs(du), np.abs(dv))
    for c, v in enumerate(vals):
        rec[c] = fm.grid_fold(v, nb, fm.SUM, THREADS, PER)
    rec[R_MAX] = fm.grid_fold(mx, nb, fm.NANMAX, THREADS, PER)
    refresh = bool(force) or (every >= 1 and rec[R_SINCE] + 1.0 >= every)
    if refresh:
        n4 = -(-n // 4) * 4
        anchor[0, :n4], anchor[1, :n4], anchor[2, :n4] = fld[FLD_U, :n4], fld[FLD_V, :n4], fld[FLD_P, :n4]
        rec[R_SINCE] = 0.0
        rec[R_REFRESHES] += 1.0
    else:
        rec[R_SINCE] += 1.0
    return anchor, rec
