"""fp64 model of the hard wall conditions (TEST INFRASTRUCTURE).

Two independent statements of the output transform u = g + D N_u, v = D N_v, p = N_p:
  * HardBcNet wraps oracle.autograd_ref.RefFCNet with the ansatz as a torch module, so fields, residuals, loss and the
    parameter gradient come from autograd through the ansatz (constrained_step);
  * transform_streams / transpose_streams are the closed-form forward-mode map of the four streams (value, d/dX, d/dY,
    Laplacian) and its transpose, operation by operation as the point stages write them, in numpy at any dtype (fp32:
    the stages' arithmetic up to the compiler's fused multiply-adds and the last place of expf);
  * constrained_fwdmode / constrained_value compose that map with oracle.fwdmode_ref's forward-mode sweeps: the
    constrained step as the kernels run it, in passes, so that a looping point count costs seconds, and with an
    optional relative error per Laplacian term for the sensitivity controls of tests/test_hardbc_terms.py.
"""
import numpy as np
import torch

from oracle import autograd_ref as ar


class HardBc:
    """The descriptor (pinn_hard_bc_t): X = (xi - x0) inv_len, Y = (eta - y0) inv_len."""

    def __init__(self, lift_power=2, lid_sharpness=10.0, origin=(0.0, 0.0), inv_len=1.0):
        self.m, self.r = int(lift_power), float(lid_sharpness)
        self.x0, self.y0, self.inv_len = float(origin[0]), float(origin[1]), float(inv_len)

    def struct(self):
        from nsfnet_amd import _lib
        return _lib.HardBcStruct(1, self.m, self.x0, self.y0, self.inv_len, self.r)


class HardBcNet(torch.nn.Module):
    """(u, v, p) = (g + D N_u, D N_v, N_p) of the wrapped net N; parameters() are N's, in its order."""

    def __init__(self, net, bc):
        super().__init__()
        self.net, self.bc = net, bc

    def forward(self, X):
        b = self.bc
        N = self.net(X)
        Xc, Yc = (X[:, 0] - b.x0) * b.inv_len, (X[:, 1] - b.y0) * b.inv_len
        D = 16.0 * Xc * (1.0 - Xc) * Yc * (1.0 - Yc)
        lid = 1.0 - torch.cosh(b.r * (Xc - 0.5)) / np.cosh(0.5 * b.r)
        g = lid * Yc ** b.m
        return torch.stack((g + D * N[:, 0], D * N[:, 1], N[:, 2]), dim=1)


def constrained_net(flat, L, H, bc):
    """HardBcNet over a fp64 RefFCNet(2, 3, L, H) holding the flat parameter vector."""
    net = ar.RefFCNet(2, 3, L, H).double()
    torch.nn.utils.vector_to_parameters(torch.as_tensor(np.asarray(flat), dtype=torch.float64), net.parameters())
    return HardBcNet(net, bc)


def _col(a, rg=False):
    return torch.tensor(np.asarray(a, dtype=np.float64)).reshape(-1, 1).requires_grad_(rg)


def physical_fields(model, x, y, scale=1.0):
    """u, v, p, the first derivatives and the Laplacians in the cavity's own coordinates, by autograd through `model`."""
    f = ar.ns_fields(model, x, y)
    s, s2 = scale, scale * scale
    return dict(u=f["u"], v=f["v"], p=f["p"], u_x=f["u_x"] * s, u_y=f["u_y"] * s, v_x=f["v_x"] * s, v_y=f["v_y"] * s,
                p_x=f["p_x"] * s, p_y=f["p_y"] * s, u_d=(f["u_xx"] + f["u_yy"]) * s2, v_d=(f["v_xx"] + f["v_yy"]) * s2)


def constrained_step(model, x, y, Re, xb, yb, ub, vb, alpha_b=1.0, alpha_e=1.0, scale=1.0, w=None, net_e=None,
                     vis_t=None, sup=None, alpha_s=0.0, eq4_weight=0.1):
    """One evaluation of the loss of PinnEngine.loss_and_grad on `model` (NSFnet/pinn_solver.py:197-226, ev-NSFnet/
    pinn_solver.py:372-428), everything fp64 by autograd: dict(fields, eqs, sums_eq, loss_b, loss_s, loss, grad[,
    grad_e], pred_b).  net_e: the entropy net (ev flavour; vis_t = the artificial viscosity of this evaluation).
    sup = (x, y, u, v, p): supervised samples, a NaN in p masks that pressure target."""
    xt, yt = _col(x, True), _col(y, True)
    f = physical_fields(model, xt, yt, scale)
    u, v = f["u"], f["v"]
    nu = 1.0 / Re + (0.0 if vis_t is None else _col(vis_t))
    eq1 = (u * f["u_x"] + v * f["u_y"]) + f["p_x"] - nu * f["u_d"]
    eq2 = (u * f["v_x"] + v * f["v_y"]) + f["p_y"] - nu * f["v_d"]
    eqs = [eq1, eq2, f["u_x"] + f["v_y"]]
    weights = [1.0, 1.0, 1.0]
    if net_e is not None:
        e = net_e(torch.cat((xt, yt), dim=1))[:, 0:1]
        eqs.append((eq1 * (u - 0.5) + eq2 * (v - 0.5)) - e)
        weights.append(eq4_weight)
    wt = 1.0 if w is None else _col(w)
    sums_eq = [torch.sum(wt * r * r) for r in eqs]
    loss_e = sum(c * s for c, s in zip(weights, sums_eq)) / len(np.asarray(x).reshape(-1))
    pred_b = model(torch.cat((_col(xb), _col(yb)), dim=1))
    loss_b = (torch.mean(torch.square(_col(ub).reshape(-1) - pred_b[:, 0])) +
              torch.mean(torch.square(_col(vb).reshape(-1) - pred_b[:, 1])))
    loss_s = torch.zeros((), dtype=torch.float64)
    if sup is not None and alpha_s != 0.0:
        out = model(torch.cat((_col(sup[0]), _col(sup[1])), dim=1))
        loss_s = (torch.mean(torch.square(_col(sup[2]).reshape(-1) - out[:, 0])) +
                  torch.mean(torch.square(_col(sup[3]).reshape(-1) - out[:, 1])))
        if sup[4] is not None:
            ok = torch.tensor(np.isfinite(np.asarray(sup[4], dtype=np.float64)).reshape(-1))
            if bool(ok.any()):
                loss_s = loss_s + torch.mean(torch.square(_col(sup[4]).reshape(-1)[ok] - out[:, 2][ok]))
    loss = alpha_b * loss_b + alpha_e * loss_e + alpha_s * loss_s
    params = list(model.parameters()) + ([] if net_e is None else list(net_e.parameters()))
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, params)]
    n_main = len(list(model.parameters()))
    flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).numpy()
    out = dict(fields={k: t.detach().numpy().reshape(-1) for k, t in f.items()},
               eqs=[r.detach().numpy().reshape(-1) for r in eqs], sums_eq=[float(s.detach()) for s in sums_eq],
               loss_b=float(loss_b.detach()), loss_s=float(loss_s.detach()), loss=float(loss.detach()), grad=flat(grads[:n_main]),
               pred_b=pred_b.detach().numpy())
    if net_e is not None:
        out["grad_e"] = flat(grads[n_main:])
    return out


# ---- the closed-form map of the point stages (include/nsfnet_pinn.h, "hard boundary conditions") ----
def point_factors(bc, xi, eta, dtype=np.float64):
    """dict(D, Dx, Dy, Dd, g, gx, gy, gd) at the points, every operation in `dtype`; c = 1 / cosh(r / 2) in double,
    rounded to `dtype`; Y^m by repeated multiplication."""
    t = dtype
    xi, eta = np.asarray(xi, dtype=t), np.asarray(eta, dtype=t)
    one, two, half = t(1.0), t(2.0), t(0.5)
    X, Y = (xi - t(bc.x0)) * t(bc.inv_len), (eta - t(bc.y0)) * t(bc.inv_len)
    ax, ay = X * (one - X), Y * (one - Y)
    r, c = t(bc.r), t(1.0 / np.cosh(0.5 * bc.r))
    arg = r * (X - half)
    ep, em = np.exp(arg), np.exp(-arg)
    ch, sh = half * (ep + em) * c, half * (ep - em) * c
    lid, lid1, lid2 = one - ch, -r * sh, -r * r * ch
    pm2 = np.ones_like(Y)
    for _ in range(2, bc.m):
        pm2 = pm2 * Y
    pm1 = pm2 * Y if bc.m >= 2 else np.ones_like(Y)
    pm = pm1 * Y
    fm = t(bc.m)
    return dict(D=t(16.0) * ax * ay, Dx=t(16.0) * (one - two * X) * ay, Dy=t(16.0) * ax * (one - two * Y),
                Dd=t(-32.0) * (ax + ay), g=lid * pm, gx=lid1 * pm, gy=lid * fm * pm1,
                gd=lid2 * pm + lid * (fm * (fm - one)) * pm2)


# The seven Laplacian-stream terms of the map and its transpose (each enters the loss with weight nu only) and the value
# mode's D: the keys of `rel`, a dict of relative errors the closed forms below take for the sensitivity controls.
FORWARD_TERMS = ("lap_g", "lapD_N", "cross", "D_lapN")      # Lap g, Lap D N, 2 (D_X N_X + D_Y N_Y), D Lap N
TRANSPOSE_TERMS = ("t_lapD", "t_cross", "t_D")              # Lap D a_D, 2 D_X a_D / 2 D_Y a_D, D a_D
LAPLACIAN_TERMS = FORWARD_TERMS + TRANSPOSE_TERMS
VALUE_TERM = "v_D"                                          # the D of the value mode's adjoint


def _gain(rel, key):
    return 1.0 + (0.0 if not rel else float(rel.get(key, 0.0)))


def transform_streams(h, n, nx, ny, nd, lift, rel=None):
    """(c, c_X, c_Y, Lap c) of c = lift g + D N from the net's streams (N, N_X, N_Y, Lap N).  rel: relative errors of
    the Laplacian's terms (FORWARD_TERMS), for the controls."""
    two = h["D"].dtype.type(2.0)
    c = h["D"] * n
    cx = h["Dx"] * n + h["D"] * nx
    cy = h["Dy"] * n + h["D"] * ny
    if not rel:
        cd = h["Dd"] * n + two * (h["Dx"] * nx + h["Dy"] * ny) + h["D"] * nd
    else:
        cd = (_gain(rel, "lapD_N") * (h["Dd"] * n) + _gain(rel, "cross") * (two * (h["Dx"] * nx + h["Dy"] * ny)) +
              _gain(rel, "D_lapN") * (h["D"] * nd))
    if lift:
        c, cx, cy, cd = h["g"] + c, h["gx"] + cx, h["gy"] + cy, (h["gd"] if not rel else _gain(rel, "lap_g") * h["gd"]) + cd
    return c, cx, cy, cd


def transpose_streams(h, a, ax, ay, ad, rel=None):
    """Adjoints of the net's four streams from the adjoints of (c, c_X, c_Y, Lap c).  rel: relative errors of the
    terms that carry a_D (TRANSPOSE_TERMS), for the controls."""
    two = h["D"].dtype.type(2.0)
    if not rel:
        return (h["D"] * a + h["Dx"] * ax + h["Dy"] * ay + h["Dd"] * ad, h["D"] * ax + two * h["Dx"] * ad,
                h["D"] * ay + two * h["Dy"] * ad, h["D"] * ad)
    kd, kc, k0 = _gain(rel, "t_lapD"), _gain(rel, "t_cross"), _gain(rel, "t_D")
    return (h["D"] * a + h["Dx"] * ax + h["Dy"] * ay + kd * (h["Dd"] * ad), h["D"] * ax + kc * (two * h["Dx"] * ad),
            h["D"] * ay + kc * (two * h["Dy"] * ad), k0 * (h["D"] * ad))


# ---- the constrained step in forward mode: what the kernels run, pass by pass, in fp64 ----
def _factors64(bc, x, y, factor_dtype):
    h = point_factors(bc, x, y, dtype=factor_dtype)
    return {k: np.asarray(v, dtype=np.float64) for k, v in h.items()}


def constrained_fwdmode(params, bc, x, y, Re, alpha_e=1.0, vis_t=None, e=None, w=None, scale=1.0, eq4_weight=0.1,
                        params_e=None, chunk=8192, rel=None, factor_dtype=np.float64):
    """The residual term of a constrained plan as the sweeps compute it: fr.forward4, the scale factors, the map of
    the point stage (transform_streams), fr.residuals, the output-adjoint seeds of fr.pde_loss_and_grad, the transpose
    (transpose_streams), the scale factors again, fr.backward4 - in passes of <= chunk points normalised by the global
    N, like fr.pde_loss_and_grad_chunked, whose arguments these are (params: fr.unflatten's pairs; params_e: the
    entropy net, e defaults to its output, grad_e is its gradient).  rel: relative errors per term (LAPLACIAN_TERMS);
    factor_dtype: the dtype point_factors runs in (fp32: the stage's own factors, pushed through this fp64 model).
    Returns dict(fields: u, v, p, u_x, u_y, v_x, v_y; eqs; sums; grad[, grad_e])."""
    from oracle import fwdmode_ref as fr
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N, s, s2 = x.size, float(scale), float(scale) * float(scale)
    opt = lambda a, lo, hi: None if a is None else np.asarray(a, dtype=np.float64).reshape(-1)[lo:hi]
    cw = [1.0, 1.0, 1.0, eq4_weight]
    sums, grad, grad_e, eqs_all, flds = None, None, None, [], []
    for lo in range(0, N, int(chunk)):
        hi = min(N, lo + int(chunk))
        xs, ys = x[lo:hi], y[lo:hi]
        ek, saved_e = opt(e, lo, hi), None
        if params_e is not None:
            ev, saved_e = fr.forward1(params_e, xs, ys)
            if ek is None:
                ek = ev[:, 0]
        out, saved = fr.forward4(params, xs, ys)
        h = _factors64(bc, xs.astype(factor_dtype), ys.astype(factor_dtype), factor_dtype)
        phys = out * np.array([1.0, s, s, s2])                  # derivatives in the cavity's own X, Y
        con = phys.copy()
        for c, lift in ((0, True), (1, False)):
            con[:, c, :] = np.stack(transform_streams(h, *(phys[:, c, k] for k in range(4)), lift=lift, rel=rel), axis=1)
        vt = opt(vis_t, lo, hi)
        eqs = fr.residuals(con, Re, vt, ek, 1.0)
        ww = np.ones(hi - lo) if w is None else opt(w, lo, hi)
        ps = np.array([float(np.sum(ww * q * q)) for q in eqs])
        g = [2.0 * alpha_e * cw[k] * ww * eqs[k] / N for k in range(len(eqs))]
        u, v = con[:, 0, 0], con[:, 1, 0]
        nu = 1.0 / Re + (0.0 if vt is None else vt)
        g4 = g[3] if len(eqs) == 4 else np.zeros(hi - lo)
        r1, r2, r3 = g[0] + g4 * (u - 0.5), g[1] + g4 * (v - 0.5), g[2]
        adj = np.zeros_like(con)                                # adjoints of the constrained streams (and of p's)
        adj[:, 0, 0] = r1 * con[:, 0, 1] + r2 * con[:, 1, 1] + (g4 * eqs[0] if len(eqs) == 4 else 0.0)
        adj[:, 1, 0] = r1 * con[:, 0, 2] + r2 * con[:, 1, 2] + (g4 * eqs[1] if len(eqs) == 4 else 0.0)
        adj[:, 0, 1], adj[:, 0, 2], adj[:, 0, 3] = r1 * u + r3, r1 * v, -nu * r1
        adj[:, 1, 1], adj[:, 1, 2], adj[:, 1, 3] = r2 * u, r2 * v + r3, -nu * r2
        adj[:, 2, 1], adj[:, 2, 2] = r1, r2
        for c in (0, 1):
            adj[:, c, :] = np.stack(transpose_streams(h, *(adj[:, c, k] for k in range(4)), rel=rel), axis=1)
        gk, _ = fr.backward4(params, xs, ys, saved, adj * np.array([1.0, s, s, s2]))
        sums = ps if sums is None else sums + ps
        grad = gk if grad is None else grad + gk
        if params_e is not None:
            ge = fr.backward1(params_e, xs, ys, saved_e, (-g4).reshape(-1, 1))
            grad_e = ge if grad_e is None else grad_e + ge
        eqs_all.append(eqs)
        flds.append(con)
    con = np.concatenate(flds)
    res = dict(sums=[float(q) for q in sums], grad=grad,
               eqs=[np.concatenate([q[k] for q in eqs_all]) for k in range(len(eqs_all[0]))],
               fields=dict(u=con[:, 0, 0], v=con[:, 1, 0], p=con[:, 2, 0], u_x=con[:, 0, 1], u_y=con[:, 0, 2],
                           v_x=con[:, 1, 1], v_y=con[:, 1, 2], u_d=con[:, 0, 3], v_d=con[:, 1, 3], p_x=con[:, 2, 1],
                           p_y=con[:, 2, 2]))
    if params_e is not None:
        res["grad_e"] = grad_e
    return res


def constrained_value(params, bc, x, y, targets=None, coef=None, chunk=8192, rel=None, factor_dtype=np.float64):
    """Value mode of a constrained plan: fr.forward1, pred_u = g + D N_u, pred_v = D N_v, pred_p = N_p, the squared
    errors against the finite targets (NaN / inf = masked), the net's output adjoints coef (pred - target) D (p: no D),
    fr.backward1 - in passes like fr.value_loss_and_grad_chunked, whose arguments and result these are.  rel: the
    relative error of the adjoint's D (VALUE_TERM)."""
    from oracle import fwdmode_ref as fr
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N = x.size
    tg = [None if t is None else np.asarray(t, dtype=np.float64).reshape(-1) for t in (list(targets or ()) + [None] * 3)[:3]]
    cf = np.zeros(3) if coef is None else np.asarray(coef, dtype=np.float64).reshape(-1)[:3]
    sums, grad, preds = np.zeros(4), None, []
    for lo in range(0, N, int(chunk)):
        hi = min(N, lo + int(chunk))
        xs, ys = x[lo:hi], y[lo:hi]
        net, saved = fr.forward1(params, xs, ys)
        h = _factors64(bc, xs.astype(factor_dtype), ys.astype(factor_dtype), factor_dtype)
        pred = np.stack([h["g"] + h["D"] * net[:, 0], h["D"] * net[:, 1], net[:, 2]], axis=1)
        adj = np.zeros_like(pred)
        for c in range(3):
            if tg[c] is None:
                continue
            ok = np.isfinite(tg[c][lo:hi])
            d = np.where(ok, pred[:, c] - np.where(ok, tg[c][lo:hi], 0.0), 0.0)
            sums[c] += np.sum(d * d)
            if c == 2:
                sums[3] += ok.sum()
            adj[:, c] = cf[c] * d * (_gain(rel, VALUE_TERM) * h["D"] if c < 2 else 1.0)
        gk = fr.backward1(params, xs, ys, saved, adj)
        grad = gk if grad is None else grad + gk
        preds.append(pred)
    return dict(pred=np.concatenate(preds), sums=[float(q) for q in sums], grad=grad)


def special_points(lo=0.0, hi=1.0):
    """The four corners, one point on each wall and the centre of the cavity [lo, hi]^2."""
    m, q = 0.5 * (lo + hi), lo + 0.25 * (hi - lo)
    x = [lo, hi, lo, hi, q, m, lo, hi, m]
    y = [lo, lo, hi, hi, lo, hi, m, q, m]
    return np.array(x, dtype=np.float32), np.array(y, dtype=np.float32)
