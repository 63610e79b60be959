"""fp64 statement of the viscosity identification (csrc/visc.hip, PinnEngine.set_viscosity_identification; TEST
INFRASTRUCTURE): the Laplacian planes and the sum S of d loss / d nu = -(2 alpha_e / N) S from oracle.fwdmode_ref, a
numpy restatement of pinn_visc_update, operation by operation, and the Kovasznay flow with the fp64 training run the
GPU test is judged against.

    python tests/visc_model.py --write        runs the fp64 model of the Kovasznay identification (KOV below) and writes
                                              tests/golden/visc_kovasznay_4x50.npz: Re after every 100 updates
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fwdmode_ref as fr  # noqa: E402

STATE = 8       # PINN_VISC_STATE: theta, m, v, beta1^t, beta2^t, t, last G, skipped
SLOT = 5        # the slot of the equation block of the loss sums that carries S
GOLDEN = os.path.join(ROOT, "tests", "golden", "visc_kovasznay_4x50.npz")


# ---- one evaluation ----
def evaluate(flat, L, H, x, y, nu, alpha_e=1.0, vis_t=None, e=None, w=None, scale=1.0, w4=0.1, bc=None, want_grad=True,
             ff=False):
    """The collocation term at viscosity nu (Re = 1 / nu): dict(u, v, eqs, lap = (Lap u, Lap v) physical, sums, loss_e,
    grad (d loss_e / d params), t (the per-point terms), S, kappa = sum|t| / |S|, dnu = -(2 alpha_e / N) S).  bc: a
    hardbc_model.HardBc - the constrained fields of a hard-wall plan (scale must undo its inv_len).  want_grad False
    (plain flavour, no weights): forward only, in passes of 4096 points; grad is None.  ff: layer 0 of flat is a frozen
    sine layer (tests/fourier_model.py; plain flavour, no walls): its 3 H gradient entries are +0.0."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    P = fr.unflatten(np.asarray(flat, dtype=np.float64), 2, 3, L, H)
    N, Re = x.size, 1.0 / float(nu)
    if ff:
        import fourier_model as fo
        assert bc is None and e is None and vis_t is None and want_grad
        r = fo.pde_loss_and_grad(P, x, y, Re, alpha_e=alpha_e, scale=scale, w=w)
        r["grad"] = fo.freeze(r["grad"], H)
        out = r["out"]
        u, v = out[:, 0, 0], out[:, 1, 0]
        lap = (out[:, 0, 3] * scale * scale, out[:, 1, 3] * scale * scale)
    elif not want_grad:
        assert bc is None and e is None and vis_t is None
        out = np.concatenate([fr.forward4(P, x[lo:lo + 4096], y[lo:lo + 4096])[0] for lo in range(0, N, 4096)])
        eqs = fr.residuals(out, Re, None, None, scale)
        ww = np.ones(N) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
        r = dict(eqs=eqs, sums=[float(np.sum(ww * q * q)) for q in eqs], grad=None)
        u, v = out[:, 0, 0], out[:, 1, 0]
        lap = (out[:, 0, 3] * scale * scale, out[:, 1, 3] * scale * scale)
    elif bc is None:
        r = fr.pde_loss_and_grad(P, x, y, Re, alpha_e=alpha_e, vis_t=vis_t, e=e, w=w, scale=scale, eq4_weight=w4)
        out = r["out"]
        u, v = out[:, 0, 0], out[:, 1, 0]
        lap = (out[:, 0, 3] * scale * scale, out[:, 1, 3] * scale * scale)
    else:
        import hardbc_model as hm
        r = hm.constrained_fwdmode(P, bc, x, y, Re, alpha_e=alpha_e, vis_t=vis_t, e=e, w=w, scale=scale, eq4_weight=w4)
        f = r["fields"]
        u, v, lap = f["u"], f["v"], (f["u_d"], f["v_d"])
    eqs, sums = r["eqs"], r["sums"]
    k4 = w4 if len(eqs) == 4 else 0.0
    t = terms(eqs, u, v, lap, w, k4)
    S = float(np.sum(t))
    loss_e = alpha_e * (sums[0] + sums[1] + sums[2] + (k4 * sums[3] if len(eqs) == 4 else 0.0)) / N
    return dict(u=u, v=v, eqs=eqs, lap=lap, sums=sums, loss_e=loss_e, grad=r["grad"], t=t, S=S,
                kappa=float(np.sum(np.abs(t)) / max(abs(S), 1e-300)), dnu=-2.0 * alpha_e * S / N)


def terms(eqs, u, v, lap, w=None, w4=0.0):
    """t_i = w_i ((eq1 + w4 eq4 (u - 1/2)) Lap u + (eq2 + w4 eq4 (v - 1/2)) Lap v)"""
    ww = 1.0 if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    a1, a2 = eqs[0], eqs[1]
    if w4 != 0.0:
        a1 = a1 + w4 * eqs[3] * (u - 0.5)
        a2 = a2 + w4 * eqs[3] * (v - 0.5)
    return ww * (a1 * lap[0] + a2 * lap[1])


# ---- the evaluation rows of tests/test_viscosity_gpu.py (their input conditions: tests/test_viscosity_cpu.py) ----
N_ROW = 69          # a ragged last tile at 16 and at 32 points per tile
ROWS = {
    "2x8-fp32": dict(L=2, H=8, prec="fp32", Re=100.0, re0=40.0, seed=1, names=("fwd_kernel", "bwd_kernel", "dw_kernel")),
    "4x50-fp32-ev": dict(L=4, H=50, prec="fp32", Re=400.0, re0=25.0, seed=2, names=("fwd_kernel", "bwd_kernel", "dw_kernel"),
                         ev=True, weights=True, scale=2.0),
    "6x256-fp32": dict(L=6, H=256, prec="fp32", Re=2000.0, re0=5.0, seed=3,
                       names=("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel")),
    # (pinn_plan_kernel has no fused role: a fused plan reports its forward and reverse roles, so this row and the next
    # assert the same names, and only $PINN_FUSE tells them apart - the fused kernel is what the default launches)
    "6x256-bf16x3-fused": dict(L=6, H=256, prec="bf16x3", Re=2000.0, re0=5.0, seed=3,
                               names=("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")),
    "6x256-bf16x3-unfused": dict(L=6, H=256, prec="bf16x3", Re=2000.0, re0=5.0, seed=3, env=(("PINN_FUSE", "0"),),
                                 names=("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")),
    "6x256-bf16x3-wave8": dict(L=6, H=256, prec="bf16x3", Re=2000.0, re0=5.0, seed=3, env=(("PINN_SCHED", "0"),),
                               names=("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")),
    "3x400-bf16x3-wsplit": dict(L=3, H=400, prec="bf16x3", Re=1.0, re0=0.4, seed=4,
                                names=("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")),
    "4x50-bf16x3-hardbc": dict(L=4, H=50, prec="bf16x3", Re=100.0, re0=40.0, seed=5, hard_bc=True,
                               names=("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")),
}
EV_NET = (4, 40)        # the entropy net of the ev row
ALPHA_EVM = 0.05

# ---- the second set of rows: the families, variants and switches the eight above do not reach ----
# say: what the plan's $PINN_VERBOSE lines must hold - the only proof of the path where rows differ by a switch that
# kernel_names() does not show ($PINN_FUSE: a fused plan reports its forward and reverse roles).  Rows with the same net,
# points, Re and re0 share one fp64 reference (ref_key).  Seeds, Re and re0 were chosen on the fp64 model alone, by the
# conditions of tests/test_viscosity_cpu.py (kappa <= 3 at both estimates; the two estimates more than ten bars apart in
# S, eq1 and the gradient; sine rows: a straight fp32 evaluation within a quarter of each bar): Re = 400, re0 = 25 (the
# ev row's pair) met them for every net, and per net the seed is the first of 1, 2, ... that met them there (at Re the
# viscous term is a few per cent of the rest of eq1, so the earlier seeds of the hard-wall and sine nets cancel in S:
# kappa 3.7 to 38).
_F32 = ("fwd_kernel", "bwd_kernel", "dw_kernel")
_F32W = ("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel")
_B8 = ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")
_B8W = ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel")
_PIPE = ("fwd_pipe_kernel", "bwd_pipe_kernel", "dw_bf16_kernel")
_SPLIT = ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
_WSPLIT = ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")
_HBC1, _FF1 = ("PINN_HBC_SPLIT", "1"), ("PINN_FF_SPLIT", "1")
_HB256 = dict(L=3, H=256, Re=400.0, re0=25.0, seed=5, hard_bc=True)
_HB400 = dict(L=3, H=400, prec="bf16x3", Re=400.0, re0=25.0, seed=4, hard_bc=True)
_FF256 = dict(L=3, H=256, prec="bf16x3", Re=400.0, re0=25.0, seed=3, ff=True)
ROWS.update({
    # the 8-wave wide bf16 sweeps (the select stands behind their prologue's LDS setup): the net and points of the wide
    # role-split row above
    "3x400-bf16x3-wave8": dict(ROWS["3x400-bf16x3-wsplit"], env=(("PINN_WSPLIT", "0"),), names=_B8W),
    # the same family at its register limit, NW = 16 (hidden 512 has no role-split pair: the default)
    "2x512-bf16x3": dict(L=2, H=512, prec="bf16x3", Re=400.0, re0=25.0, seed=1, names=_B8W),
    "3x256-bf16x3-pipe": dict(L=3, H=256, prec="bf16x3", Re=400.0, re0=25.0, seed=1,
                              env=(("PINN_SCHED", "1"),), names=_PIPE, say=("schedule fwd 1 bwd 1",)),
    # hard walls: lap holds the Laplacian after hard_bc_apply
    "2x8-fp32-hardbc": dict(L=2, H=8, prec="fp32", Re=400.0, re0=25.0, seed=4, hard_bc=True, names=_F32,
                            say=("constrained sweeps: 8-wave kernels (PINN_HBC_SPLIT=0)",)),
    "3x256-fp32-hardbc": dict(_HB256, prec="fp32", names=_F32W, say=("constrained sweeps: 8-wave kernels (PINN_HBC_SPLIT=0)",)),
    "3x256-bf16x3-hardbc-fused": dict(_HB256, prec="bf16x3", env=(_HBC1,), names=_SPLIT,
                                      say=("constrained sweeps: fused role-split kernel (PINN_HBC_SPLIT=1)",)),
    "3x256-bf16x3-hardbc-split": dict(_HB256, prec="bf16x3", env=(_HBC1, ("PINN_FUSE", "0")), names=_SPLIT,
                                      say=("constrained sweeps: role-split kernels, two launches (PINN_HBC_SPLIT=1)",)),
    "3x400-bf16x3-hardbc-wsplit": dict(_HB400, env=(_HBC1,), names=_WSPLIT,
                                       say=("constrained sweeps: wide role-split kernels (PINN_HBC_SPLIT=1)",)),
    "3x400-bf16x3-hardbc-wave8": dict(_HB400, env=(("PINN_WSPLIT", "0"),), names=_B8W,
                                      say=("constrained sweeps: 8-wave kernels (PINN_HBC_SPLIT=0)",)),
    # the frozen sine first layer (frequencies: sigma = 2, tests/test_fourier_gpu.py)
    "2x8-fp32-ff": dict(L=2, H=8, prec="fp32", Re=400.0, re0=25.0, seed=3, ff=True, names=_F32,
                        say=("frozen sine first layer: 8-wave kernels",)),
    "3x256-bf16x3-ff": dict(_FF256, names=_B8, say=("frozen sine first layer: 8-wave kernels",)),
    "3x256-bf16x3-ff-fused": dict(_FF256, env=(_FF1,), names=_SPLIT,
                                  say=("frozen sine sweeps: fused role-split kernel (PINN_FF_SPLIT=1)",)),
    "3x256-bf16x3-ff-split": dict(_FF256, env=(_FF1, ("PINN_FUSE", "0")), names=_SPLIT,
                                  say=("frozen sine sweeps: role-split kernels, two launches (PINN_FF_SPLIT=1)",)),
    "3x400-bf16x3-ff-wsplit": dict(L=3, H=400, prec="bf16x3", Re=400.0, re0=25.0, seed=5, ff=True,
                                   env=(_FF1,), names=_WSPLIT, say=("frozen sine sweeps: wide role-split kernels (PINN_FF_SPLIT=1)",)),
    # w4 != 0 together with vis_t, weights and coord_scale = 2 on a bf16x3 family (the entropy net runs bf16x3, too)
    "4x50-bf16x3-ev": dict(L=4, H=50, prec="bf16x3", Re=400.0, re0=25.0, seed=1, ev=True, weights=True,
                           scale=2.0, names=_B8),
})
FF_SIGMA = 2.0
# plain bf16 (TERMS = 1): judged bit for bit only (tests/test_viscosity_gpu.py, device nu against the launch constant,
# and the lap plane from two viscosities) - the suite has no fp64 bar for plain bf16 at these shapes
BIT_ROWS = {
    "3x256-bf16-fused": dict(L=3, H=256, prec="bf16", Re=2000.0, re0=5.0, seed=3, names=_SPLIT),
    "3x256-bf16-unfused": dict(L=3, H=256, prec="bf16", Re=2000.0, re0=5.0, seed=3, env=(("PINN_FUSE", "0"),), names=_SPLIT),
    "3x400-bf16-wsplit": dict(L=3, H=400, prec="bf16", Re=1.0, re0=0.4, seed=4, names=_WSPLIT),
}


# the lap plane from two viscosities: two estimates whose fp32 reciprocals are a power of two apart (nu_a = 2 nu_b, both
# exact), on the plain-bf16 rows, one hard-wall row and one sine row
TWO_RE0 = (32.0, 64.0)
LAP_ROWS = tuple(BIT_ROWS) + ("3x256-bf16x3-hardbc-fused", "3x256-bf16x3-ff-fused")
# the engine's options with the scalar on: the 2x8 fp32 net at N_OPT collocation points, batches of B_OPT (no multiple
# of 16), a pool of N_POOL candidates
N_OPT, B_OPT, N_POOL = 203, 75, 301


def pool_points(n=N_POOL):
    """The candidate points of the resampling-pool test (fp32)."""
    rng = np.random.RandomState(77)
    return rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)


def ref_key(name):
    """What a row's fp64 reference depends on: rows that differ only in precision, switches and kernels share it."""
    r = dict(BIT_ROWS, **ROWS)[name]
    return tuple(r.get(k) for k in ("L", "H", "seed", "Re", "re0", "hard_bc", "ff", "ev", "weights", "scale"))


def row_case(name, n=N_ROW):
    """The inputs of a row: flat (fp32), x, y (fp32), w (fp32 or None), scale, Re and, ev row, flat_e; sine row: B, the
    frequencies [H / 2, 2], and flat carries their embedding as layer 0."""
    from oracle import autograd_ref as ar
    r = dict(BIT_ROWS, **ROWS)[name]
    rng = np.random.RandomState(100 + r["seed"])
    lo, hi = (-1.0, 1.0) if r.get("scale", 1.0) != 1.0 else (0.0, 1.0)
    x = (lo + (hi - lo) * rng.rand(n)).astype(np.float32)
    y = (lo + (hi - lo) * rng.rand(n)).astype(np.float32)
    w = (0.3 + rng.rand(n)).astype(np.float32) if r.get("weights") else None
    flat = ar.flat_params(ar.seeded_net(3, r["L"], r["H"], seed=r["seed"])).numpy().copy()
    flat_e = ar.flat_params(ar.seeded_net(1, *EV_NET, seed=r["seed"] + 50)).numpy().copy() if r.get("ev") else None
    B = None
    if r.get("ff"):
        import fourier_model as fo
        B = FF_SIGMA * np.random.RandomState(7 + r["H"] + r["seed"]).randn(r["H"] // 2, 2)
        flat = fo.with_first_layer(flat, r["H"], B)
    return dict(r, name=name, flat=flat, x=x, y=y, w=w, scale=r.get("scale", 1.0), flat_e=flat_e, B=B)


def row_re0(c, shifted):
    """The starting estimate a row's evaluation is made at: the configured Re, or (shifted) the row's re0 - far enough
    from Re for the viscous term to tell them apart (tests/test_viscosity_cpu.py), so that a kernel which keeps the
    launch constant 1 / Re, in all or in some of its tiles, misses the model."""
    return c["re0"] if shifted else c["Re"]


def row_reference(c, vis_t=None, re0=None, **over):
    """evaluate() of a row at nu = fp32(1 / re0) (re0 None: the configured Re; vis_t0 = 20 / Re keeps the configured
    one).  ev row: e from the fp64 entropy net; vis_t as given (the GPU test hands in the plane the device used) or
    min(20 / Re, alpha_evm |e|).  over: overrides (w=None, scale=1.0 ... for the
    controls)."""
    nu = float(np.float32(1.0) / np.float32(c["Re"] if re0 is None else re0))
    kw = dict(w=c["w"], scale=c["scale"])
    if c.get("ev"):
        Pe = fr.unflatten(c["flat_e"].astype(np.float64), 2, 1, *EV_NET)
        e = fr.forward1(Pe, c["x"].astype(np.float64), c["y"].astype(np.float64))[0][:, 0]
        kw.update(e=e, vis_t=np.minimum(20.0 / c["Re"], ALPHA_EVM * np.abs(e)) if vis_t is None else vis_t)
    if c.get("hard_bc"):
        import hardbc_model as hm
        kw["bc"] = hm.HardBc()
    if c.get("ff"):
        kw["ff"] = True
    kw.update(over)
    return evaluate(c["flat"], c["L"], c["H"], c["x"], c["y"], nu, **kw)


# ---- pinn_visc_update, one rounding per operation as the header lists them ----
def new_state(re0):
    """(state, nu32) of an optimiser that has made no update: nu32 = fp32(1) / fp32(re0), theta = ln nu32."""
    nu = np.float32(1.0) / np.float32(re0)
    return np.array([math.log(float(nu)), 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0]), nu


def update(state, nu32, s32, coef, lr, beta1=0.9, beta2=0.999, eps=1e-8, theta_min=-math.inf, theta_max=math.inf):
    """The state after one pinn_visc_update on the fp32 sum s32 at the fp32 viscosity nu32 (in place), and the new
    fp32 nu - float32(exp(theta)) by numpy's exp, which the device's may differ from by an fp32 ulp."""
    f = np.float64
    s = f(np.float32(s32))
    if not np.isfinite(s):
        state[7] += 1.0
        return state, np.float32(nu32)
    G = f(coef) * s
    g = f(np.float32(nu32)) * G
    p1, p2 = f(state[3]) * f(beta1), f(state[4]) * f(beta2)
    c1, c2 = f(1.0) - f(beta1), f(1.0) - f(beta2)
    m = f(beta1) * f(state[1]) + c1 * g
    v = f(beta2) * f(state[2]) + (c2 * g) * g
    bc1, bc2 = f(1.0) - p1, f(1.0) - p2
    step = f(lr) / bc1
    denom = np.sqrt(v) / np.sqrt(bc2) + f(eps)
    theta = f(state[0]) - step * (m / denom)
    theta = f(theta_min) if theta < theta_min else theta
    theta = f(theta_max) if theta > theta_max else theta
    state[0], state[1], state[2], state[3], state[4] = theta, m, v, p1, p2
    state[5] += 1.0
    state[6] = G
    return state, np.float32(np.exp(theta))


# ---- Kovasznay flow ----
def kovasznay(x, y, Re=40.0):
    """The exact (u, v, p) of Kovasznay (1948) at Reynolds number Re."""
    lam = Re / 2.0 - math.sqrt(Re * Re / 4.0 + 4.0 * math.pi ** 2)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ex = np.exp(lam * x)
    return (1.0 - ex * np.cos(2.0 * math.pi * y), lam / (2.0 * math.pi) * ex * np.sin(2.0 * math.pi * y),
            0.5 * (1.0 - np.exp(2.0 * lam * x)))


# the identification run of tests/test_viscosity_gpu.py and of --write
KOV = dict(Re=40.0, re0=10.0, L=4, H=50, n_f=1000, n_s=300, n_b=260, alpha_e=1.0, alpha_b=10.0, alpha_s=10.0,
           lr=1e-3, lr_nu=1e-2, updates=2000, every=100, box=((-0.5, 1.0), (-0.5, 1.5)), seed=0)


def kovasznay_case(seed=None):
    """The points (fp32, what the engine is given), the exact data at them and the initial parameters of the run."""
    from oracle import autograd_ref as ar
    k = KOV
    seed = k["seed"] if seed is None else seed
    rng = np.random.RandomState(1000 + seed)
    (x0, x1), (y0, y1) = k["box"]
    pts = lambda n: ((x0 + (x1 - x0) * rng.rand(n)).astype(np.float32), (y0 + (y1 - y0) * rng.rand(n)).astype(np.float32))
    xf, yf = pts(k["n_f"])
    xs, ys = pts(k["n_s"])
    q = k["n_b"] // 4
    s = rng.rand(4, q)
    xb = np.concatenate([x0 + (x1 - x0) * s[0], x0 + (x1 - x0) * s[1], np.full(q, x0), np.full(q, x1)]).astype(np.float32)
    yb = np.concatenate([np.full(q, y0), np.full(q, y1), y0 + (y1 - y0) * s[2], y0 + (y1 - y0) * s[3]]).astype(np.float32)
    us, vs, ps = kovasznay(xs, ys, k["Re"])
    ub, vb, _ = kovasznay(xb, yb, k["Re"])
    flat = ar.flat_params(ar.seeded_net(3, k["L"], k["H"], seed=seed)).numpy().astype(np.float32)
    f32 = lambda a: a.astype(np.float32)
    return dict(xf=xf, yf=yf, xs=xs, ys=ys, us=f32(us), vs=f32(vs), ps=f32(ps), xb=xb, yb=yb, ub=f32(ub), vb=f32(vb),
                flat=flat)


def kovasznay_model(case, updates=None, every=None):
    """The run in fp64: Adam on the net (oracle adam_step) and the update above on theta, the viscosity carried as the
    fp32 the kernels would read.  Returns Re after every `every` updates."""
    k = KOV
    updates = k["updates"] if updates is None else updates
    every = k["every"] if every is None else every
    d = lambda a: np.asarray(a, dtype=np.float64)
    L, H, N = k["L"], k["H"], k["n_f"]
    p = d(case["flat"])
    m, v = np.zeros_like(p), np.zeros_like(p)
    st, nu = new_state(k["re0"])
    out = []
    for t in range(1, updates + 1):
        P = fr.unflatten(p, 2, 3, L, H)
        r = evaluate(p, L, H, case["xf"], case["yf"], float(nu), alpha_e=k["alpha_e"])
        b = fr.bc_loss_and_grad(P, d(case["xb"]), d(case["yb"]), d(case["ub"]), d(case["vb"]), alpha_b=k["alpha_b"])
        cs = 2.0 * k["alpha_s"] / k["n_s"]
        s = fr.value_loss_and_grad_chunked(P, case["xs"], case["ys"], targets=[case["us"], case["vs"], case["ps"]],
                                           coef=[cs, cs, cs])
        g = r["grad"] + b["grad"] + s["grad"]
        p, m, v = fr.adam_step(p, g, m, v, t, k["lr"])
        st, nu = update(st, nu, np.float32(r["S"]), -2.0 * k["alpha_e"] / N, k["lr_nu"])
        if t % every == 0:
            out.append(1.0 / float(nu))
    return np.array(out)


if __name__ == "__main__":
    if "--write" in sys.argv:
        for seed in range(5):       # the first seed whose fp64 run ends within 2.5 % of Re
            tr = kovasznay_model(kovasznay_case(seed))
            err = abs(tr[-1] - KOV["Re"]) / KOV["Re"]
            print("seed %d: Re after %d updates %.4f (%.2f %%)" % (seed, KOV["updates"], tr[-1], 100.0 * err), flush=True)
            if err <= 0.025:
                os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
                np.savez(GOLDEN, re=tr, seed=np.array(seed), every=np.array(KOV["every"]))
                print("wrote", GOLDEN)
                break
        else:
            sys.exit("no seed of 0..4 met the 2.5 % condition")
