"""numpy statement of the Reynolds-number continuation (csrc/visc_sched.h / visc_sched.hip,
PinnEngine.set_reynolds_continuation; TEST INFRASTRUCTURE): the schedule of include/nsfnet_pinn.h operation by
operation, the record the step launch leaves, and the ev cases of the GPU rows with the fp64 oracle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = dict(geometric=0, linear_re=1, linear_nu=2)
RECORD = 6      # PINN_RAMP_RECORD: t, s, Re_t, nu_t, cap_t, done


def schedule(re_start, re_end, updates, hold=0, shape="geometric", stairs=0, cap_factor=0.0):
    """The constants of a ramp as the engine forms them: the fp32 ends are what the residual launches make of their
    constants, 1.0f / (float)Re and (float)(cap_factor / Re)."""
    f32 = np.float32
    return dict(shape=shape, stairs=int(stairs), hold=int(hold), updates=int(updates), re_start=float(re_start),
                re_end=float(re_end), cap_factor=float(cap_factor),
                nu_start=f32(1.0) / f32(re_start), nu_end=f32(1.0) / f32(re_end),
                cap_start=f32(cap_factor / re_start) if cap_factor > 0.0 else f32(0.0),
                cap_end=f32(cap_factor / re_end) if cap_factor > 0.0 else f32(0.0))


def value(c, t):
    """The record [t, s, Re_t, nu_t, cap_t, done] of position t: fp64, one rounding per operation in the header's
    order, nu_t and cap_t rounded once to fp32; the ends selected."""
    f = np.float64
    d = int(t) - c["hold"]
    s = f(0.0) if d <= 0 else f(1.0) if d >= c["updates"] else f(d) / f(c["updates"])
    if c["stairs"] > 0 and s < 1.0:
        k = f(c["stairs"])
        s = np.floor(s * k) / k
    with_cap = c["cap_factor"] > 0.0
    done = 1.0 if s >= 1.0 else 0.0
    if s <= 0.0:
        return [float(t), float(s), c["re_start"], float(c["nu_start"]), float(c["cap_start"]) if with_cap else 0.0, done]
    if s >= 1.0:
        return [float(t), float(s), c["re_end"], float(c["nu_end"]), float(c["cap_end"]) if with_cap else 0.0, done]
    n0, n1 = f(c["nu_start"]), f(c["nu_end"])
    if c["shape"] == "linear_re":
        r0, r1 = f(1.0) / n0, f(1.0) / n1
        nu = f(1.0) / (r0 + s * (r1 - r0))
    elif c["shape"] == "linear_nu":
        nu = n0 + s * (n1 - n0)
    else:
        l0, l1 = np.log(n0), np.log(n1)
        nu = np.exp(l0 + s * (l1 - l0))
    nu = min(max(nu, min(n0, n1)), max(n0, n1))
    cap = 0.0
    if with_cap:
        c0, c1 = f(c["cap_start"]), f(c["cap_end"])
        cap = float(np.float32(min(max(f(c["cap_factor"]) * nu, min(c0, c1)), max(c0, c1))))
    return [float(t), float(s), float(f(1.0) / nu), float(np.float32(nu)), cap, done]


def positions(c):
    """The positions the schedule is judged at: 0, hold, hold + 1, the middle, the last ramp update, the end, 3e9."""
    h, u = c["hold"], c["updates"]
    return [0, h, h + 1, h + u // 2, h + u - 1, h + u, 3_000_000_000]


# ---- the ev rows of tests/test_recont_gpu.py ----
# One row per forward family that reads the cap (the fused kernel and its two-launch form included): an engine at Re
# with re_start = R0 against a plain engine at Re = R0.  alpha_evm is chosen so that at the start the cap binds at part
# of the points; the seed is the first of 1, 2, ... for which both groups hold a quarter of the points
# (tests/test_recont_cpu.py asserts the conditions with the fp64 oracle).
N_ROW = 69
EV_NET = (4, 40)
EV_RE, EV_R0, EV_FACTOR = 400.0, 25.0, 20.0
_F32 = ("fwd_kernel", "bwd_kernel", "dw_kernel")
_F32W = ("fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel")
_B8 = ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")
_B8W = ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel")
_PIPE = ("fwd_pipe_kernel", "bwd_pipe_kernel", "dw_bf16_kernel")
_SPLIT = ("fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel")
_WSPLIT = ("fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel")
EV_ROWS = {
    "ev-4x50-fp32": dict(L=4, H=50, prec="fp32", names=_F32),
    "ev-3x256-fp32": dict(L=3, H=256, prec="fp32", names=_F32W),
    "ev-4x50-bf16x3": dict(L=4, H=50, prec="bf16x3", names=_B8),
    "ev-3x400-bf16x3-wave8": dict(L=3, H=400, prec="bf16x3", env=(("PINN_WSPLIT", "0"),), names=_B8W),
    "ev-3x256-bf16x3-pipe": dict(L=3, H=256, prec="bf16x3", env=(("PINN_SCHED", "1"),), names=_PIPE),
    "ev-3x256-bf16x3-fused": dict(L=3, H=256, prec="bf16x3", names=_SPLIT),
    "ev-3x256-bf16x3-unfused": dict(L=3, H=256, prec="bf16x3", env=(("PINN_FUSE", "0"),), names=_SPLIT),
    "ev-3x400-bf16x3-wsplit": dict(L=3, H=400, prec="bf16x3", names=_WSPLIT),
}
MAX_SEED = 8
MARGIN = 2e-3           # no alpha_evm |e| closer to the cap at R0 than this, relative: four bf16x3 plane bars


def ev_case(name, seed):
    """The inputs of an ev row for a seed: flat, flat_e (fp32), x, y, w (fp32), and alpha_evm = the cap at the start
    over the middle of the sorted |e|: about half the points then sit on either side of the cap at R0."""
    from oracle import autograd_ref as ar
    from oracle import fwdmode_ref as fr
    r = EV_ROWS[name]
    rng = np.random.RandomState(300 + seed)
    x, y = rng.rand(N_ROW).astype(np.float32), rng.rand(N_ROW).astype(np.float32)
    w = (0.3 + rng.rand(N_ROW)).astype(np.float32)
    flat = ar.flat_params(ar.seeded_net(3, r["L"], r["H"], seed=seed)).numpy().copy()
    flat_e = ar.flat_params(ar.seeded_net(1, *EV_NET, seed=seed + 50)).numpy().copy()
    Pe = fr.unflatten(flat_e.astype(np.float64), 2, 1, *EV_NET)
    e = fr.forward1(Pe, x.astype(np.float64), y.astype(np.float64))[0][:, 0]
    a = np.sort(np.abs(e))
    # the threshold goes into the widest gap between two neighbours of the sorted |e| that leaves a quarter of the
    # points on either side: no |e| sits on it
    q = N_ROW // 4 + 1
    i = q + int(np.argmax(a[q + 1:N_ROW - q] / a[q:N_ROW - q - 1]))
    mid = float(np.sqrt(a[i] * a[i + 1]))
    alpha_evm = float(np.float32(EV_FACTOR / EV_R0 / mid))
    return dict(r, name=name, seed=seed, flat=flat, flat_e=flat_e, x=x, y=y, w=w, e=e, alpha_evm=alpha_evm,
                Re=EV_RE, R0=EV_R0, ev=True, scale=1.0)


def ev_reference(c, Re=None, nu=None, cap=None):
    """The fp64 evaluation of an ev case at Reynolds number Re with its cap EV_FACTOR / Re (or at the fp32 pair nu, cap
    of a position inside the ramp): dict(vis_t, vtm, cap, binds, eqs, sums, grad, loss_e) - binds: the points where the
    cap, not alpha_evm |e|, is the artificial viscosity."""
    from oracle import fwdmode_ref as fr
    cap = np.float64(np.float32(EV_FACTOR / Re)) if cap is None else np.float64(cap)
    nu = float(np.float32(1.0) / np.float32(Re)) if nu is None else float(nu)
    vtm = (np.float32(c["alpha_evm"]) * np.abs(c["e"]).astype(np.float32)).astype(np.float64)
    vis_t = np.minimum(cap, vtm)
    P = fr.unflatten(c["flat"].astype(np.float64), 2, 3, c["L"], c["H"])
    r = fr.pde_loss_and_grad(P, c["x"].astype(np.float64), c["y"].astype(np.float64), 1.0 / nu, alpha_e=1.0, vis_t=vis_t,
                             e=c["e"], w=c["w"].astype(np.float64), scale=1.0, eq4_weight=0.1)
    s = r["sums"]
    return dict(vis_t=vis_t, vtm=vtm, cap=float(cap), binds=vtm >= cap, eqs=r["eqs"], sums=s, grad=r["grad"],
                loss_e=(s[0] + s[1] + s[2] + 0.1 * s[3]) / c["x"].size)


def ev_seed(name):
    """The first seed of 1, 2, ... at which the cap at R0 binds at a quarter of the points at least, leaves a quarter
    free and has no point within MARGIN of it (None: none up to MAX_SEED)."""
    for seed in range(1, MAX_SEED + 1):
        c = ev_case(name, seed)
        cap = np.float64(np.float32(EV_FACTOR / c["R0"]))
        vtm = (np.float32(c["alpha_evm"]) * np.abs(c["e"]).astype(np.float32)).astype(np.float64)      # (ev_reference's)
        b = vtm >= cap
        if min(b.sum(), (~b).sum()) >= N_ROW / 4.0 and (np.abs(vtm - cap) > MARGIN * cap).all():
            return seed
    return None
