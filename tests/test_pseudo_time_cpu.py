"""Pseudo-time stepping of the residual loss, without a device: the fp64 model's gradient against
central differences of its loss, the fixed point at u = u*, the refresh cadence of the advance model, what the C ABI
refuses and how it resolves a pseudo-time plan, and the argument checks, refusals and cadence of the engine and the
solvers on the CPU stand-ins."""
import ctypes

import numpy as np
import pytest
import torch

import hardbc_model as hm
import ptime_model as pm
from oracle import autograd_ref as ar
from oracle import fwdmode_ref as fr


def _flat(n_out, L, H, seed):
    return ar.flat_params(ar.seeded_net(n_out, L, H, seed=seed)).numpy().astype(np.float64)


def _anchor_of(L, H, seed, x, y, bc=None, scale=1.0):
    """Anchors [3, N]: the fields of an independently seeded net of the same shape."""
    P = fr.unflatten(_flat(3, L, H, seed), 2, 3, L, H)
    f = pm.residual_term(P, x, y, 100.0, np.zeros((3, len(x))), 0.0, 0.0, bc=bc, scale=scale)["fields"]
    return np.stack([f["u"], f["v"], f["p"]])


# ---- the model's gradient against central differences of its loss, fp64 ----
@pytest.mark.parametrize("case", ["plain", "ev", "hard_walls"])
def test_model_gradient_equals_central_differences(case):
    L, H, N, Re = 2, 8, 37, 400.0
    rng = np.random.RandomState(3)
    flat = _flat(3, L, H, 11)
    kw, bc, scale, lo = {}, None, 1.0, 0.0
    if case == "ev":      # e, w and the lagged viscosity are constants of the loss
        kw = dict(e=0.3 * rng.randn(N), w=0.3 + rng.rand(N), vis_t=0.01 * rng.rand(N))
    if case == "hard_walls":
        bc, scale, lo = hm.HardBc(lift_power=3, origin=(-1.0, -1.0), inv_len=0.5), 2.0, -1.0
    x, y = lo + (1.0 - lo) * rng.rand(N), lo + (1.0 - lo) * rng.rand(N)
    anchor = _anchor_of(L, H, 12, x, y, bc, scale)
    sigma, sigma_p = 0.7, 0.3

    def term(p):
        return pm.residual_term(fr.unflatten(p, 2, 3, L, H), x, y, Re, anchor, sigma, sigma_p, alpha_e=1.5, bc=bc,
                                scale=scale, **kw)

    r = term(flat)
    assert np.abs(np.asarray(r["sums"][:3]) - np.asarray(r["steady_sums"])).max() > 1e-3     # the terms carry weight
    h = 1e-6
    fd = np.array([(term(flat + h * d)["loss_e"] - term(flat - h * d)["loss_e"]) / (2.0 * h) for d in np.eye(flat.size)])
    rel = np.linalg.norm(fd - r["grad"]) / np.linalg.norm(r["grad"])
    print("%s: gradient against central differences, rel-L2 = %.3e" % (case, rel))
    assert rel < 1e-8


def test_model_with_zero_rates_is_the_steady_oracle():
    L, H, N = 3, 10, 50
    rng = np.random.RandomState(0)
    x, y, P = rng.rand(N), rng.rand(N), fr.unflatten(_flat(3, L, H, 2), 2, 3, L, H)
    e, w = rng.randn(N), 0.5 + rng.rand(N)
    r = pm.residual_term(P, x, y, 100.0, rng.randn(3, N), 0.0, 0.0, alpha_e=2.0, e=e, w=w)
    ref = fr.pde_loss_and_grad(P, x, y, 100.0, alpha_e=2.0, e=e, w=w)
    np.testing.assert_array_equal(r["grad"], ref["grad"])
    np.testing.assert_array_equal(r["sums"], ref["sums"])


# ---- the fixed point, and the advance model ----
def _planes(L, H, seed, x, y, npad):
    """fp32 field planes [FLD_COUNT, npad] of a seeded net at the points (what an evaluation leaves)."""
    P = fr.unflatten(_flat(3, L, H, seed), 2, 3, L, H)
    r = pm.residual_term(P, x, y, 100.0, np.zeros((3, len(x))), 0.0, 0.0)
    fld = np.zeros((pm.FLD_COUNT, npad), dtype=np.float32)
    n = len(x)
    for k, v in ((pm.FLD_U, r["fields"]["u"]), (pm.FLD_V, r["fields"]["v"]), (pm.FLD_P, r["fields"]["p"]),
                 (pm.FLD_EQ1, r["eqs"][0]), (pm.FLD_EQ2, r["eqs"][1]), (pm.FLD_EQ3, r["eqs"][2])):
        fld[k, :n] = v
    return fld


def test_forced_advance_then_reevaluation_has_no_drift_and_the_steady_loss():
    L, H, N, npad = 2, 8, 37, 64
    rng = np.random.RandomState(5)
    x, y = rng.rand(N), rng.rand(N)
    w = (0.5 + rng.rand(N)).astype(np.float32)
    fld = _planes(L, H, 4, x, y, npad)
    anchor, rec = pm.advance(fld, N, rng.randn(3, npad).astype(np.float32), every=0, force=True, w=w)
    assert rec[pm.R_DRIFT_UV] > 0.0 and rec[pm.R_MAX] > 0.0 and rec[pm.R_SINCE] == 0.0 and rec[pm.R_REFRESHES] == 1.0
    np.testing.assert_array_equal(anchor[:, :40], fld[[pm.FLD_U, pm.FLD_V, pm.FLD_P], :40])      # whole quads past n = 37
    # the same weights evaluated again: the planes are the same, the next (unforced) advance sees no drift at all
    anchor2, rec2 = pm.advance(fld, N, anchor, every=0, force=False, w=w, record=rec)
    assert rec2[pm.R_DRIFT_UV] == 0.0 and rec2[pm.R_DRIFT_P] == 0.0 and rec2[pm.R_MAX] == 0.0
    assert rec2[pm.R_SINCE] == 1.0 and rec2[pm.R_REFRESHES] == 1.0
    np.testing.assert_array_equal(anchor2, anchor)
    # ... and the minimised term is the steady one, bit for bit, at any rates
    P = fr.unflatten(_flat(3, L, H, 4), 2, 3, L, H)
    own = _anchor_of(L, H, 4, x, y)
    r = pm.residual_term(P, x, y, 100.0, own, 123.0, 45.0, w=w)
    s = pm.residual_term(P, x, y, 100.0, own, 0.0, 0.0, w=w)
    assert r["sums"] == r["steady_sums"] == s["sums"] and r["loss_e"] == s["loss_e"]
    np.testing.assert_array_equal(r["grad"].shape, s["grad"].shape)


@pytest.mark.parametrize("every", [1, 3, 4])
def test_refresh_fires_on_exactly_every_nth_update(every):
    L, H, N, npad = 2, 8, 21, 32
    rng = np.random.RandomState(6)
    x, y = rng.rand(N), rng.rand(N)
    anchor, rec = rng.randn(3, npad).astype(np.float32), None
    fired = []
    for t in range(1, 11):
        fld = _planes(L, H, 20 + t, x, y, npad)         # the field moves with every update
        before = anchor.copy()
        anchor, rec = pm.advance(fld, N, anchor, every=every, record=rec)
        refreshed = not np.array_equal(anchor, before)
        assert refreshed == (t % every == 0)
        if refreshed:
            fired.append(t)
            np.testing.assert_array_equal(anchor[:, :N], fld[[pm.FLD_U, pm.FLD_V, pm.FLD_P], :N])
        assert rec[pm.R_SINCE] == t % every and rec[pm.R_REFRESHES] == len(fired)
    assert fired == list(range(every, 11, every))
    # every = 0: never by the cadence
    _, rec = pm.advance(fld, N, anchor, every=0, record=rec)
    assert rec[pm.R_REFRESHES] == len(fired)


def test_advance_model_propagates_a_nan_and_folds_like_a_plain_sum():
    N, npad = 5000, 5024
    rng = np.random.RandomState(8)
    fld = rng.randn(pm.FLD_COUNT, npad).astype(np.float32)
    anchor = rng.randn(3, npad).astype(np.float32)
    w = (0.5 + rng.rand(N)).astype(np.float32)
    _, rec = pm.advance(fld, N, anchor, every=0, w=w)
    q = fld[:, :N].astype(np.float64)
    a = anchor[:, :N].astype(np.float64)
    want = [np.sum(w * q[pm.FLD_EQ1] ** 2), np.sum(w * q[pm.FLD_EQ2] ** 2), np.sum(w * q[pm.FLD_EQ3] ** 2),
            np.sum(w * ((q[pm.FLD_U] - a[0]) ** 2 + (q[pm.FLD_V] - a[1]) ** 2)), np.sum(w * (q[pm.FLD_P] - a[2]) ** 2)]
    np.testing.assert_allclose(rec[:5], want, rtol=1e-13)
    assert rec[pm.R_MAX] == max(np.abs(q[pm.FLD_U] - a[0]).max(), np.abs(q[pm.FLD_V] - a[1]).max())
    fld[pm.FLD_U, 4321] = np.nan
    _, rec = pm.advance(fld, N, anchor, every=0, w=w)
    assert np.isnan(rec[pm.R_MAX]) and np.isnan(rec[pm.R_DRIFT_UV]) and np.isfinite(rec[pm.R_DRIFT_P])


# ---- the C ABI: plan creation and the refusals work without a device ----
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def _net(lib, n_out, L, H, prec=(0, 0, 0)):
    from nsfnet_amd import _lib
    h = ctypes.c_void_p()
    _lib.check(lib.pinn_net_create(n_out, L, H, ctypes.byref(h)), "pinn_net_create")
    _lib.check(lib.pinn_net_set_precision(h, *prec), "pinn_net_set_precision")
    return h


def _create(lib, net, n, bc=None):
    h = ctypes.c_void_p()
    rc = lib.pinn_plan_create_pseudo_time(net, n, None if bc is None else ctypes.byref(bc), ctypes.byref(h))
    return rc, h, lib.pinn_last_error().decode()


def _names(lib, plan):
    return tuple((lib.pinn_plan_kernel(plan, k) or b"").decode() for k in range(3))


def test_abi_keeps_its_version_and_exports_the_new_symbols(lib):
    assert lib.pinn_abi_version() == 3
    for name in ("pinn_plan_create_pseudo_time", "pinn_plan_set_pseudo_time", "pinn_plan_pseudo_time",
                 "pinn_ptime_scratch_bytes", "pinn_ptime_advance"):
        assert hasattr(lib, name)


def test_abi_plan_entry_points_refuse_bad_arguments(lib):
    from nsfnet_amd import _lib
    net = _net(lib, 3, 2, 16)
    rc, plan, err = _create(lib, net, 100)
    assert rc == 0, err
    a16 = ctypes.c_void_p(4096)            # never dereferenced: the plan only keeps the address
    s, sp = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    assert lib.pinn_plan_pseudo_time(plan, ctypes.byref(s), ctypes.byref(sp)) == 0 and (s.value, sp.value) == (0.0, 0.0)
    for sig, sigp, anchor, text in ((-0.5, 0.0, a16, "sigma"), (1.0, -1e-3, a16, "sigma"), (float("nan"), 0.0, a16, "sigma"),
                                    (1.0, float("inf"), a16, "sigma"), (1.0, 0.0, None, "anchor"),
                                    (1.0, 0.0, ctypes.c_void_p(4100), "aligned")):
        rc = lib.pinn_plan_set_pseudo_time(plan, anchor, sig, sigp)
        assert rc != 0 and text in lib.pinn_last_error().decode(), (sig, sigp, anchor)
    # a residual call before the anchors are set is refused, in all three entry points
    one = ctypes.c_void_p(256)
    coef = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 0.0)
    rc = lib.pinn_residual_forward(plan, one, one, one, one, None, None, None, None, one, 100.0, 0.0, 0.0, 1.0, 0, None, None)
    assert rc != 0 and "anchors are unset" in lib.pinn_last_error().decode()
    rc = lib.pinn_residual_backward(plan, one, one, one, one, None, None, None, one, coef, 100.0, 1.0, None, None)
    assert rc != 0 and "anchors are unset" in lib.pinn_last_error().decode()
    rc = lib.pinn_residual_forward_backward(plan, one, one, one, one, None, None, None, None, one, coef, 100.0, 0.0, 0.0,
                                            1.0, None, None, None)
    assert rc != 0 and "anchors are unset" in lib.pinn_last_error().decode()
    assert lib.pinn_plan_set_pseudo_time(plan, a16, 0.75, 0.25) == 0
    assert lib.pinn_plan_pseudo_time(plan, ctypes.byref(s), ctypes.byref(sp)) == 0 and (s.value, sp.value) == (0.75, 0.25)
    assert lib.pinn_plan_set_pseudo_time(plan, a16, 0.0, 0.0) == 0          # zero rates are allowed
    # any other plan refuses both calls
    plain = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 100, 4, ctypes.byref(plain)) == 0
    assert lib.pinn_plan_set_pseudo_time(plain, a16, 1.0, 0.0) != 0 and "not a pseudo-time plan" in lib.pinn_last_error().decode()
    assert lib.pinn_plan_pseudo_time(plain, ctypes.byref(s), ctypes.byref(sp)) != 0
    assert lib.pinn_plan_set_pseudo_time(None, a16, 1.0, 0.0) != 0
    # an entropy net has no pseudo-time term; a bad wall descriptor is refused as on a constrained plan
    net_e = _net(lib, 1, 2, 16)
    rc, _, err = _create(lib, net_e, 100)
    assert rc != 0 and "n_out" in err
    rc, _, err = _create(lib, net, 100, _lib.HardBcStruct(1, 9, 0.0, 0.0, 1.0, 10.0))
    assert rc != 0 and "lift_power" in err
    rc, _, err = _create(lib, net, 0)
    assert rc != 0 and "point count" in err
    # walls and pseudo-time together: the plan carries both
    rc, both, err = _create(lib, net, 100, _lib.HardBcStruct(1, 3, 0.0, 0.0, 1.0, 10.0))
    assert rc == 0, err
    got = _lib.HardBcStruct()
    assert lib.pinn_plan_hard_bc(both, ctypes.byref(got)) == 0 and (got.kind, got.lift_power) == (1, 3)
    assert lib.pinn_plan_pseudo_time(both, ctypes.byref(s), ctypes.byref(sp)) == 0
    for p in (plan, plain, both):
        lib.pinn_plan_destroy(p)
    lib.pinn_net_destroy(net); lib.pinn_net_destroy(net_e)


def test_abi_advance_refuses_bad_arguments(lib):
    assert lib.pinn_ptime_scratch_bytes(0) == -1 and lib.pinn_ptime_scratch_bytes((1 << 30) + 1) == -1
    assert lib.pinn_ptime_scratch_bytes(1) > 0 and lib.pinn_ptime_scratch_bytes(1) % 8 == 0
    p = ctypes.c_void_p(4096)
    ok = dict(n=100, fields=p, npad=128, w=None, anchor=p, every=3, force=0, scratch=p, record=p)
    call = lambda **kw: lib.pinn_ptime_advance(*[dict(ok, **kw)[k] for k in ("n", "fields", "npad", "w", "anchor", "every",
                                                                             "force", "scratch", "record")], None)
    for kw, text in ((dict(n=0), "n must be"), (dict(n=(1 << 30) + 1), "n must be"), (dict(fields=None), "null"),
                     (dict(anchor=None), "null"), (dict(scratch=None), "null"), (dict(record=None), "null"),
                     (dict(npad=96), "npad"), (dict(npad=102), "npad"), (dict(every=-1), "every"),
                     (dict(fields=ctypes.c_void_p(4100)), "16-byte"), (dict(anchor=ctypes.c_void_p(4104)), "16-byte"),
                     (dict(w=ctypes.c_void_p(4100)), "16-byte"), (dict(scratch=ctypes.c_void_p(4100)), "8-byte"),
                     (dict(record=ctypes.c_void_p(4100)), "8-byte")):
        assert call(**kw) != 0 and text in lib.pinn_last_error().decode(), kw


def test_pseudo_time_plan_resolves_onto_the_8_wave_families(lib, monkeypatch):
    from nsfnet_amd import _lib
    switches = ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_FUSE", "PINN_TILE_COLS", "PINN_HBC_SPLIT")
    for k in switches:
        monkeypatch.delenv(k, raising=False)
    net = _net(lib, 3, 6, 256, (1, 1, 1))
    plain = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 360000, 4, ctypes.byref(plain)) == 0
    assert _names(lib, plain)[:2] == ("fwd_split_kernel", "bwd_split_kernel")        # what the feature steps back from
    lib.pinn_plan_destroy(plain)
    walls = _lib.HardBcStruct(1, 2, 0.0, 0.0, 1.0, 10.0)
    seen = []
    for sched in (None, "0", "1", "2"):
        for fuse in (None, "0", "1"):
            for split in (None, "0", "1"):
                for name, val in (("PINN_SCHED", sched), ("PINN_FUSE", fuse), ("PINN_HBC_SPLIT", split)):
                    if val is None:
                        monkeypatch.delenv(name, raising=False)
                    else:
                        monkeypatch.setenv(name, val)
                for bc in (None, walls):
                    rc, plan, err = _create(lib, net, 360000, bc)
                    assert rc == 0, err
                    assert _names(lib, plan) == ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"), (sched, fuse, split)
                    seen.append((lib.pinn_plan_workspace_bytes(plan, 1), lib.pinn_plan_padded_points(plan)))
                    lib.pinn_plan_destroy(plan)
    assert len(set(seen)) == 1
    # ... the plan PINN_SCHED=0 PINN_WSPLIT=0 PINN_FUSE=0 give a plain one
    for k in ("PINN_SCHED", "PINN_WSPLIT", "PINN_FUSE"):
        monkeypatch.setenv(k, "0")
    monkeypatch.delenv("PINN_HBC_SPLIT", raising=False)
    off = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 360000, 4, ctypes.byref(off)) == 0
    assert _names(lib, off) == ("fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel")
    assert (lib.pinn_plan_workspace_bytes(off, 1), lib.pinn_plan_padded_points(off)) == seen[0]
    lib.pinn_plan_destroy(off); lib.pinn_net_destroy(net)
    for k in switches:
        monkeypatch.delenv(k, raising=False)
    # hidden 400: the wide pair, not the wide role-split sweeps
    net = _net(lib, 3, 3, 400, (1, 1, 1))
    plain = ctypes.c_void_p()
    assert lib.pinn_plan_create(net, 5000, 4, ctypes.byref(plain)) == 0
    assert _names(lib, plain)[:2] == ("fwd_wsplit_kernel", "bwd_wsplit_kernel")
    for bc in (None, walls):
        for split in ("0", "1"):
            monkeypatch.setenv("PINN_HBC_SPLIT", split)
            rc, plan, err = _create(lib, net, 5000, bc)
            assert rc == 0, err
            assert _names(lib, plan) == ("fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel")
            lib.pinn_plan_destroy(plan)
    lib.pinn_plan_destroy(plain); lib.pinn_net_destroy(net)


def test_plans_of_the_engine_are_created_as_pseudo_time_plans(lib):
    """ResidualPlan(pseudo_time=True) creates the C plan through pinn_plan_create_pseudo_time (no device is needed to
    create a plan), with the net's wall descriptor where it has one."""
    from nsfnet_amd import engine as eng

    class Net:      # what PointPlan reads of a DeviceNet
        def __init__(self, lib, handle, bc):
            self.lib, self.handle, self.hard_bc, self.device = lib, handle, bc, torch.device("cpu")

    h = _net(lib, 3, 2, 16)
    plan = eng.PointPlan(Net(lib, h, hm.HardBc(lift_power=4).struct()), [0.1, 0.2], [0.3, 0.4], 4, with_backward=False,
                         pseudo_time=True)
    assert plan.hard_bc()["lift_power"] == 4
    s, sp = ctypes.c_float(), ctypes.c_float()
    assert lib.pinn_plan_pseudo_time(plan.handle, ctypes.byref(s), ctypes.byref(sp)) == 0
    plain = eng.PointPlan(Net(lib, h, None), [0.1, 0.2], [0.3, 0.4], 4, with_backward=False)
    assert lib.pinn_plan_pseudo_time(plain.handle, ctypes.byref(s), ctypes.byref(sp)) != 0
    del plan, plain
    lib.pinn_net_destroy(h)


# ---- engine and solvers against the CPU stand-ins ----
def _case():
    rng = np.random.RandomState(0)
    xb, yb, ub, vb = (a.reshape(-1)[::64] for a in ar.cavity_boundary())
    return dict(x=rng.rand(70), y=rng.rand(70), xb=xb, yb=yb, ub=ub, vb=vb)


def _install(monkeypatch):
    """tests/fakes.py, with a residual plan that knows the pseudo-time term (ptime_model.residual_term) and the advance
    of ptime_model in place of the launch."""
    import fakes
    fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng

    class PtPlan(fakes.FakeResidualPlan):
        def __init__(self, net, x, y, weights=None, with_backward=True, ws=None, pseudo_time=False):
            super().__init__(net, x, y, weights, with_backward, ws)
            self.is_pseudo_time, self.anchor, self.rates = pseudo_time, None, (0.0, 0.0)

        def set_pseudo_time(self, sigma, sigma_p):
            assert self.is_pseudo_time
            if self.anchor is None:
                self.anchor = torch.zeros(3, self.npad)
            self.rates = (float(sigma), float(sigma_p))

        def kernel_names(self):
            return ("fwd_kernel", "bwd_kernel", "dw_kernel")

        def _term(self, alpha_e=1.0, eq4_weight=0.1):
            Re, ev, vt, scale = self._ctx
            x, y = self._xy()
            w = None if self.w is None else self.w.numpy().astype(np.float64)
            return pm.residual_term(self.net.pairs(), x, y, Re, self.anchor[:, :self.n].numpy(), *self.rates,
                                    alpha_e=alpha_e, vis_t=vt, e=ev, w=w, scale=scale, eq4_weight=eq4_weight)

        def forward(self, Re, e=None, vis_t0=0.0, alpha_evm=0.0, scale=1.0, save=True, sums_out=None):
            super().forward(Re, e, vis_t0, alpha_evm, scale, save, sums_out)
            if self.is_pseudo_time:
                so = self.sums if sums_out is None else sums_out
                for k, v in enumerate(self._term()["sums"][:3]):
                    so[k] = v

        def backward(self, Re, coef_eq, e=None, scale=1.0, want_ebar=False, phases=3):
            if not self.is_pseudo_time:
                return super().backward(Re, coef_eq, e, scale, want_ebar, phases)
            self._grad = self._term(alpha_e=0.5 * coef_eq[0] * self.n, eq4_weight=coef_eq[3] / coef_eq[0])["grad"]

    def advance(plan, every, force, scratch, record):
        anchor, rec = pm.advance(plan.fields.numpy(), plan.n, plan.anchor.numpy(), every, force,
                                 None if plan.w is None else plan.w.numpy(), record.numpy())
        plan.anchor.copy_(torch.tensor(anchor))
        record.copy_(torch.tensor(rec))

    monkeypatch.setattr(eng, "ResidualPlan", PtPlan)
    monkeypatch.setattr(eng, "ptime_scratch", lambda n, device: torch.zeros(8, dtype=torch.float64))
    monkeypatch.setattr(eng, "ptime_advance", advance)
    return eng


def test_engine_checks_its_arguments_and_the_order_of_calls(monkeypatch):
    eng = _install(monkeypatch)
    c = _case()
    E = eng.PinnEngine("cpu", 2, 8, 100.0)
    assert E.pseudo_time_info() is None
    for kw in (dict(dtau=0.0, every=1), dict(dtau=-1.0, every=1), dict(dtau=float("nan"), every=1),
               dict(dtau=float("inf"), every=1), dict(dtau=1.0, every=-1), dict(dtau=1.0, every=2.5),
               dict(dtau=1.0, every=1, pressure_dtau=0.0), dict(dtau=1.0, every=1, pressure_dtau=float("nan")),
               dict(every=3, pressure_dtau=1.0)):
        with pytest.raises(ValueError, match="pseudo-time"):
            E.set_pseudo_time(**kw)
        assert E.pseudo_time_info() is None
    for off in (dict(), dict(dtau=None, every=5), dict(dtau=0.5, every=0)):
        E.set_pseudo_time(**off)
        assert E.pseudo_time_info() is None
    E.set_pseudo_time(dtau=0.5, every=4, pressure_dtau=0.25)
    i = E.pseudo_time_info()
    assert (i["dtau"], i["pressure_dtau"], i["sigma"], i["sigma_p"], i["every"]) == (0.5, 0.25, 2.0, 4.0, 4)
    assert i["kernels"] is None and i["refreshes"] is None
    E.set_pseudo_time(dtau=0.5, every=4)
    assert E.pseudo_time_info()["sigma_p"] == 0.0 and E.pseudo_time_info()["pressure_dtau"] is None
    E.set_collocation(c["x"], c["y"])
    for kw in (dict(dtau=0.5, every=4), dict()):
        with pytest.raises(ValueError, match="before set_collocation"):
            E.set_pseudo_time(**kw)
    assert E.pseudo_time_info()["kernels"][-1] == "ptime_advance_kernel"
    with pytest.raises(RuntimeError, match="pseudo-time"):
        eng.PinnEngine("cpu", 2, 8, 100.0).reset_pseudo_time()


def test_engine_refuses_batching_resampling_chunks_and_the_l2_mode(monkeypatch):
    eng = _install(monkeypatch)
    c = _case()
    E = eng.PinnEngine("cpu", 2, 8, 100.0)
    E.set_pseudo_time(dtau=0.5, every=2)
    with pytest.raises(ValueError, match="pseudo-time.*chunk_points"):
        E.set_collocation(c["x"], c["y"], chunk_points=32)
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(c["xb"], c["yb"], c["ub"], c["vb"])
    with pytest.raises(ValueError, match="mini-batching.*pseudo-time"):
        E.set_batching(16)
    E.set_batching(0)                       # off stays allowed
    with pytest.raises(ValueError, match="resample.*pseudo-time"):
        E.resample()
    with pytest.raises(ValueError, match="pseudo-time stepping needs the MSE loss"):
        E.loss_and_grad("L2")
    # the other order: batching first
    B = eng.PinnEngine("cpu", 2, 8, 100.0)
    B._batch = object()
    with pytest.raises(ValueError, match="pseudo-time.*mini-batching"):
        B.set_pseudo_time(dtau=0.5, every=2)


def test_engine_anchors_at_attach_and_advances_once_per_update(monkeypatch):
    eng = _install(monkeypatch)
    c = _case()
    E = eng.PinnEngine("cpu", 2, 8, 100.0, alpha_b=10.0)
    E.net.set_flat(torch.tensor(_flat(3, 2, 8, 1), dtype=torch.float32))
    E.set_pseudo_time(dtau=0.5, every=3, pressure_dtau=2.0)
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(c["xb"], c["yb"], c["ub"], c["vb"])
    f = E.plan_f
    assert f.rates == (2.0, 0.5)
    first = f.anchor.clone()
    np.testing.assert_array_equal(first[0, :f.n].numpy(), f.field("u").numpy())         # the field of the attached weights
    np.testing.assert_array_equal(first[2, :f.n].numpy(), f.field("p").numpy())
    i = E.pseudo_time_info()
    assert (i["since_refresh"], i["refreshes"]) == (0, 1)
    # anchored at its own field the term is the steady one
    E.loss_and_grad()
    lt = E.loss_terms()
    assert "loss_e_steady" in lt and "drift" in lt
    g0 = E.grads.clone()
    E.adam_step(1e-2)
    lt = E.loss_terms()
    assert float(lt["drift"]) == 0.0
    assert abs(float(lt["loss_e"]) - float(lt["loss_e_steady"])) <= 1e-6 * float(lt["loss_e"])
    assert E.pseudo_time_info()["since_refresh"] == 1
    # evaluations alone never advance; updates do, and every third one refreshes
    E.loss_and_grad(); E.loss_and_grad()
    assert E.pseudo_time_info()["since_refresh"] == 1
    assert float(E.loss_terms()["loss_e"]) != float(lt["loss_e"])                      # the weights moved off the anchors
    assert not torch.equal(E.grads, g0)
    seen = []
    for _ in range(6):
        E.step(1e-2)
        j = E.pseudo_time_info()
        seen.append((j["since_refresh"], j["refreshes"]))
    assert seen == [(2, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3)]
    assert float(E.loss_terms()["drift"]) > 0.0
    assert not torch.equal(f.anchor, first)
    # the anchors are one update old: the planes of the evaluation the refreshing update used
    E.step(1e-2)                # since 2
    E.step(1e-2)                # refresh
    np.testing.assert_array_equal(f.anchor[0, :f.n].numpy(), f.field("u").numpy())
    # reset_pseudo_time re-anchors at the current weights and restarts the count
    E.step(1e-2)
    E.reset_pseudo_time()
    j = E.pseudo_time_info()
    assert (j["since_refresh"], j["refreshes"]) == (0, 5) and f.rates == (2.0, 0.5)
    np.testing.assert_array_equal(f.anchor[1, :f.n].numpy(), f.field("v").numpy())
    # the graph key carries the settings
    assert ("ptime", 2.0, 0.5, 3) in E._graph_key(1e-3, False)
    assert not any(isinstance(k, tuple) and k and k[0] == "ptime" for k in eng.PinnEngine("cpu", 2, 8, 100.0)._graph_key(1e-3, False))


def test_lbfgs_call_counts_as_one_update(monkeypatch):
    eng = _install(monkeypatch)
    c = _case()
    E = eng.PinnEngine("cpu", 2, 8, 100.0, alpha_b=10.0)
    E.net.set_flat(torch.tensor(_flat(3, 2, 8, 1), dtype=torch.float32))
    E.set_pseudo_time(dtau=0.5, every=100)
    E.set_collocation(c["x"], c["y"])
    E.set_boundary(c["xb"], c["yb"], c["ub"], c["vb"])
    calls = []
    monkeypatch.setattr(eng._lbfgs, "step", lambda space, state, **kw: (calls.append([space.evaluate() for _ in range(4)]), (0.0, {}))[1])
    monkeypatch.setattr(eng, "LbfgsHistory", lambda n, m, dev: type("H", (), {"history_size": m})())
    monkeypatch.setattr(eng._EngineSpace, "evaluate", lambda self: self.e._loss_and_grad())
    E.lbfgs_step(max_iter=4)
    assert len(calls) == 1 and E.pseudo_time_info()["since_refresh"] == 1          # four evaluations, one advance


def test_solvers_carry_the_option_and_reanchor_on_load(monkeypatch, tmp_path):
    _install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es, pinn_solver as ps
    monkeypatch.chdir(tmp_path)
    c = _case()
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=2, hidden_size=8, N_f=70, bc_weight=10, device="cpu")
    assert not P._pseudo_time
    with pytest.raises(ValueError, match="pseudo-time"):
        P.set_pseudo_time_stepping(-1.0, 3)
    P.set_pseudo_time_stepping(0.5, 3, pressure_dtau=4.0)
    assert P._pseudo_time and P.engine.pseudo_time_info()["sigma_p"] == 0.25
    P.set_boundary_data(X=(c["xb"], c["yb"], c["ub"], c["vb"]))
    P.set_eq_training_data(X=(c["x"], c["y"]))
    with pytest.raises(ValueError, match="before set_collocation"):
        P.set_pseudo_time_stepping(0.5, 3)
    line = P._pseudo_time_log()
    assert "steady loss_e" in line and "drift_uv" in line and "refreshes=1" in line
    P.save("pt.pth", N_HLayer=2, N_neu=8, N_f=70)
    import os
    files = sorted(f for _, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert files == ["eq_losses.mat", "pt.pth"] or files == ["pt.pth"]                 # no anchors in a checkpoint
    ck = [os.path.join(d, "pt.pth") for d, _, fs in os.walk(str(tmp_path)) if "pt.pth" in fs][0]
    P.load(ck)
    assert P.engine.pseudo_time_info()["refreshes"] == 2                               # load re-anchors
    Q = es.PysicsInformedNeuralNetwork(Re=800, layers=2, layers_1=2, hidden_size=8, hidden_size_1=8, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    Q.set_pseudo_time_stepping(0.25, 10)
    assert Q._pseudo_time and Q.engine.pseudo_time_info()["every"] == 10
    Q.set_pseudo_time_stepping(None, 0)
    assert not Q._pseudo_time


# ---- the ev YAML and the convergence script ----
def test_yaml_key_is_off_by_default_and_parses(tmp_path):
    import contextlib
    import importlib.util
    import io
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_ptime", os.path.join(root, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    cfg = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = cfg
    spec.loader.exec_module(cfg)
    prod = os.path.join(root, "nsfnet_amd", "dropin", "ev_nsfnet", "configs", "production.yaml")
    assert not cfg.ConfigManager.from_file(prod).config.training.pseudo_time.enabled
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  pseudo_time: {enabled: true, dtau: 0.25, every: 50, pressure_dtau: 2}\n")
    pt = cfg.ConfigManager.from_file(str(p)).config.training.pseudo_time
    assert (pt.enabled, pt.dtau, pt.every, pt.pressure_dtau) == (True, 0.25, 50, 2.0)
    p.write_text("training:\n  pseudo_time: {dtau: 0.25}\n")
    assert not cfg.ConfigManager.from_file(str(p)).config.training.pseudo_time.enabled
    for bad in ("dtau: 0", "dtau: -1", "every: 0", "pressure_dtau: -1"):
        p.write_text("training:\n  pseudo_time: {enabled: true, %s}\n" % bad)
        with pytest.raises(ValueError, match="pseudo_time"):
            cfg.ConfigManager.from_file(str(p))
    for other in ("resampling: {enabled: true}", "batching: {enabled: true, batch_points: 100}"):
        p.write_text("training:\n  pseudo_time: {enabled: true}\n  %s\n" % other)
        with pytest.raises(ValueError, match="pseudo_time does not go together"):
            cfg.ConfigManager.from_file(str(p))
    out = io.StringIO()
    p.write_text("training:\n  pseudo_time: {enabled: true, dtau: 0.5, every: 20}\n")
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "pseudo-time: dtau=0.5 every=20 pressure_dtau=None" in out.getvalue()


def test_scripts_carry_the_option():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conv = open(os.path.join(root, "scripts", "converge_ev.py")).read()
    assert '"--pseudo-time"' in conv and "set_pseudo_time_stepping(a.pseudo_time[0]" in conv
    assert conv.index("set_pseudo_time_stepping") < conv.index("P.set_eq_training_data")
    train = open(os.path.join(root, "nsfnet_amd", "dropin", "ev_nsfnet", "train.py")).read()
    assert train.index("set_pseudo_time_stepping") < train.index("PINN.set_eq_training_data")
