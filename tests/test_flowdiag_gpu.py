"""GPU tests of the flow diagnostics: pinn_flow_stream_function and pinn_flow_stats on
synthetic planes against the numpy statement of tests/flowdiag_model.py, bit for bit - every row entry and the whole
psi plane -, then the engine: the record of a net's own planes, psi against the fp64 oracle, observe-only, graph replay
against eager, a training state resumed mid-cadence, and the two trained nets whose branches the record tells apart."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import flowdiag_model as fdm  # noqa: E402
import fold_model as fm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402
from oracle import fwdmode_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NPAD = 128          # the planes' stride is padded to a multiple of this, as a plan pads it

# (nx, ny): the smallest grid; odd, unequal, n % 4 != 0; more columns than one workgroup of the scan; several blocks of
# the reduction with a last-block finish; 525 625 points > 512 x 1024, so the grid-stride loop repeats
GRIDS = [(5, 3), (33, 17), (300, 5), (129, 65), (725, 725)]


def _axes(nx, ny, uniform=True):
    xs = np.linspace(0.0, 1.0, nx).astype(np.float32).astype(np.float64)
    s = np.linspace(0.0, 1.0, ny)
    ys = (s if uniform else 0.5 * (1.0 - np.cos(np.pi * s))).astype(np.float32).astype(np.float64)      # clustered at the walls
    return xs, ys


def _synthetic(nx, ny, seed=0):
    """fp32 planes [6, n]: a clockwise vortex with corner eddies plus noise over three decades, so that every quadrant
    has a maximum and the products the kernels form are not exact in fp64 (a fused multiply-add would show)."""
    rng = np.random.RandomState(seed)
    xs, ys = _axes(nx, ny)
    X, Y = np.meshgrid(xs, ys)
    u = -np.sin(np.pi * X) ** 2 * np.sin(2 * np.pi * Y) * np.pi + 0.3 * np.sin(3 * np.pi * X) * np.cos(5 * np.pi * Y)
    fld = 0.2 * rng.randn(6, nx * ny) * 10.0 ** rng.uniform(-3.0, 0.0, size=(6, nx * ny))
    fld[fdm.U] += u.reshape(-1)
    return fld.astype(np.float32)


def _device_planes(fld, n):
    """Device planes [FLD_COUNT, npad] of the rows, everything past n (and the planes the kernels never read)
    poisoned with NaN."""
    from nsfnet_amd import engine as eng
    npad = -(-n // NPAD) * NPAD
    t = torch.full((eng.FLD_COUNT, npad), float("nan"), dtype=torch.float32, device=DEV)
    t[:6, :n] = torch.tensor(np.asarray(fld, np.float32)[:, :n], device=DEV)
    return t


def _run(fld, xs, ys, eps=1e-3, t=-1.0, every=7, capacity=3, planes=None, psi_in=None):
    """Both entry points on fresh state: (row, psi, state, scratch head) as numpy."""
    from nsfnet_amd import engine as eng
    nx, ny = len(xs), len(ys)
    F = _device_planes(fld, nx * ny) if planes is None else planes
    dxs, dys = torch.tensor(xs, device=DEV), torch.tensor(ys, device=DEV)
    psi = torch.full((nx * ny,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = eng.flow_scratch(DEV)
    st = torch.zeros(eng.FLOW_STATE, dtype=torch.float64, device=DEV)
    ring = torch.zeros(capacity, eng.FLOW_RECORD, dtype=torch.float64, device=DEV)
    if psi_in is None:
        eng.flow_stream_function(F, nx, ny, dys, psi)
    else:
        psi.copy_(torch.tensor(psi_in, device=DEV))
    eng.flow_stats(F, nx, ny, dxs, dys, psi, eps, t, every, scratch, st, ring)
    torch.cuda.synchronize()
    return ring[0].cpu().numpy(), psi.cpu().numpy(), st.cpu().numpy(), scratch[:32].cpu().numpy()


def _model(fld, xs, ys, eps=1e-3, t=-1.0, every=7, psi_in=None):
    st, ring = np.zeros(fdm.STATE), np.zeros((3, fdm.RECORD))
    psi = fdm.stream_function(fld[fdm.U], ys, len(xs), len(ys)) if psi_in is None else np.asarray(psi_in, np.float64)
    return fdm.stats(fld, psi, xs, ys, eps, t, every, st, ring), psi, st


def _same(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = np.flatnonzero(~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------- the kernels on synthetic planes
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_both_kernels_match_the_model_bit_for_bit(nx, ny):
    fld = _synthetic(nx, ny, seed=nx + ny)
    xs, ys = _axes(nx, ny)
    row, psi, st, scr = _run(fld, xs, ys)
    mrow, mpsi, mst = _model(fld, xs, ys)
    _same(psi, mpsi, "psi")
    _same(row, mrow, "row")
    _same(st, mst, "state")
    assert scr[0] == 0.0 and row[0] == 7.0 and row[27] == 0.0 and not row[28:].any()     # the ticket is 0 again
    assert np.isfinite(row).all() and row[21] > 0.0
    # the scratch head is what the header says: psi_min, its point, ..., the quadrant counts
    n = nx * ny
    assert scr[1] == row[3] and scr[2] == float(np.argmin(mpsi)) and scr[16] == 0.0
    _same(scr[17:21] / float(n), row[[8, 12, 16, 20]], "counts")


def test_a_non_uniform_grid_and_a_second_call_on_the_same_scratch():
    from nsfnet_amd import engine as eng
    nx, ny = 33, 17
    xs, ys = _axes(nx, ny, uniform=False)
    fld = _synthetic(nx, ny, seed=4)
    row, psi, _, _ = _run(fld, xs, ys, eps=5e-3, t=12.5)
    mrow, mpsi, _ = _model(fld, xs, ys, eps=5e-3, t=12.5)
    _same(psi, mpsi, "psi")
    _same(row, mrow, "row")
    assert row[0] == 12.5
    # a sequence on one scratch, state and ring: the cadence position is device state, the ring wraps
    F = _device_planes(fld, nx * ny)
    dxs, dys = torch.tensor(xs, device=DEV), torch.tensor(ys, device=DEV)
    psi_d = torch.zeros(nx * ny, dtype=torch.float64, device=DEV)
    scratch = eng.flow_scratch(DEV)
    st = torch.zeros(eng.FLOW_STATE, dtype=torch.float64, device=DEV)
    ring = torch.zeros(2, eng.FLOW_RECORD, dtype=torch.float64, device=DEV)
    mst, mring = np.zeros(fdm.STATE), np.zeros((2, fdm.RECORD))
    for k, t in enumerate((-1.0, -1.0, 40.0, -1.0)):
        F[fdm.U, :nx * ny] *= 1.25
        eng.flow_stream_function(F, nx, ny, dys, psi_d)
        eng.flow_stats(F, nx, ny, dxs, dys, psi_d, 1e-3, t, 3, scratch, st, ring)
        f = F[:6, :nx * ny].cpu().numpy()
        fdm.stats(f, fdm.stream_function(f[fdm.U], ys, nx, ny), xs, ys, 1e-3, t, 3, mst, mring)
    torch.cuda.synchronize()
    _same(st.cpu().numpy(), mst, "state")
    _same(ring.cpu().numpy().reshape(-1), mring.reshape(-1), "ring")
    assert list(fdm.history(st.cpu().numpy(), ring.cpu().numpy())[:, 0]) == [40.0, 9.0]


def test_planted_ties_and_an_extremum_on_each_edge():
    nx, ny = 33, 17
    xs, ys = _axes(nx, ny)
    fld = _synthetic(nx, ny, seed=9)
    n = nx * ny
    base = 0.01 * np.random.RandomState(1).rand(n) - 0.005
    node = lambda i, j: j * nx + i
    cases = {
        "ties": ([node(20, 9), node(4, 3), node(28, 14)], [node(30, 2), node(18, 6)]),
        "left": ([node(0, 8)], [node(0, 3)]),
        "right": ([node(nx - 1, 5)], [node(nx - 1, 12)]),
        "bottom": ([node(7, 0)], [node(25, 0)]),
        "lid": ([node(11, ny - 1)], [node(16, ny - 2)]),
        "corner": ([node(0, 0)], [node(nx - 1, 0)]),
    }
    for name, (mins, maxs) in cases.items():
        psi = base.copy()
        psi[mins] = -2.0
        psi[maxs] = 3.0
        row, _, _, scr = _run(fld, xs, ys, psi_in=psi)
        mrow, _, _ = _model(fld, xs, ys, psi_in=psi)
        _same(row, mrow, name)
        assert scr[2] == float(min(mins)), name          # the lowest point of the tie
        assert row[3] == -2.0 and 3.0 in row[[7, 11, 15, 19]], name
    psi = base.copy()
    psi[node(5, ny - 1)] = 50.0                          # on the lid: the mass defect, no quadrant's maximum
    row, _, _, _ = _run(fld, xs, ys, psi_in=psi)
    _same(row, _model(fld, xs, ys, psi_in=psi)[0], "lid maximum")
    assert row[22] == 50.0 and row[[7, 11, 15, 19]].max() < 1.0


def test_poisoned_padding_does_not_reach_a_result_and_a_planted_nan_blanks_the_record():
    nx, ny = 33, 17                                      # n = 561: the last quad of every plane is partial
    xs, ys = _axes(nx, ny)
    fld = _synthetic(nx, ny, seed=2)
    row, psi, st, _ = _run(fld, xs, ys)                  # _device_planes poisons everything past n
    assert np.isfinite(row).all() and np.isfinite(psi).all() and st[fdm.S_NONFINITE] == 0.0
    for plane, at, count in ((fdm.U, 5 * nx + 7, ny - 5), (fdm.UY, 40, 1), (fdm.VY, nx * ny - 1, 1)):
        bad = fld.copy()
        bad[plane, at] = np.nan if plane != fdm.VY else np.inf
        row, psi, st, _ = _run(bad, xs, ys)
        mrow, mpsi, mst = _model(bad, xs, ys)
        _same(row, mrow, "row")
        _same(psi, mpsi, "psi")
        _same(st, mst, "state")
        assert row[27] == count and np.isnan(row[1:27]).all() and row[0] == 7.0 and not row[28:].any()
        assert st[fdm.S_NONFINITE] == 1.0


# ---------------------------------------------------------------- engines
def _bc(every=16):
    return tuple(a.reshape(-1)[::every].astype(np.float32) for a in ar.cavity_boundary())


def _engine(L, H, prec, variant="plain", seed=5, flow=None, points=True):
    from nsfnet_amd import engine as eng
    E = eng.PinnEngine(DEV, L, H, 2000.0, alpha_b=10.0, alpha_e=1.0, precision=prec)
    E.net.set_flat(torch.tensor(ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().copy()))
    if variant == "hard":
        E.set_hard_boundary(lift_power=2)
    elif variant == "fourier":
        E.set_fourier_features(sigma=1.0, seed=3)
    if points:
        rng = np.random.RandomState(seed)
        E.set_collocation(rng.rand(2000).astype(np.float32), rng.rand(2000).astype(np.float32))
        E.set_boundary(*_bc())
    if flow is not None:
        E.set_flow_diagnostics(**flow)
    return E


def _oracle_u(E, variant, x, y):
    """u of the engine's net at the points, by the fp64 oracle."""
    P = fr.unflatten(E.net.params.cpu().numpy().astype(np.float64), 2, 3, E.net.n_hidden, E.net.hidden)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if variant == "hard":
        import hardbc_model as hm
        return hm.constrained_value(P, hm.HardBc(lift_power=2), x, y)["pred"][:, 0]
    if variant == "fourier":
        import fourier_model
        return fourier_model.forward1(P, x, y)[0][:, 0]
    return fr.forward1(P, x, y)[0][:, 0]


def _device_record(E):
    """(row, psi, planes) of the engine's last diagnostic, as numpy."""
    d = E._flow
    torch.cuda.synchronize()
    k = int(d.state[0].item())
    return d.ring[(k - 1) % d.capacity].cpu().numpy(), d.psi.cpu().numpy(), d.plan.fields.cpu().numpy()


U_BAR = {"fp32": 2e-5, "bf16x3": 5e-4}      # the field bars of tests/test_hip_kernels.py, relative to max |u|


@pytest.mark.parametrize("variant", ["plain", "hard", "fourier"])
@pytest.mark.parametrize("L,H", [(2, 16), (3, 24)])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_the_record_is_the_model_on_the_plans_own_planes(L, H, prec, variant):
    nx, ny = 33, 17
    E = _engine(L, H, prec, variant, flow=dict(nx=nx, ny=ny, every=1, history=4), points=False)
    r = E.flow_diagnostics(t=3.0)
    row, psi, planes = _device_record(E)
    d = E._flow
    xs, ys = d.xs.cpu().numpy(), d.ys.cpu().numpy()
    mrow, mpsi, _ = _model(planes[:6, :nx * ny], xs, ys, t=3.0, every=1)
    _same(psi, mpsi, "psi")
    _same(row, mrow, "row")
    assert r["t"] == 3.0 and r["nonfinite"] == 0.0 and r["psi_min"] == row[3]
    # psi against the fp64 oracle: a trapezoid sum of an error bounded by b over the length L is bounded by L b
    x, y = np.tile(xs, ny), np.repeat(ys, nx)
    u = _oracle_u(E, variant, x, y)
    b = U_BAR[prec] * np.abs(u).max()
    err_u = np.abs(planes[0, :nx * ny] - u).max()
    want = fdm.stream_function(u, ys, nx, ny)
    err = np.abs(psi - want).max()
    print("%s %dx%d %s: max |u - oracle| = %.3e (bar %.3e), max |psi - oracle| = %.3e" % (variant, L, H, prec, err_u, b, err))
    assert err <= (ys[-1] - ys[0]) * b
    f = E.flow_fields(refresh=False)
    assert f["psi"].shape == (ny, nx) and torch.equal(f["omega"].reshape(-1), d.plan.field("v_x") - d.plan.field("u_y"))


def _params(E):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (E.net.params, E.net.m, E.net.v)]


@pytest.mark.parametrize("L,H,prec", [(2, 16, "fp32"), (3, 24, "bf16x3")])
def test_observing_leaves_the_training_bitwise_alone(L, H, prec, monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    E = _engine(L, H, prec, flow=dict(nx=33, ny=17, every=2, history=8))
    R = _engine(L, H, prec)
    for _ in range(5):
        E.step(1e-3); R.step(1e-3)
    for a, b in zip(_params(E), _params(R)):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    h = E.flow_history()
    assert list(h[:, 0]) == [2.0, 4.0] and np.isfinite(h).all()


@pytest.mark.parametrize("validate", [False, True])
def test_graph_replay_equals_eager_in_the_ring(validate, monkeypatch):
    every = 3

    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E = _engine(3, 24, "fp32", flow=dict(nx=33, ny=17, every=every, history=8))
        if validate:
            rng = np.random.RandomState(17)
            x, y = rng.rand(301).astype(np.float32), rng.rand(301).astype(np.float32)
            E.set_validation(x, y, np.sin(x), np.cos(y), every=2, history=8)
        for _ in range(4 * every + 1):                   # every key is captured on its first use and replayed after
            E.step(1e-3)
        torch.cuda.synchronize()
        return E, E.flow_history(), (E.validation_history() if validate else None), _params(E)

    Eg, hg, vg, pg = run(True)
    Ee, he, ve, pe = run(False)
    assert len(Eg._graphs) == (4 if validate else 2) and not Ee._graphs
    assert list(he[:, 0]) == [3.0, 6.0, 9.0, 12.0]
    _same(hg.reshape(-1), he.reshape(-1), "flow ring")
    if validate:
        _same(vg.reshape(-1), ve.reshape(-1), "validation ring")
    for a, b in zip(pg, pe):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_a_training_state_resumes_mid_cadence(tmp_path, monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "0")
    flow = dict(nx=33, ny=17, every=3, history=2)
    whole = _engine(3, 24, "fp32", flow=flow)
    for _ in range(10):
        whole.step(1e-3)
    first = _engine(3, 24, "fp32", flow=flow)
    for _ in range(5):
        first.step(1e-3)
    path = str(tmp_path / "s.bin")
    first.save_training_state(path)
    second = _engine(3, 24, "fp32", seed=6, flow=flow)
    assert second.load_training_state(path)["changed"] == []
    for _ in range(5):
        second.step(1e-3)
    torch.cuda.synchronize()
    _same(second._flow.state.cpu().numpy(), whole._flow.state.cpu().numpy(), "state")
    _same(second._flow.ring.cpu().numpy().reshape(-1), whole._flow.ring.cpu().numpy().reshape(-1), "ring")
    assert list(whole.flow_history()[:, 0]) == [6.0, 9.0]


# ---------------------------------------------------------------- the two trained nets on the DNS grid
@pytest.fixture(scope="module")
def dns_topology():
    import flow_topology as ft
    X, Y, U, V = ft.load_dns(os.path.join(ROOT, "tests", "golden", "dns", "cavity_Re2000_256.mat"))
    return ft.topology(X, Y, U, V)


def _trained(name, L, H):
    from nsfnet_amd import engine as eng
    E = eng.PinnEngine(DEV, L, H, 2000.0, precision="bf16x3")
    E.net.load_state_dict(torch.load(os.path.join(ROOT, "tests", "golden", "trained", name), map_location="cpu",
                                     weights_only=True))
    E.set_flow_diagnostics(nx=257, ny=257, every=1)
    r = E.flow_diagnostics(t=0.0)
    row, psi, planes = _device_record(E)
    d = E._flow
    mrow, mpsi, _ = _model(planes[:6, :257 * 257], d.xs.cpu().numpy(), d.ys.cpu().numpy(), t=0.0, every=1)
    _same(psi, mpsi, name + " psi")
    _same(row, mrow, name + " row")
    print(name, {k: r[k] for k in ("x_c", "y_c", "psi_min", "counter_area", "mass_defect", "div_max")})
    return r


def test_the_ev_net_is_on_the_dns_branch(dns_topology):
    r, p = _trained("ev_re2000_6x80_net.pth", 6, 80), dns_topology["primary"]
    assert abs(r["x_c"] - p["x"]) < 0.02 and abs(r["y_c"] - p["y"]) < 0.02
    assert abs(r["psi_min"] - p["psi_min"]) < 0.05 * abs(p["psi_min"])
    eddies = {e["where"]: e for e in dns_topology["eddies"]}
    for where, q in (("bottom-right", "br"), ("bottom-left", "bl")):
        assert abs(r["x_" + q] - eddies[where]["x"]) < 0.03 and abs(r["y_" + q] - eddies[where]["y"]) < 0.03, where
    assert r["counter_area"] < 0.1


def test_the_plain_net_is_on_the_other_branch(dns_topology):
    r, p = _trained("nsfnet_re2000_4x120_net.pth", 4, 120), dns_topology["primary"]
    assert np.hypot(r["x_c"] - p["x"], r["y_c"] - p["y"]) > 0.1
    assert r["counter_area"] > 0.25


# ---------------------------------------------------------------- the coordinate map and the script's device path
def test_the_record_is_physical_under_the_coordinate_map():
    """N on xi = 2 x - 1 at coordinate scale 2 against N'(x) = N(2 x - 1) at scale 1 (W0' = 2 W0, b0' = b0 - W0 (1, 1)): one
    physical field, so one record up to the fp32 rounding of the planes and of the first layer."""
    from nsfnet_amd import engine as eng
    L, H, nx, ny = 3, 24, 33, 17
    flat = ar.flat_params(ar.seeded_net(3, L, H, seed=5)).numpy().astype(np.float64)
    W0, b0 = flat[:2 * H].reshape(H, 2).copy(), flat[2 * H:3 * H].copy()
    plain = flat.copy()
    plain[:2 * H], plain[2 * H:3 * H] = (2.0 * W0).reshape(-1), b0 - W0.sum(axis=1)
    rows = []
    for params, scale in ((flat, 2.0), (plain, 1.0)):
        E = eng.PinnEngine(DEV, L, H, 2000.0, precision="fp32", coord_scale=scale)
        E.net.set_flat(torch.tensor(params, dtype=torch.float32))
        E.set_flow_diagnostics(nx=nx, ny=ny, every=1)
        rows.append(E.flow_diagnostics(t=1.0))
        row, psi, planes = _device_record(E)
        d = E._flow
        assert float(d.plan.x.min()) == (-1.0 if scale == 2.0 else 0.0)
        _same(d.xs.cpu().numpy(), np.linspace(0.0, 1.0, nx), "xs")
        mrow, mpsi, _ = _model(planes[:6, :nx * ny], d.xs.cpu().numpy(), d.ys.cpu().numpy(), t=1.0, every=1)
        _same(psi, mpsi, "psi")
        _same(row, mrow, "row")
    a, b = rows
    print({k: (a[k], b[k]) for k in ("x_c", "y_c", "psi_min", "mass_defect", "ke", "counter_area")})
    floor = max(abs(b["psi_min"]), 1e-3)
    for k in ("psi_min", "mass_defect", "ke", "enstrophy", "div_rms", "omega_c"):
        assert abs(a[k] - b[k]) <= 1e-4 * max(abs(b[k]), floor), (k, a[k], b[k])
    assert abs(a["x_c"] - b["x_c"]) <= 1e-3 and abs(a["y_c"] - b["y_c"]) <= 1e-3
    assert abs(a["counter_area"] - b["counter_area"]) <= 2.0 / (nx * ny)


def test_the_scripts_device_path_reproduces_the_engines_record(monkeypatch):
    """scripts/flow_topology.py --device-fields: device_fields() + topology(psi=...) on the ev net give the primary
    vortex, the mass defect and the corner eddies of the engine's own record."""
    import flow_topology as ft
    monkeypatch.setenv("NSFNET_PRECISION", "bf16x3")
    X, Y, _, _ = ft.load_dns(os.path.join(ROOT, "tests", "golden", "dns", "cavity_Re2000_256.mat"))
    net = os.path.join(ROOT, "tests", "golden", "trained", "ev_re2000_6x80_net.pth")
    u, v, psi = ft.device_fields(net, X, Y, 6, 80)
    assert u.shape == v.shape == psi.shape == X.shape
    t = ft.topology(X, Y, u, v, psi=psi)
    from nsfnet_amd import engine as eng
    E = eng.PinnEngine(DEV, 6, 80, 2000.0)
    E.net.load_state_dict(torch.load(net, map_location="cpu", weights_only=True))
    E.set_flow_diagnostics(xs=X[0], ys=Y[:, 0], every=1)
    r = E.flow_diagnostics(t=0.0)
    p = t["primary"]
    assert p["psi_min"] == r["psi_min"] and abs(p["x"] - r["x_c"]) <= 1e-12 and abs(p["y"] - r["y_c"]) <= 1e-12
    assert t["mass_defect"] == r["mass_defect"] and abs(t["kinetic_energy"] - r["ke"]) <= 1e-12
    eddies = {e["where"]: e for e in t["eddies"]}
    for where, q in (("bottom-right", "br"), ("bottom-left", "bl")):
        assert eddies[where]["psi"] == r["psi_max_" + q] and abs(eddies[where]["x"] - r["x_" + q]) <= 1e-12, where
        assert abs(eddies[where]["area"] - r["area_" + q]) <= 2.0 / X.size, where
