"""CPU tests of the flow diagnostics: the numpy model of tests/flowdiag_model.py against
scripts/flow_topology.py on the DNS fields and on an analytic vortex, its tie, edge and NaN rules, the argument
refusals of the C ABI (no device needed: they come before any launch), and the host logic around the entry points on
the model-backed fakes - off is off, the cadence and its graph keys, the order behind an update, the refusals, the
solvers, the ev drop-in's YAML key and the training state.  The kernels are checked against the model in
test_flowdiag_gpu.py."""
import contextlib
import ctypes
import importlib.util
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import flow_topology as ft  # noqa: E402
import flowdiag_model as fdm  # noqa: E402
import fold_model as fm  # noqa: E402

DNS = os.path.join(ROOT, "tests", "golden", "dns")
DNS_FILES = {2000: "cavity_Re2000_256.mat", 3000: "cavity_Re3000_256_Uniform.mat", 4000: "cavity_Re4000_384_Uniform.mat",
             5000: "cavity_Re5000_256_Uniform.mat"}
L, H, RE = 2, 10, 400.0
LR = 2.0 ** -10


def tensor_grid(X, Y, U, V):
    """(planes [6, n] with u and v filled, xs, ys) of a field on a tensor grid in either axis order, x fastest."""
    if np.abs(np.diff(Y, axis=0)).max() <= np.abs(np.diff(Y, axis=1)).max():      # y along axis 1: transpose
        X, Y, U, V = X.T, Y.T, U.T, V.T
    fld = np.zeros((6, U.size))
    fld[fdm.U], fld[fdm.V] = U.reshape(-1), V.reshape(-1)
    return fld, X[0].copy(), Y[:, 0].copy()


@pytest.fixture(scope="module")
def dns():
    """Per Reynolds number: the script's topology and the model's row and psi, each computed once."""
    out = {}
    for Re, f in DNS_FILES.items():
        X, Y, U, V = ft.load_dns(os.path.join(DNS, f))
        fld, xs, ys = tensor_grid(X, Y, U, V)
        row, psi = fdm.diagnose(fld, xs, ys)
        out[Re] = dict(script=ft.topology(X, Y, U, V), row=row, psi=psi, shape=X.shape, grid=(X, Y, U))
    return out


# ------------------------------------------------------------------ the model against scripts/flow_topology.py
@pytest.mark.parametrize("Re", sorted(DNS_FILES))
def test_primary_vortex_is_the_scripts(dns, Re):
    d = dns[Re]
    p, row = d["script"]["primary"], d["row"]
    X, Y, U = d["grid"]
    psi = ft.stream_function(X, Y, U)
    assert np.abs(psi.reshape(-1) - d["psi"]).max() <= 1e-12
    assert int(np.argmin(psi)) == int(np.argmin(d["psi"]))                      # the same node
    assert abs(row["x_c"] - p["x"]) <= 1e-12 and abs(row["y_c"] - p["y"]) <= 1e-12
    assert abs(row["psi_min"] - p["psi_min"]) <= 1e-12
    assert abs(row["mass_defect"] - d["script"]["mass_defect"]) <= 1e-12
    assert abs(row["ke"] - d["script"]["kinetic_energy"]) <= 1e-12
    assert row["nonfinite"] == 0.0 and row["t"] == 0.0


@pytest.mark.parametrize("Re", sorted(DNS_FILES))
def test_quadrant_rows_are_the_scripts_eddies(dns, Re):
    d = dns[Re]
    row, n = d["row"], d["shape"][0] * d["shape"][1]
    eddies = {e["where"]: e for e in d["script"]["eddies"]}
    for where, q in (("bottom-right", "br"), ("bottom-left", "bl"), ("top-left", "tl")):
        if where not in eddies:
            continue
        e = eddies[where]
        assert abs(row["psi_max_" + q] - e["psi"]) <= 1e-12, where
        assert abs(row["x_" + q] - e["x"]) <= 1e-12 and abs(row["y_" + q] - e["y"]) <= 1e-12, where
        assert abs(row["area_" + q] - e["area"]) <= 2.0 / n, where
    assert "bottom-right" in eddies and "bottom-left" in eddies
    assert row["area_tr"] == 0.0
    assert row["counter_area"] == ((row["area_bl"] + row["area_br"]) + row["area_tl"]) + row["area_tr"]
    if Re == 2000:
        # the top-left eddy is only starting: 14 nodes, 2.12e-4 of the grid, at the script's min_area of 2e-4
        assert row["area_tl"] < 3e-4
    else:
        assert "top-left" in eddies and row["area_tl"] > 0.004


def test_the_two_numbers_of_the_dns_branch(dns):
    r = dns[2000]["row"]
    assert abs(r["x_c"] - 0.5240) < 1e-4 and abs(r["y_c"] - 0.5495) < 1e-4 and abs(r["psi_min"] + 0.10990) < 1e-5
    assert abs(r["counter_area"] - 0.0586) < 1e-4
    assert abs(r["psi_max_br"] - 2.167e-3) < 1e-6 and abs(r["area_br"] - 0.04248361) < 1e-8


def test_an_analytic_vortex_in_both_axis_orders():
    n = 201
    s = np.linspace(0.0, 1.0, n)
    X, Y = np.meshgrid(s, s)
    U = -np.sin(np.pi * X) ** 2 * 2 * np.pi * np.sin(np.pi * Y) * np.cos(np.pi * Y)
    V = 2 * np.pi * np.sin(np.pi * X) * np.cos(np.pi * X) * np.sin(np.pi * Y) ** 2
    rows = []
    for Xg, Yg, Ug, Vg in ((X, Y, U, V), (X.T, Y.T, U.T, V.T)):
        fld, xs, ys = tensor_grid(Xg, Yg, Ug, Vg)
        row, _ = fdm.diagnose(fld, xs, ys)
        t = ft.topology(Xg, Yg, Ug, Vg)
        assert abs(row["x_c"] - 0.5) < 2e-3 and abs(row["y_c"] - 0.5) < 2e-3 and abs(row["psi_min"] + 1.0) < 1e-3
        assert abs(row["x_c"] - t["primary"]["x"]) <= 1e-12 and abs(row["psi_min"] - t["primary"]["psi_min"]) <= 1e-12
        assert row["counter_area"] == 0.0 and row["mass_defect"] < 1e-3
        rows.append(row)
    assert rows[0] == rows[1]


def _planes(nx, ny, seed=0):
    rng = np.random.RandomState(seed)
    return rng.randn(6, nx * ny).astype(np.float32)


def test_ties_take_the_lowest_point_and_edges_are_not_refined():
    nx, ny = 7, 5
    xs, ys = np.linspace(0, 1, nx), np.linspace(0, 1, ny) ** 2
    fld = _planes(nx, ny)
    psi = np.zeros(nx * ny)
    psi[[9, 17, 23]] = -2.0                          # the minimum three times: point 9 = node (2, 1)
    psi[[4, 11]] = 3.0                               # BR maximum twice: point 4 = node (4, 0), on the bottom edge
    psi[nx * (ny - 1) + 3] = -7.0                    # the lid row takes part in the minimum, not in a quadrant maximum
    psi[nx * (ny - 1) + 5] = 9.0
    st, ring = np.zeros(fdm.STATE), np.zeros((2, fdm.RECORD))
    r = dict(zip(fdm.ROW, fdm.stats(fld, psi, xs, ys, 1e-3, 5.0, 1, st, ring)))
    assert r["psi_min"] == -7.0 and r["y_c"] == ys[-1] and r["mass_defect"] == 9.0
    psi[nx * (ny - 1) + 3] = 0.0
    r = dict(zip(fdm.ROW, fdm.stats(fld, psi, xs, ys, 1e-3, 6.0, 1, st, ring)))
    assert r["psi_min"] == -2.0 and (r["x_c"], r["y_c"]) == fdm.centre(psi, 9, xs, ys)
    assert r["psi_max_br"] == 3.0 and r["y_br"] == ys[0]             # the tie's lowest point lies on the edge: y as it is
    X, Y = np.meshgrid(xs, ys)
    assert (r["x_c"], r["y_c"]) == ft._refine(psi.reshape(ny, nx), 1, 2, X, Y)
    assert (r["x_br"], r["y_br"]) == ft._refine(psi.reshape(ny, nx), 0, 4, X, Y)
    assert r["t"] == 6.0 and st[fdm.S_RECORDS] == 2.0 and st[fdm.S_CADENCE] == 0.0
    assert fm.same_bits(fdm.history(st, ring)[:, 0], [5.0, 6.0])


def test_a_nonfinite_node_blanks_the_record():
    nx, ny = 5, 4
    xs, ys = np.linspace(0, 1, nx), np.linspace(0, 1, ny)
    fld = _planes(nx, ny, 3)
    st, ring = np.zeros(fdm.STATE), np.zeros((3, fdm.RECORD))
    good, _ = fdm.diagnose(fld, xs, ys, t=-1.0, every=10, state=st, ring=ring)
    assert good["t"] == 10.0 and good["nonfinite"] == 0.0 and np.isfinite(list(good.values())).all()
    for plane, count in ((fdm.U, ny - 1), (fdm.VX, 1), (fdm.UX, 1)):      # a NaN in u poisons psi from its row up
        bad = fld.copy()
        bad[plane, nx + 2] = np.nan
        row, _ = fdm.diagnose(bad, xs, ys, t=-1.0, every=10, state=st, ring=ring)
        assert row["nonfinite"] == count and row["t"] > 10.0
        assert all(np.isnan(v) for k, v in row.items() if k not in ("t", "nonfinite"))
        assert not ring[int(st[fdm.S_RECORDS] - 1) % 3, 28:].any()       # the padding stays +0
    assert st[fdm.S_NONFINITE] == 3.0 and st[fdm.S_CADENCE] == 4.0 and st[fdm.S_RECORDS] == 4.0


def test_a_quadrant_without_nodes_below_the_lid():
    xs, ys = np.linspace(0, 1, 4), np.array([0.0, 0.1, 1.0])
    row, _ = fdm.diagnose(_planes(4, 3, 1), xs, ys)
    assert np.isnan(row["psi_max_tl"]) and np.isnan(row["x_tr"]) and row["area_tl"] == row["area_tr"] == 0.0
    assert np.isfinite(row["psi_max_bl"]) and np.isfinite(row["counter_area"])


# ------------------------------------------------------------------ the C ABI refuses by name, before any launch
@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def test_abi_refuses_bad_arguments_by_name(lib):
    assert lib.pinn_flow_scratch_bytes() >= (32 + 16 * 512) * 8
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    def stats(nx=5, ny=4, fields=p, npad=32, xs=p, ys=p, psi=p, eps=1e-3, t=-1.0, every=1, scratch=p, state=p, ring=p,
              capacity=4):
        return lib.pinn_flow_stats(nx, ny, fields, npad, xs, ys, psi, eps, t, every, scratch, state, ring, capacity, None)

    for kw, word in ((dict(nx=2), b"nx must be"), (dict(ny=2), b"ny must be"), (dict(nx=1 << 16, ny=1 << 16), b"nx * ny"),
                     (dict(npad=16), b"npad"), (dict(npad=22), b"npad"), (dict(fields=None), b"fields"),
                     (dict(fields=odd), b"fields"), (dict(capacity=0), b"capacity"), (dict(every=0), b"every"),
                     (dict(eps=-1.0), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(t=-2.0), b"t must be"),
                     (dict(xs=None), b"null"), (dict(state=odd), b"8-byte"), (dict(psi=ctypes.c_void_p(p.value + 8)), b"psi")):
        assert stats(**kw) == -22 and word in lib.pinn_last_error(), kw
        assert b"pinn_flow_stats" in lib.pinn_last_error()
    f = lib.pinn_flow_stream_function
    assert f(2, 4, p, 32, p, p, None) == -22 and b"pinn_flow_stream_function: nx must be" in lib.pinn_last_error()
    assert f(5, 4, p, 32, None, p, None) == -22 and b"null" in lib.pinn_last_error()
    assert f(5, 4, p, 32, p, ctypes.c_void_p(p.value + 8), None) == -22 and b"psi" in lib.pinn_last_error()


# ------------------------------------------------------------------ the engine and the solvers on the fakes
def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", seed=5, setup=None):
    import flowdiag_fakes
    flowdiag_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=2, hidden_e=6, alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev)
    rng = np.random.RandomState(seed)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"])
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    if setup is not None:
        setup(e)
    return e


def _model_row(e, t, every=1):
    d = e._flow
    st, ring = np.zeros(fdm.STATE), np.zeros((1, fdm.RECORD))
    psi = fdm.stream_function(d.plan.fields[0].numpy(), d.ys.numpy(), d.nx, d.ny)
    return fdm.stats(d.plan.fields.numpy(), psi, d.xs.numpy(), d.ys.numpy(), d.eps, t, every, st, ring), psi


def test_off_is_off_in_the_call_log_and_in_the_state_file(monkeypatch, tmp_path):
    import flowdiag_fakes
    case = _case()
    never = _engine(monkeypatch, case, "ev")
    toggled = _engine(monkeypatch, case, "ev")
    toggled.set_flow_diagnostics(nx=9, ny=7, every=2)
    toggled.set_flow_diagnostics(every=0)
    logs = []
    for e in (never, toggled):
        del flowdiag_fakes.CALLS[:]
        for _ in range(3):
            e.step(LR)
        logs.append(list(flowdiag_fakes.CALLS))
        assert e.flow_info() is None and not [c for c in logs[-1] if c[0].startswith("flow")]
        with pytest.raises(RuntimeError, match="flow diagnostics are off"):
            e.flow_history()
    assert logs[0] == logs[1]
    assert never._graph_key(LR, False) == toggled._graph_key(LR, False)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    never.save_training_state(a)
    toggled.save_training_state(b)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    import state_model as sm
    header, _ = sm.parse(raw)
    assert "flow" not in header["fingerprint"] and "flow" not in header["info"] and "flow_n" not in header["host"]
    assert not [s for s in header["segments"] if s["name"].startswith("flow")]
    on = _engine(monkeypatch, case, "ev", setup=lambda e: e.set_flow_diagnostics(nx=9, ny=7, every=2, history=16))
    on.step(LR)
    c = str(tmp_path / "c.bin")
    on.save_training_state(c)
    header, _ = sm.parse(open(c, "rb").read())
    assert header["fingerprint"]["flow"] == dict(nx=9, ny=7, capacity=16) and header["info"]["flow"] == [2, 1e-3]
    assert header["host"]["flow_n"] == 1
    assert [s["name"] for s in header["segments"] if s["name"].startswith("flow")] == [
        "flow.state", "flow.ring", "flow.xs", "flow.ys"]
    with pytest.raises(ValueError, match="fingerprint key 'flow'"):
        never.load_training_state(c)


def test_the_cadence_its_rows_and_the_order_behind_an_update(monkeypatch):
    import flowdiag_fakes
    case = _case()
    e = _engine(monkeypatch, case)
    xv, yv = np.linspace(0, 1, 6), np.linspace(0, 1, 5)
    X, Y = np.meshgrid(xv, yv)
    e.set_convergence_monitor(window=2)
    e.set_validation(X.reshape(-1), Y.reshape(-1), u=X.reshape(-1), v=Y.reshape(-1), every=2)
    e.set_flow_diagnostics(nx=9, ny=7, every=3, history=2)
    assert e.flow_info()["last"] is None and e.flow_history().shape == (0, fdm.RECORD)
    want_t = []
    for i in range(1, 10):
        del flowdiag_fakes.CALLS[:]
        due = e._flow_due()
        assert due == (i % 3 == 0)
        e.step(LR)
        names = [c[0] for c in flowdiag_fakes.CALLS]
        behind = [n for n in names if n in ("monitor_observe", "val_stats", "flow_stream_function", "flow_stats")]
        want = ["monitor_observe"] + (["val_stats"] if i % 2 == 0 else []) + (
            ["flow_stream_function", "flow_stats"] if due else [])
        assert behind == want, i
        if due:
            want_t.append(float(i))
            assert [c for c in flowdiag_fakes.CALLS if c[0] == "flow_stats"] == [("flow_stats", 9, 7, 1e-3, -1.0, 3)]
            row, psi = _model_row(e, float(i))
            assert fm.same_bits(e.flow_history()[-1], row)
            assert fm.same_bits(e.flow_fields(refresh=False)["psi"].numpy().reshape(-1), psi)
    assert want_t == [3.0, 6.0, 9.0] and list(e.flow_history()[:, 0]) == [6.0, 9.0]      # the ring of 2 wrapped
    info = e.flow_info()
    assert info["records"] == 3 and info["nonfinite"] == 0 and info["last"]["t"] == 9.0 and (info["nx"], info["ny"]) == (9, 7)
    e.lbfgs_step(max_iter=2)                         # one call = one update; the explicit record does not move the cadence
    assert e._flow.n == 10
    r = e.flow_diagnostics()
    assert r["t"] == 10.0 and e._flow.state[fdm.S_CADENCE] == 3.0 and e.flow_info()["records"] == 4
    f = e.flow_fields()
    assert f["psi"].shape == (7, 9) and f["psi"].dtype == torch.float64 and f["omega"].shape == (7, 9)
    assert torch.equal(f["omega"], f["psi"].new_tensor(0).float() + (e._flow.plan.field("v_x") - e._flow.plan.field("u_y")).view(7, 9))
    assert fm.same_bits(f["xs"].numpy(), np.linspace(0, 1, 9).astype(np.float32).astype(np.float64))


def test_graph_keys_name_the_grid_eps_and_what_the_step_does(monkeypatch):
    e = _engine(monkeypatch, _case())
    off = e._graph_key(LR, False)
    e.set_flow_diagnostics(nx=9, ny=7, every=3)
    plain = e._graph_key(LR, False)
    assert plain != off and plain[:len(off)] == off and ("flow", 9, 7, 3, 1e-3, 4096) in plain
    diag = e._graph_key(LR, False, False, True)
    assert diag != plain and "diagnose" in diag
    xv = np.linspace(0, 1, 5)
    e.set_validation(xv, xv, u=xv, v=xv, every=2)
    keys = {e._graph_key(LR, False, v, d) for v in (False, True) for d in (False, True)}
    assert len(keys) == 4
    for kw in (dict(nx=10), dict(ny=8), dict(eps=2e-3), dict(every=4)):
        e.set_flow_diagnostics(**dict(dict(nx=9, ny=7, every=3), **kw))
        assert e._graph_key(LR, False, False, True) not in keys, kw
    e.set_flow_diagnostics(every=0)
    e.set_validation(None, None, every=0)
    assert e._graph_key(LR, False) == off


def test_refusals_name_the_argument(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    for kw, word in ((dict(nx=2), "nx must be >= 3"), (dict(ny=1), "ny must be >= 3"), (dict(every=-1), "every"),
                     (dict(eps=-1e-3), "eps"), (dict(eps=float("inf")), "eps"), (dict(history=0), "history"),
                     (dict(xs=[0.0, 0.5]), "xs must have at least 3"), (dict(ys=[0.0, 0.5, 0.5]), "ys must be finite and strictly"),
                     (dict(xs=[0.0, 1.0, 1.0 + 1e-9]), "xs must be finite and strictly increasing in fp32"),
                     (dict(domain=(0.0, 0.0, 0.0, 1.0)), "domain")):
        with pytest.raises(ValueError, match="flow diagnostics: .*" + word):
            e.set_flow_diagnostics(**kw)
        assert e.flow_info() is None
    e.set_flow_diagnostics(xs=[0.0, 0.25, 1.0], ys=[0.0, 0.5, 0.75, 1.0], every=1)
    assert (e._flow.nx, e._flow.ny) == (3, 4) and e._flow.plan.n == 12
    assert list(e._flow.plan.x[:4].numpy()) == [0.0, 0.25, 1.0, 0.0] and list(e._flow.plan.y[:4].numpy()) == [0.0, 0.0, 0.0, 0.5]
    with pytest.raises(ValueError, match="flow_diagnostics: t must be"):
        e.flow_diagnostics(t=-1.0)
    with pytest.raises(ValueError, match="before any point set is attached"):
        e.set_hard_boundary()
    with pytest.raises(ValueError, match="before any point set is attached"):
        e.set_fourier_features(sigma=1.0)


def _bare(monkeypatch, **kw):
    import flowdiag_fakes
    flowdiag_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    e = eng.PinnEngine("cpu", L, H, RE, **kw)
    e.net.set_flat(torch.tensor(np.random.RandomState(5).randn(e.P) * 0.3, dtype=torch.float32))
    return e


def test_domain_defaults_to_where_the_cavity_lies(monkeypatch):
    e = _bare(monkeypatch)
    e.set_flow_diagnostics(nx=3, ny=3, every=1)
    assert list(e._flow.xs.numpy()) == [0.0, 0.5, 1.0] and list(e._flow.plan.x[:3].numpy()) == [0.0, 0.5, 1.0]
    e.set_flow_diagnostics(nx=3, ny=5, every=1, domain=(-1.0, 1.0, 0.0, 2.0))
    assert list(e._flow.xs.numpy()) == [-1.0, 0.0, 1.0] and list(e._flow.ys.numpy()) == [0.0, 0.5, 1.0, 1.5, 2.0]
    # hard walls say where the cavity lies: their box is the domain, their origin the physical (0, 0)
    e = _bare(monkeypatch)
    e.set_hard_boundary(origin=(0.25, -0.5), inv_len=1.0)
    e.set_flow_diagnostics(nx=3, ny=5, every=1)
    assert list(e._flow.plan.x[:3].numpy()) == [0.25, 0.75, 1.25] and list(e._flow.plan.y[::3].numpy()) == [-0.5, -0.25, 0.0, 0.25, 0.5]
    assert list(e._flow.xs.numpy()) == [0.0, 0.5, 1.0] and list(e._flow.ys.numpy()) == [0.0, 0.25, 0.5, 0.75, 1.0]
    e = _bare(monkeypatch, coord_scale=2.0)
    e.set_hard_boundary(origin=(-1.0, -1.0), inv_len=0.5)
    e.set_flow_diagnostics(nx=3, ny=3, every=1)
    assert list(e._flow.plan.x[:3].numpy()) == [-1.0, 0.0, 1.0] and list(e._flow.xs.numpy()) == [0.0, 0.5, 1.0]
    # the [-1, 1] map of the ev data loader without hard walls; any other scale needs the walls to say where the cavity is
    e = _bare(monkeypatch, coord_scale=2.0)
    e.set_flow_diagnostics(nx=5, ny=3, every=1)
    assert list(e._flow.plan.x[:5].numpy()) == [-1.0, -0.5, 0.0, 0.5, 1.0] and list(e._flow.plan.y[::5].numpy()) == [-1.0, 0.0, 1.0]
    assert list(e._flow.xs.numpy()) == [0.0, 0.25, 0.5, 0.75, 1.0] and list(e._flow.ys.numpy()) == [0.0, 0.5, 1.0]
    e = _bare(monkeypatch, coord_scale=3.0)
    with pytest.raises(ValueError, match="flow diagnostics: coordinate scale 3 is neither"):
        e.set_flow_diagnostics(nx=3, ny=3, every=1)
    assert e.flow_info() is None
    e = _bare(monkeypatch)
    e.set_flow_diagnostics(nx=3, ny=3, every=1)
    e.scale = 2.0
    with pytest.raises(RuntimeError, match="the coordinate scale changed from 1 to 2"):
        e.flow_diagnostics()


def test_the_record_is_physical_under_the_coordinate_map(monkeypatch):
    """The net N on input coordinates xi = 2 x - 1 at coordinate scale 2 is the net N'(x) = N(2 x - 1) at scale 1 (layer
    0: W0' = 2 W0, b0' = b0 - W0 (1, 1)): the same physical field, so the same record up to the fp32 rounding of the
    planes and of the changed first layer - not psi doubled, not the quarter [0, 1]^2 of the mapped cavity."""
    mapped = _bare(monkeypatch, coord_scale=2.0)
    plain = _bare(monkeypatch)
    flat = mapped.net.params.numpy().astype(np.float64).copy()
    W0, b0 = flat[:2 * H].reshape(H, 2), flat[2 * H:3 * H]
    flat[2 * H:3 * H] = b0 - W0.sum(axis=1)
    flat[:2 * H] = (2.0 * W0).reshape(-1)
    plain.net.set_flat(torch.tensor(flat, dtype=torch.float32))
    rows = []
    for e in (mapped, plain):
        e.set_flow_diagnostics(nx=33, ny=17, every=1)
        rows.append(e.flow_diagnostics(t=1.0))
        assert fm.same_bits(e._flow.xs.numpy(), np.linspace(0.0, 1.0, 33))
        row, psi = _model_row(e, 1.0)
        assert fm.same_bits(e.flow_history()[-1], row)
    assert float(mapped._flow.plan.x.min()) == -1.0 and float(plain._flow.plan.x.min()) == 0.0
    a, b = rows
    scale = max(abs(a["psi_min"]), 1e-3)
    for k in ("psi_min", "mass_defect", "ke", "enstrophy", "div_rms", "omega_c"):
        assert abs(a[k] - b[k]) <= 1e-4 * max(abs(b[k]), scale), (k, a[k], b[k])
    assert abs(a["x_c"] - b["x_c"]) <= 1e-3 and abs(a["y_c"] - b["y_c"]) <= 1e-3
    assert abs(a["counter_area"] - b["counter_area"]) <= 2.0 / (33 * 17)


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_a_training_state_resumes_mid_cadence_with_the_same_ring(monkeypatch, tmp_path, flavour):
    case, K = _case(), 5
    setup = lambda e: e.set_flow_diagnostics(nx=9, ny=7, every=3, history=2)
    whole = _engine(monkeypatch, case, flavour, setup=setup)
    for _ in range(2 * K):
        whole.step(LR)
    first = _engine(monkeypatch, case, flavour, setup=setup)
    for _ in range(K):                               # 5 updates: one record, two updates into the next cadence
        first.step(LR)
    path = str(tmp_path / "s.bin")
    first.save_training_state(path)
    second = _engine(monkeypatch, case, flavour, seed=77, setup=setup)
    assert second.load_training_state(path)["changed"] == []
    assert second._flow.n == K and fm.same_bits(second._flow.state.numpy(), first._flow.state.numpy())
    other = _engine(monkeypatch, case, flavour, setup=lambda e: e.set_flow_diagnostics(nx=9, ny=7, every=3, history=2,
                                                                                      domain=(0.0, 2.0, 0.0, 1.0)))
    with pytest.raises(ValueError, match="flow.xs"):
        other.load_training_state(path)
    for _ in range(K):
        second.step(LR)
    assert whole.flow_info()["records"] == 3 and list(whole.flow_history()[:, 0]) == [6.0, 9.0]
    assert fm.same_bits(second._flow.state.numpy(), whole._flow.state.numpy())
    assert fm.same_bits(second._flow.ring.numpy(), whole._flow.ring.numpy())
    np.testing.assert_array_equal(second.net.params.numpy(), whole.net.params.numpy())


def test_observing_does_not_change_the_training(monkeypatch):
    case = _case()
    a = _engine(monkeypatch, case, "ev")
    b = _engine(monkeypatch, case, "ev", setup=lambda e: e.set_flow_diagnostics(nx=9, ny=7, every=2))
    for _ in range(4):
        a.step(LR)
        b.step(LR)
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    np.testing.assert_array_equal(a.net_e.params.numpy(), b.net_e.params.numpy())
    assert b.flow_info()["records"] == 2


def _plain(monkeypatch, case):
    import flowdiag_fakes
    flowdiag_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    torch.manual_seed(1)
    P = ps.PysicsInformedNeuralNetwork(Re=400, layers=L, hidden_size=H, N_f=70, bc_weight=10, device="cpu")
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_every = P.save_every = 0
    return P


def _ev(monkeypatch, case):
    import flowdiag_fakes
    flowdiag_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    torch.manual_seed(0)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=L, layers_1=2, hidden_size=H, hidden_size_1=6, N_f=70,
                                       alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_interval = 1000
    P.save = lambda *a, **k: None
    return P


@pytest.mark.parametrize("kind", ["plain", "ev"])
def test_the_solvers_pass_it_on_and_log_the_vortex_line(monkeypatch, kind):
    P = (_plain if kind == "plain" else _ev)(monkeypatch, _case())
    assert P._flow_diag is False
    P.set_flow_diagnostics(nx=9, ny=7, every=2, eps=2e-3, history=8)
    assert P._flow_diag and P.flow_log() == "vortex: no record yet" and P.flow_history().shape == (0, fdm.RECORD)
    assert (P.engine._flow.eps, P.engine._flow.capacity) == (2e-3, 8)
    for _ in range(4):
        P.engine.step(LR)
    h = P.flow_history()
    assert list(h[:, 0]) == [2.0, 4.0]
    r = dict(zip(fdm.ROW, h[-1]))
    assert P.flow_log() == "vortex (%.4f, %.4f) psi_min %.4f counter-area %.3f mass %.1e" % (
        r["x_c"], r["y_c"], r["psi_min"], r["counter_area"], r["mass_defect"])
    if kind == "ev":
        P.current_stage, P.loss, P.loss_e, P.loss_b = "Stage 1", 0.0, 0.0, 0.0
        for k in ("eq1", "eq2", "eq3", "eq4"):
            setattr(P, "loss_" + k, 0.0)
    else:
        P.loss_eq1 = P.loss_eq2 = P.loss_eq3 = torch.zeros(())
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.print_log(0.0, None, 3, 10)
    assert P.flow_log() in out.getvalue()
    P.set_flow_diagnostics(every=0)
    assert P._flow_diag is False and P.engine.flow_info() is None


def _config_module():
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_flow", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_yaml_key_parses_and_is_validated(tmp_path):
    cfg = _config_module()
    prod = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                    "production.yaml"))
    assert prod.config.training.flow_diagnostics is None             # absent: off
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  flow_diagnostics: {nx: 129, ny: 65, every: 500, eps: 0.002}\n")
    fd = cfg.ConfigManager.from_file(str(p)).config.training.flow_diagnostics
    assert (fd.nx, fd.ny, fd.every, fd.eps) == (129, 65, 500, 0.002)
    p.write_text("training:\n  flow_diagnostics: {every: 250}\n")
    fd = cfg.ConfigManager.from_file(str(p)).config.training.flow_diagnostics
    assert (fd.nx, fd.ny, fd.every, fd.eps) == (257, 257, 250, 1e-3)
    for bad in ("nx: 2", "ny: 0", "every: 0", "eps: -0.1", "eps: .inf"):
        p.write_text("training:\n  flow_diagnostics: {%s}\n" % bad)
        with pytest.raises(ValueError, match="training.flow_diagnostics"):
            cfg.ConfigManager.from_file(str(p))
    for off in ("null", "false"):
        p.write_text("training:\n  flow_diagnostics: %s\n" % off)
        assert cfg.ConfigManager.from_file(str(p)).config.training.flow_diagnostics is None


def test_converge_ev_writes_flow_jsonl(monkeypatch, tmp_path):
    """The script on the fakes, a 2 x 8 net and 40 points: 5 updates of stage 1 at --flow-diag 2 9 7 give two rows of
    flow.jsonl and the last record in the stage record."""
    import json
    import flowdiag_fakes
    flowdiag_fakes.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    spec = importlib.util.spec_from_file_location("converge_ev_flow", os.path.join(ROOT, "scripts", "converge_ev.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "run"
    monkeypatch.setattr(sys, "argv", ["converge_ev.py", "--dns", os.path.join(DNS, DNS_FILES[3000]), "--out", str(out),
                                      "--first", "1", "--last", "1", "--epochs-scale", "1e-5", "--nf", "40", "--layers", "2",
                                      "--hidden", "8", "--flow-diag", "2", "9", "7"])
    cwd = os.getcwd()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            mod.main()
    finally:
        os.chdir(cwd)
    rows = [json.loads(l) for l in open(out / "flow.jsonl")]
    assert [r["t"] for r in rows] == [2.0, 4.0] and all(r["stage"] == 1 and r["nonfinite"] == 0.0 for r in rows)
    assert set(fdm.ROW) <= set(rows[0])
    rec = json.loads(open(out / "stages.jsonl").readline())
    assert rec["flow"]["t"] == 4.0 and rec["flow"]["psi_min"] == rows[-1]["psi_min"]


def test_the_script_takes_a_stream_function_it_is_given(dns):
    """scripts/flow_topology.py --device-fields: topology() with psi handed in is topology() that integrates itself."""
    X, Y, U = dns[2000]["grid"]
    V = ft.load_dns(os.path.join(DNS, DNS_FILES[2000]))[3]
    assert ft.topology(X, Y, U, V, psi=dns[2000]["psi"].reshape(X.shape)) == dns[2000]["script"]
