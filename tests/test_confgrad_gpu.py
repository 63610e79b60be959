"""GPU tests of the conflict-free combination of the per-term gradients: the Gram, coefficient
and combine kernels against tests/confgrad_model.py, the equal-projection property of the device output, the whole step
against the fp64 oracle's per-term gradients through the real sweeps, the launch accounting, graph replay, the
compositions (chunked passes, mini-batching, weight factorization) and the ev drop-in with the YAML block on."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import confgrad_model as cm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402
from oracle import fwdmode_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = float(np.finfo(np.float32).eps)


def _bc(every=16):
    return tuple(a.reshape(-1)[::every].astype(np.float32) for a in ar.cavity_boundary())


def _rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _plain_engine(L, H, n, prec="fp32", alpha_b=10.0, alpha_e=1.0, seed=5, Re=400.0, chunk=None, batch=0, rwf=False):
    from nsfnet_amd import engine as eng
    flat = ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().copy()
    E = eng.PinnEngine(DEV, L, H, Re, alpha_b=alpha_b, alpha_e=alpha_e, precision=prec)
    E.net.set_flat(torch.tensor(flat))
    rng = np.random.RandomState(seed)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    E.set_collocation(x, y, chunk_points=chunk)
    E.set_boundary(*_bc())
    if batch:
        E.set_batching(batch, seed=3)
    if rwf:
        E.set_weight_factorization(seed=1)
    return E, flat, x, y


# ---------------------------------------------------------------- kernels against the model
def _vectors(P, kind, rng):
    gr = (rng.randn(P) * 10.0 ** rng.uniform(-3, 1, P)).astype(np.float32)
    gb = (rng.randn(P) * 1e-2).astype(np.float32)
    gs = (rng.randn(P) * 1e-3).astype(np.float32)
    if kind == "two_terms":
        gs = None
    elif kind == "zero_b":
        gb[:] = 0
    elif kind == "all_zero":
        gr[:] = 0; gb[:] = 0; gs[:] = 0
    elif kind == "nan_s":
        gs[P // 2] = np.nan
    elif kind == "antiparallel":
        gb = (-2.0 * gr).astype(np.float32)
    return [gr, gb, gs]


def _run_kernels(vecs, rec0):
    from nsfnet_amd import engine as eng
    P = vecs[0].size
    dv = [None if v is None else torch.tensor(v, device=DEV) for v in vecs]
    parts = eng.confgrad_partials(P, DEV)
    coef = torch.zeros(3, device=DEV)
    rec = torch.tensor(rec0, device=DEV)
    eng.confgrad_gram(dv, P, parts)
    eng.confgrad_coef(parts, P, 2 if vecs[2] is None else 3, coef, rec)
    g = torch.empty(P, device=DEV)
    eng.confgrad_combine(g, dv[0], dv[1], dv[2], coef)
    torch.cuda.synchronize()
    return parts.cpu().numpy(), coef.cpu().numpy(), rec.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("P", [1, 257, 330499])
@pytest.mark.parametrize("kind", ["plain", "two_terms", "zero_b", "all_zero", "nan_s", "antiparallel"])
def test_kernels_match_model(P, kind):
    rng = np.random.RandomState(P % 1000 + len(kind))
    vecs = _vectors(P, kind, rng)
    rec0 = np.zeros(cm.RECORD)
    rec0[10:13] = (5, 1, 2)                                   # counters carried from earlier steps
    parts, coef, rec, g = _run_kernels(vecs, rec0)
    again = _run_kernels(vecs, rec0)
    for a, b in zip((parts, coef, rec, g), again):
        np.testing.assert_array_equal(a, b)                  # bit-reproducible
    ref_parts = cm.block_partials(vecs, P)
    np.testing.assert_allclose(parts.reshape(-1, 6), ref_parts, rtol=1e-12, atol=0)
    m = 2 if vecs[2] is None else 3
    ref = cm.coefficients(cm.sum_partials(ref_parts), m, rec0)
    if kind in ("plain", "two_terms") and P > 1:
        # the coefficient bound below is 1e-12 x cond(M) x 10: hold the inputs to cond(M) <= 10
        a, b, c = ref[3:6]
        assert np.linalg.cond(np.array([[1, a, b], [a, 1, c], [b, c, 1]])) <= 10.0
        assert ref[11] == 1 and ref[12] == 2 and (ref[6:6 + m] > 0).all()
    # guard branches and counters exactly as the model decides them
    np.testing.assert_array_equal(rec[10:13], ref[10:13])
    fallback = ref[11] == 2
    if P == 1 and kind != "all_zero":
        assert fallback                                       # one parameter: every cosine is +-1
    want = dict(plain=P == 1, two_terms=P == 1, zero_b=P == 1, all_zero=False, nan_s=True, antiparallel=True)[kind]
    assert fallback == want
    assert rec[12] - 2 == dict(zero_b=1, all_zero=3).get(kind, 0)          # zero-norm terms dropped in this step
    if fallback:
        assert list(rec[6:9]) == [1.0, 1.0, 1.0]
    if kind == "all_zero":
        assert list(rec[6:9]) == [0.0, 0.0, 0.0] and rec[9] == 0.0
    np.testing.assert_allclose(rec[:10], ref[:10], rtol=1e-10, atol=0)
    assert list(coef) == [np.float32(v) for v in rec[6:9]]
    ref_g = cm.combine(vecs[0], vecs[1], vecs[2], coef)
    fin = np.isfinite(ref_g)
    assert np.array_equal(np.isfinite(g), fin)
    if fin.any():
        scale = sum(abs(float(coef[t])) * np.abs(vecs[t][np.isfinite(vecs[t])]).max() for t in range(m))
        np.testing.assert_allclose(g[fin], ref_g[fin], rtol=0, atol=4 * EPS * scale + 1e-300)


def test_combine_output_has_equal_projections():
    """g . g_t / |g_t| agree across the terms, and g . g is the record's |g|^2: both to the rounding of the fp32
    coefficients and of the three fp32 operations per element, 8 eps sum |k_t| n_t in the 2-norm."""
    P = 330499
    vecs = _vectors(P, "plain", np.random.RandomState(P % 1000 + len("plain")))
    _, coef, rec, g = _run_kernels(vecs, np.zeros(cm.RECORD))
    assert rec[11] == 0 and rec[12] == 0
    g = g.astype(np.float64)
    v64 = [v.astype(np.float64) for v in vecs]
    norms = [np.linalg.norm(v) for v in v64]
    bound = 8 * EPS * sum(abs(float(coef[t])) * norms[t] for t in range(3))
    proj = [g @ v / n for v, n in zip(v64, norms)]
    print("projections", proj, "spread", np.ptp(proj), "bound", bound)
    assert min(proj) > 0 and np.ptp(proj) <= bound
    # | |g| - rec | <= bound  =>  | g.g - rec^2 | <= (2 rec + bound) bound
    assert abs(g @ g - rec[9] ** 2) <= (2 * rec[9] + bound) * bound


# ---------------------------------------------------------------- against the fp64 oracle through the real sweeps
@functools.lru_cache(maxsize=None)
def _oracle_terms(L, H, n, seed=5, Re=400.0):
    """fp64 g_r and g_b (unit boundary weight) of _plain_engine(L, H, n): computed once, shared, never modified."""
    flat = ar.flat_params(ar.seeded_net(3, L, H, seed=seed)).numpy().astype(np.float64)
    rng = np.random.RandomState(seed)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    P = fr.unflatten(flat, 2, 3, L, H)
    xb, yb, ub, vb = (a.astype(np.float64) for a in _bc())
    gr = fr.pde_loss_and_grad(P, x.astype(np.float64), y.astype(np.float64), Re, alpha_e=1.0)["grad"]
    gb = fr.bc_loss_and_grad(P, xb, yb, ub, vb, alpha_b=1.0)["grad"]
    gr.setflags(write=False); gb.setflags(write=False)
    return gr, gb


@pytest.mark.parametrize("L,H,n", [(2, 16, 40000), (3, 64, 20000)])
def test_step_matches_model_on_oracle_terms(L, H, n):
    """fp32 mode at point counts where the sweeps' tile loops repeat, alpha_b = 10.  Bar 1e-3 of max|g|: each term
    carries the 2e-4 bar of the term-split assembly, each of the two coefficients is a ratio of norms (2 x 2e-4).
    The test prints the measured figures; DESIGN.md section 7.8 says which of them have been recorded."""
    from nsfnet_amd import engine as eng
    E, _, _, _ = _plain_engine(L, H, n)
    E.set_conflict_free_gradients()
    E.loss_and_grad()
    torch.cuda.synchronize()
    g = E.grads.cpu().numpy().astype(np.float64)
    info = E.conflict_info()
    gr, gb = _oracle_terms(L, H, n)
    g_ref, rec = cm.step([gr, 10.0 * gb, None])
    assert rec[11] == 0 and rec[12] == 0
    err = _rel_max(g, g_ref)
    print("confgrad oracle (%d, %d, %d): err %.3e  cos %.4f (oracle %.4f)  k (%.4f, %.4f)  n_r %.6e (%.6e)  n_b %.6e (%.6e)"
          % (L, H, n, err, info["cos_rb"], rec[3], info["k_r"], info["k_b"], info["n_r"], rec[0], info["n_b"], rec[1]))
    assert info["steps"] == 1 and info["fallbacks"] == 0 and info["dropped"] == 0
    assert err < 1e-3
    assert abs(info["n_r"] - rec[0]) <= 4e-4 * rec[0] and abs(info["n_b"] - rec[1]) <= 4e-4 * rec[1]
    assert abs(info["cos_rb"] - rec[3]) <= 4e-4          # two unit vectors, each within 2e-4
    # the assembly's Gram partials are those of the vectors it wrote, and asking for them changes nothing else
    outs = [[torch.empty(E.P, device=DEV) for _ in range(2)] for _ in range(2)]
    parts = [eng.balance_partials(E.P, DEV) for _ in range(2)]
    gram = eng.confgrad_partials(E.P, DEV)
    groups = [[E.plan_f], [E.plan_b], []]
    eng.grad_reduce_terms(E.net, groups, outs[0] + [None], partials=parts[0])
    eng.grad_reduce_terms(E.net, groups, outs[1] + [None], partials=parts[1], gram=gram)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(*parts)
    assert torch.equal(outs[0][1], E._cfg.gb)
    ref = cm.block_partials([outs[1][0].cpu().numpy(), outs[1][1].cpu().numpy(), None], E.P)
    np.testing.assert_allclose(gram.cpu().numpy().reshape(-1, 6), ref, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(gram.cpu().numpy(), E._cfg.parts.cpu().numpy())


# ---------------------------------------------------------------- launch accounting
def _call_names(monkeypatch, E, lr=1e-3):
    """The C-ABI calls of one step, in order (every one of the calls compared below is a single launch)."""
    from nsfnet_amd import _lib
    names, real = [], _lib.check

    def check(rc, what=""):
        names.append(what)
        return real(rc, what)

    monkeypatch.setattr(_lib, "check", check)
    E.step(lr)
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "check", real)
    return names


def test_one_rank_step_gains_exactly_the_coefficient_and_combine_launches(monkeypatch):
    monkeypatch.delenv("NSFNET_GRAPH", raising=False)
    A, _, _, _ = _plain_engine(3, 24, 2000)
    B, _, _, _ = _plain_engine(3, 24, 2000)
    C, _, _, _ = _plain_engine(3, 24, 2000)
    B.set_conflict_free_gradients()
    C.set_conflict_free_gradients()
    C.set_conflict_free_gradients(False)
    off, on, off_again = (_call_names(monkeypatch, E) for E in (A, B, C))
    assert off == off_again and off.count("pinn_grad_reduce") == 1
    assert not [n for n in off if "confgrad" in n or "terms" in n or "balance" in n]
    i = off.index("pinn_grad_reduce")
    assert on == off[:i] + ["pinn_grad_reduce_terms_gram", "pinn_confgrad_coef", "pinn_confgrad_combine"] + off[i + 1:]
    np.testing.assert_array_equal(A.net.params.cpu().numpy(), C.net.params.cpu().numpy())


# ---------------------------------------------------------------- graph
def test_graph_replay_is_bit_identical_to_eager(monkeypatch):
    def run(graph):
        monkeypatch.setenv("NSFNET_GRAPH", "1" if graph else "0")
        E, _, _, _ = _plain_engine(3, 24, 3000)
        E.set_conflict_free_gradients()
        for _ in range(6):
            E.step(1e-3)
        torch.cuda.synchronize()
        if graph:
            assert len(E._graphs) == 1                      # no cadence: one graph serves every step
        return E.net.params.cpu().numpy(), E._cfg.rec.cpu().numpy(), E._cfg.coef.cpu().numpy()

    eager, graph = run(False), run(True)
    for a, b in zip(eager, graph):
        np.testing.assert_array_equal(a, b)
    assert eager[1][10] == 6 and eager[1][11] == 0


# ---------------------------------------------------------------- composition
def _own_terms(**cfg):
    """The term vectors of a configuration as the feature-off step assembles them: with alpha_b = 0 the boundary
    seeds are zero and grads is g_r, with alpha_e = 0 the equation seeds are zero and grads is alpha_b g_b."""
    out = []
    for ab, ae in ((0.0, 1.0), (10.0, 0.0)):
        E, _, _, _ = _plain_engine(alpha_b=ab, alpha_e=ae, **cfg)
        E.loss_and_grad()
        torch.cuda.synchronize()
        out.append(E.grads.cpu().numpy().copy())
    return out


def _combined(**cfg):
    E, _, _, _ = _plain_engine(**cfg)
    E.set_conflict_free_gradients()
    E.loss_and_grad()
    torch.cuda.synchronize()
    return E, E.grads.cpu().numpy().copy(), E._cfg.rec.cpu().numpy()


def _assert_equals_model(g, rec, terms):
    g_ref, ref = cm.step([terms[0], terms[1], None])
    assert ref[11] == 0 and rec[11] == 0 and rec[12] == 0
    np.testing.assert_allclose(rec[:10], ref[:10], rtol=1e-10, atol=0)
    scale = sum(abs(ref[6 + t]) * np.abs(terms[t]).max() for t in range(2))
    np.testing.assert_allclose(g, g_ref, rtol=0, atol=4 * EPS * scale)


def test_chunked_passes_equal_model_and_single_pass():
    cfg = dict(L=3, H=32, n=2000)
    E, g, rec = _combined(chunk=512, **cfg)
    assert len(E.plan_f.chunks) == 4
    _assert_equals_model(g, rec, _own_terms(chunk=512, **cfg))
    _, g1, rec1 = _combined(**cfg)
    _assert_equals_model(g1, rec1, _own_terms(**cfg))
    assert np.linalg.norm(g.astype(np.float64) - g1) <= 2e-6 * np.linalg.norm(g1.astype(np.float64))
    np.testing.assert_allclose(rec[[0, 1, 6, 7, 9]], rec1[[0, 1, 6, 7, 9]], rtol=2e-6)
    E.step(1e-3)
    torch.cuda.synchronize()
    assert E.conflict_info()["steps"] == 2 and torch.isfinite(E.net.params).all()


def test_minibatching_at_full_batch_equals_model():
    cfg = dict(L=3, H=32, n=2000, batch=2000)
    E, g, rec = _combined(**cfg)
    assert E.evaluated_batch
    _assert_equals_model(g, rec, _own_terms(**cfg))
    E.step(1e-3)
    torch.cuda.synchronize()
    assert E.conflict_info()["steps"] == 2 and torch.isfinite(E.net.params).all()


def test_weight_factorization_acts_on_the_effective_gradient():
    cfg = dict(L=3, H=32, n=2000, rwf=True)
    E, g, rec = _combined(**cfg)
    _assert_equals_model(g, rec, _own_terms(**cfg))
    E.set_grad_clipping(0.5)                                 # the clipping norm sees the combined gradient's d theta
    E.step(1e-3)
    torch.cuda.synchronize()
    gth = E.net.gtheta.cpu().numpy().astype(np.float64)
    assert abs(E.optimizer_info()["grad_norm"] - np.linalg.norm(gth)) <= 1e-5 * np.linalg.norm(gth)
    assert E.conflict_info()["steps"] == 2 and torch.isfinite(E.net.params).all()


# ---------------------------------------------------------------- ev drop-in
def test_ev_dropin_runs_with_the_yaml_block(tmp_path):
    import scipy.io
    work = tmp_path / "ev"
    subprocess.run(["cp", "-r", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet"), str(work)], check=True)
    X, Y = np.meshgrid(np.linspace(0, 1, 33), np.linspace(0, 1, 33))
    dns = str(tmp_path / "dns.mat")
    scipy.io.savemat(dns, dict(X_ref=X, Y_ref=Y, U_ref=np.sin(np.pi * X) * Y, V_ref=-0.1 * np.cos(np.pi * Y) * X,
                               P_ref=X * Y))
    (work / "cfg.yaml").write_text(
        "experiment_name: t\nphysics: {Re: 2000, alpha_evm: 0.05, bc_weight: 10, eq_weight: 1}\n"
        "network: {layers: 3, layers_1: 2, hidden_size: 32, hidden_size_1: 16}\n"
        "training:\n  N_f: 2000\n  log_interval: 1\n  enable_tensorboard: false\n"
        "  conflict_free_gradients: {enabled: true}\n"
        "  training_stages:\n    - {alpha: 0.05, epochs: 3, lr: 1.0e-3, name: 'Stage 1'}\n"
        "supervision: {enabled: true, num_samples: 30, loss_weight: 0.5}\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "train.py", "--config", "cfg.yaml", "--data", dns], cwd=str(work),
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "conflict-free gradients: on" in out
    lines = [line for line in out.splitlines() if "conflict-free: |g_r|=" in line]
    assert lines, out[-2000:]
    steps = [int(line.split("fallbacks=")[1].split("/")[1].split()[0]) for line in lines]
    assert max(steps) >= 3 and all("fallbacks=0/" in line for line in lines)
    ks = [float(v.strip("(), ")) for v in lines[-1].split("k=")[1].split("fallbacks")[0].split(",")]
    assert len(ks) == 3 and all(np.isfinite(ks)) and all(k > 0 for k in ks)          # three active terms
    losses = [float(line.split("loss=")[1].split()[0]) for line in out.splitlines()
              if "loss=" in line and "eq_total=" in line]
    assert len(losses) >= 3 and all(np.isfinite(losses))
