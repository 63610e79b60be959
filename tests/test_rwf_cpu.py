"""CPU tests of the random weight factorization of the dense layers: the fp64 model against
torch autograd, the engine's host logic on the oracle-backed fakes (the off path makes the parent's calls, the order of
a step with the feature on, the clipping norm and L-BFGS on theta, both nets of the ev flavour and its freeze
schedule), the draw, the ev drop-in's YAML key and the checkpoint sidecar.  The kernels are checked against the model
in test_rwf_gpu.py."""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import optim_model as om  # noqa: E402
import rwf_model as rm  # noqa: E402
from nsfnet_amd.schedule import LrSchedule  # noqa: E402

L, H, RE = 2, 10, 400.0
SHAPE, SHAPE_E = (3, L, H), (1, 2, 6)
LR = 2.0 ** -10


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("shape", [(3, 2, 7), (1, 3, 5), (3, 1, 70)])
def test_model_chain_rule_matches_torch_autograd(shape):
    """d loss / d theta of a scalar function of the effective parameters W = exp(s) V, b: the model's chain rule on
    autograd's effective gradient against autograd through the factorisation, fp64, to 1e-12 relative to the largest
    entry."""
    rng = np.random.RandomState(sum(shape))
    P, R = rm.num_params(*shape), rm.num_rows(*shape)
    theta = np.concatenate([rng.randn(P) * 0.4, 0.5 + 0.1 * rng.randn(R)])
    net = rm.RwfNet(theta, shape)
    np.testing.assert_array_equal(net.theta().numpy(), theta)
    X = torch.tensor(rng.rand(40, 2))
    tgt = torch.tensor(rng.randn(40, shape[0]))
    eff = [t.detach().clone().requires_grad_(True) for W, b in net.weights() for t in (W, b)]
    h = X
    for l in range(len(eff) // 2):
        h = h @ eff[2 * l].t() + eff[2 * l + 1]
        h = torch.tanh(h) if l < len(eff) // 2 - 1 else h
    ((h - tgt) ** 2).mean().backward()
    G = torch.cat([t.grad.reshape(-1) for t in eff]).numpy()
    ((net(X) - tgt) ** 2).mean().backward()
    want = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).numpy()
    got, _ = rm.grad(theta, G, shape, exact_g=True)
    assert np.abs(want[P:]).min() > 0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_model_split_compose_and_layout():
    shape = (3, 2, 5)
    P, R = rm.num_params(*shape), rm.num_rows(*shape)
    assert (P, R) == (2 * 5 + 5 + 5 * 5 + 5 + 3 * 5 + 3, 13)
    rng = np.random.RandomState(0)
    params, s = rng.randn(P).astype(np.float32), (0.5 + 0.1 * rng.randn(R)).astype(np.float32)
    theta = rm.split(params, s, shape)
    assert theta.dtype == np.float32 and theta.size == P + R
    np.testing.assert_array_equal(theta[P:], s)
    g = rm.g_of(s)
    assert theta[0] == params[0] / g[0] and theta[2] == params[2] / g[1]           # layer 0: rows of length 2
    assert theta[10] == params[10] and theta[15 + 5] == params[15 + 5] / g[5 + 1]   # b_0[0]; W_1[1, 0]
    back = rm.compose(theta, shape)
    assert np.abs(back - params).max() <= 2.0 ** -23 * np.abs(params).max()
    for w, b, r, c, so in rm.layout(*shape):
        np.testing.assert_array_equal(back[b:b + r], params[b:b + r])               # biases are copied


# ------------------------------------------------------------------ the engine on the fakes
def _case(seed=42, N=70, Nb=33):
    rng = np.random.RandomState(seed)
    from oracle import autograd_ref as ar
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::63][:Nb] for a in ar.cavity_boundary())
    return dict(x=x, y=y, xb=xb, yb=yb, ub=ub, vb=vb)


def _engine(monkeypatch, case, flavour="nsfnet", **kw):
    import rwf_fakes
    rwf_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    ev = dict(flavour="ev", n_hidden_e=SHAPE_E[1], hidden_e=SHAPE_E[2], alpha_evm=0.05) if flavour == "ev" else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, **ev, **kw)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if flavour == "ev":
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
    e.set_collocation(case["x"], case["y"])
    e.set_boundary(case["xb"], case["yb"], case["ub"], case["vb"])
    return e


def _key(monkeypatch, e):
    """The graph key step() looks up (the probe of test_rba_cpu.py)."""
    keys = []

    class Stop(Exception):
        pass

    class Probe(dict):
        def get(self, key, default=None):
            keys.append(key)
            raise Stop

        def clear(self):
            pass

    monkeypatch.setattr(e, "_graphs_enabled", lambda: True)
    old = e._graphs
    e._graphs = Probe()
    with pytest.raises(Stop):
        e.step(LR)
    e._graphs = old
    monkeypatch.setattr(e, "_graphs_enabled", lambda: False)
    return keys[0]


@pytest.mark.parametrize("flavour", ["nsfnet", "ev"])
def test_off_makes_the_parents_calls(monkeypatch, flavour):
    """Never set, or set and switched off again: the same call log, step by step, with no factorization entry point
    in it, the parent's graph key, and moments of the parameters' size again."""
    import rwf_fakes
    case = _case()
    a = _engine(monkeypatch, case, flavour)
    b = _engine(monkeypatch, case, flavour)
    b.set_weight_factorization(seed=3)
    assert b.weight_factors() is not None and b.net.m.numel() == b.P + rm.num_rows(*SHAPE)
    b.set_weight_factorization(None)
    assert b.weight_factors() is None and b.factorization_info() is None and a.weight_factors() is None
    assert b.net.theta is None and b.net.m.numel() == b.P and b.net.num_train == b.P
    logs = []
    for e in (a, b):
        if flavour == "ev":
            e.e_trainable = True
        del rwf_fakes.CALLS[:]
        for _ in range(2):
            e.step(LR)
        e.lbfgs_step(max_iter=2, line_search_fn="strong_wolfe")
        logs.append(list(rwf_fakes.CALLS))
    assert logs[0] == logs[1]
    # ... and it is the log these very steps gave on the commit before the feature, recorded there with the same fakes
    with open(os.path.join(os.path.dirname(__file__), "golden", "rwf_off_call_log.json")) as f:
        assert [list(c) for c in logs[0]] == json.load(f)[flavour]
    assert not [c for c in logs[0] if c[0].startswith("rwf_")]
    assert [c for c in logs[0] if c[0] == "adam_step"][:2] == [("adam_step", 3, LR)] + (
        [("adam_step", 1, LR)] if flavour == "ev" else [("adam_step", 3, LR)])
    np.testing.assert_array_equal(a.net.params.numpy(), b.net.params.numpy())
    ka, kb = _key(monkeypatch, a), _key(monkeypatch, b)
    assert ka == kb and "rwf" not in ka
    b.set_weight_factorization()
    assert _key(monkeypatch, b) == ka + ("rwf",)


def test_turning_it_on_keeps_params_and_resets_adam_graphs_and_lbfgs(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    for _ in range(2):
        e.step(LR)
    e.lbfgs_step(max_iter=1)
    params = e.net.params.numpy().copy()
    e._graphs["stale"] = object()
    e.set_weight_factorization(mean=1.0, std=0.1, seed=7)
    assert not e._graphs and e._lbfgs is None and e._lbfgs_state.n_iter == 0
    assert e.net.adam_t == 0 and int(e.net.adam_t_dev[0]) == 0 and not e.net.m.any() and not e.net.v.any()
    np.testing.assert_array_equal(e.net.params.numpy(), params)                 # not rewritten before an update
    s = rm.draw(7, 1.0, 0.1, [SHAPE])[0]
    np.testing.assert_array_equal(e.net.theta.numpy(), rm.split(params, s, SHAPE))
    info = e.factorization_info()
    assert info["n_train"] == [e.P + rm.num_rows(*SHAPE)] and len(info["layers"]["net"]) == L + 1
    g = rm.g_of(s)
    assert info["layers"]["net"][0] == dict(min=float(g[:H].min()), max=float(g[:H].max()),
                                            mean=float(g[:H].astype(np.float64).mean()))
    f = e.weight_factors()["net"]
    assert [t.numel() for t in f] == [H, H, 3]
    np.testing.assert_array_equal(torch.cat(f).numpy(), s)
    # load_state_dict with the feature on: params exactly, V re-split with the current s
    sd = {k: torch.randn(shape) for k, shape in e.net.keys_and_shapes()}
    e.net.load_state_dict(sd)
    flat = torch.cat([sd[k].reshape(-1) for k, _ in e.net.keys_and_shapes()]).numpy()
    np.testing.assert_array_equal(e.net.params.numpy(), flat)
    np.testing.assert_array_equal(e.net.theta.numpy(), rm.split(flat, s, SHAPE))
    with pytest.raises(ValueError):
        e.set_weight_factorization(std=-1.0)
    with pytest.raises(ValueError):
        e.set_weight_factorization(factors=dict(net=torch.zeros(3)))


def test_order_of_a_step_with_the_feature_on(monkeypatch):
    """evaluate -> (combine) -> transform -> (norm) -> update -> compose -> prepare, and the update follows the model:
    Adam on theta with the model's d theta, params = compose(theta)."""
    import rwf_fakes
    case = _case()
    e = _engine(monkeypatch, case)
    e.set_weight_factorization(seed=1)
    del rwf_fakes.CALLS[:]
    theta0 = e.net.theta.numpy().copy()
    e.step(LR)
    assert [c[0] for c in rwf_fakes.CALLS] == ["grad_reduce", "rwf_grad", "adam_step", "rwf_compose", "prepare"]
    gth, _ = rm.grad(theta0, e.grads.numpy(), SHAPE)
    np.testing.assert_array_equal(e.net.gtheta.numpy(), gth.astype(np.float32))
    n = theta0.size
    p, m, v = om.update(theta0, gth.astype(np.float32), np.zeros(n), np.zeros(n), 1, LR)
    np.testing.assert_allclose(e.net.theta.numpy(), p.astype(np.float32), rtol=1e-6, atol=1e-9)
    np.testing.assert_array_equal(e.net.params.numpy(), rm.compose(e.net.theta.numpy(), SHAPE))
    assert (e.net.theta.numpy()[e.P:] != theta0[e.P:]).all()                     # the scale factors train
    # with balancing and clipping: the combine comes before the transform, the norm after it
    e.set_loss_balancing(every=1, beta=0.1)
    e.set_grad_clipping(0.5)
    del rwf_fakes.CALLS[:]
    e.step(LR)
    names = [c[0] for c in rwf_fakes.CALLS]
    assert names == ["grad_reduce_terms", "balance_combine", "rwf_grad", "grad_sqnorm", "adam_step_sched", "rwf_compose",
                     "prepare"]


def test_clipping_norm_is_taken_over_dtheta_of_all_trainable_nets(monkeypatch):
    import rwf_fakes
    case = _case()
    e = _engine(monkeypatch, case, "ev")
    e.e_trainable = True
    e.set_weight_factorization(seed=2)
    e.set_lr_schedule(LrSchedule("cosine", t_max=10, eta_min=1e-5))
    e.set_grad_clipping(0.5)
    n0, n1 = e.P + rm.num_rows(*SHAPE), e.P1 + rm.num_rows(*SHAPE_E)
    assert e.factorization_info()["n_train"] == [n0, n1]
    e.loss_and_grad()
    th, the = e.net.theta.numpy().copy(), e.net_e.theta.numpy().copy()
    del rwf_fakes.CALLS[:]
    e.adam_step(LR)
    assert [c[0] for c in rwf_fakes.CALLS] == ["rwf_grad", "rwf_grad", "grad_sqnorm", "adam_step_sched", "rwf_compose",
                                               "prepare", "adam_step_sched", "rwf_compose", "prepare"]
    assert rwf_fakes.CALLS[2] == ("grad_sqnorm", n0, n1)
    g0 = rm.grad(th, e.grads.numpy(), SHAPE)[0].astype(np.float32)
    g1 = rm.grad(the, e.grads_e.numpy(), SHAPE_E)[0].astype(np.float32)
    norm, coef = om.clip(om.sqnorm(g0, g1), 0.5)
    info = e.optimizer_info()
    assert info["grad_norm"] == norm and info["clip_coef"] == float(coef)
    assert norm != om.clip(om.sqnorm(e.grads.numpy(), e.grads_e.numpy()), 0.5)[0]
    # the entropy net frozen: its theta stays, the norm is the main net's
    the1 = e.net_e.theta.numpy().copy()
    e.e_trainable = False
    e.loss_and_grad()
    del rwf_fakes.CALLS[:]
    e.adam_step(LR)
    assert rwf_fakes.CALLS[1] == ("grad_sqnorm", n0, 0) and len([c for c in rwf_fakes.CALLS if c[0] == "rwf_grad"]) == 1
    np.testing.assert_array_equal(e.net_e.theta.numpy(), the1)


def test_lbfgs_runs_on_theta(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case)
    e.set_weight_factorization(seed=4)
    n = e.P + rm.num_rows(*SHAPE)
    theta0 = e.net.theta.numpy().copy()
    e.loss_and_grad()
    loss0 = float(e.loss_terms()["loss"])
    e.lbfgs_step(max_iter=4, history_size=5, line_search_fn="strong_wolfe")
    assert e._lbfgs.n == n and e._lbfgs.d.numel() == n and e._lbfgs.x0.numel() == n
    theta1 = e.net.theta.numpy()
    assert (theta1[:e.P] != theta0[:e.P]).any() and (theta1[e.P:] != theta0[e.P:]).any()
    np.testing.assert_array_equal(e.net.params.numpy(), rm.compose(theta1, SHAPE))
    e.loss_and_grad()
    assert float(e.loss_terms()["loss"]) < loss0
    # the first direction is -d theta: the model's chain rule at theta0, not the effective gradient
    e2 = _engine(monkeypatch, case)
    e2.set_weight_factorization(seed=4)
    e2.lbfgs_step(max_iter=1)
    e3 = _engine(monkeypatch, case)
    e3.set_weight_factorization(seed=4)
    e3.loss_and_grad()
    want = -rm.grad(theta0, e3.grads.numpy(), SHAPE)[0]
    np.testing.assert_allclose(e2._lbfgs.d.numpy(), want.astype(np.float32), rtol=1e-6, atol=1e-12)
    # turning the feature off sizes the next history on the parameters again
    e.set_weight_factorization(None)
    e.lbfgs_step(max_iter=1)
    assert e._lbfgs.n == e.P


def test_ev_factorises_both_nets_and_the_freeze_schedule_keeps_theta(monkeypatch):
    import rwf_fakes
    rwf_fakes.install(monkeypatch)
    from nsfnet_amd import ev_pinn_solver as es
    case = _case()
    torch.manual_seed(0)
    P = es.PysicsInformedNeuralNetwork(Re=800, layers=L, layers_1=SHAPE_E[1], hidden_size=H, hidden_size_1=SHAPE_E[2],
                                       N_f=70, alpha_evm=0.05, bc_weight=10, eq_weight=1)
    P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
    P.set_eq_training_data(X=(case["x"], case["y"]))
    P.log_interval = 1000
    P.save = lambda *a, **k: None
    P.set_weight_factorization(seed=9)
    e = P.engine
    s0, s1 = rm.draw(9, 0.5, 0.1, [SHAPE, SHAPE_E])
    np.testing.assert_array_equal(torch.cat(e.weight_factors()["net"]).numpy(), s0)
    np.testing.assert_array_equal(torch.cat(e.weight_factors()["net_e"]).numpy(), s1)     # the same generator, carried on
    with contextlib.redirect_stdout(io.StringIO()):
        P.train(num_epoch=3, lr=1e-3)
    assert e.net.adam_t == 2                         # re-created at epoch 1 ((epoch - 1) % 10000 == 0), as the reference
    theta, theta_e = e.net.theta.numpy().copy(), e.net_e.theta.numpy().copy()
    e.net.m.fill_(1.0); e.net_e.v.fill_(1.0)
    P.defreeze_evm_net(0)
    assert e.e_trainable and not e.net.m.any() and not e.net_e.v.any()
    assert e.net.m.numel() == theta.size and e.net_e.v.numel() == theta_e.size
    P.freeze_evm_net(1)
    np.testing.assert_array_equal(e.net.theta.numpy(), theta)
    np.testing.assert_array_equal(e.net_e.theta.numpy(), theta_e)
    np.testing.assert_array_equal(theta_e[e.P1:], s1)            # frozen throughout: its scale factors are the draw


def test_draw_is_seed_stable_and_leaves_the_global_generators_alone(monkeypatch):
    case = _case()
    e = _engine(monkeypatch, case, "ev")
    np.random.seed(11); torch.manual_seed(11)
    st_np, st_t = np.random.get_state(), torch.get_rng_state()
    e.set_weight_factorization(mean=1.0, std=0.1, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:], st_np[1:]))
    assert torch.equal(torch.get_rng_state(), st_t)
    a = [torch.cat(v).numpy().copy() for v in e.weight_factors().values()]
    e.set_weight_factorization(mean=1.0, std=0.1, seed=5)
    b = [torch.cat(v).numpy().copy() for v in e.weight_factors().values()]
    e.set_weight_factorization(mean=1.0, std=0.1, seed=6)
    c = [torch.cat(v).numpy().copy() for v in e.weight_factors().values()]
    for x, y, z, want in zip(a, b, c, rm.draw(5, 1.0, 0.1, [SHAPE, SHAPE_E])):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, want)
        assert (x != z).any()
    # pinned values: a change of the generator or of the drawing order shows here
    ref = np.random.Generator(np.random.Philox(key=5)).normal(1.0, 0.1, size=3).astype(np.float32)
    np.testing.assert_array_equal(a[0][:3], ref)
    allv = np.concatenate(a)
    assert abs(allv.mean() - 1.0) < 0.05 and 0.05 < allv.std() < 0.15


# ------------------------------------------------------------------ YAML and the sidecar
def _config_module():
    spec = importlib.util.spec_from_file_location(
        "ev_dropin_config_rwf", os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_yaml_key_is_absent_by_default_and_parses(tmp_path):
    cfg = _config_module()
    prod = cfg.ConfigManager.from_file(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                    "production.yaml"))
    assert not prod.config.training.weight_factorization.enabled
    assert "weight_factorization" not in open(os.path.join(ROOT, "nsfnet_amd", "dropin", "ev_nsfnet", "configs",
                                                           "production.yaml")).read()
    p = tmp_path / "c.yaml"
    p.write_text("training:\n  weight_factorization: {mean: 1.0, std: 0.2, seed: 4}\n")
    wf = cfg.ConfigManager.from_file(str(p)).config.training.weight_factorization
    assert (wf.enabled, wf.mean, wf.std, wf.seed) == (True, 1.0, 0.2, 4)
    p.write_text("training:\n  weight_factorization: {}\n")
    wf = cfg.ConfigManager.from_file(str(p)).config.training.weight_factorization
    assert (wf.enabled, wf.mean, wf.std, wf.seed) == (True, 0.5, 0.1, 0)
    p.write_text("training:\n  weight_factorization: {enabled: false, mean: 1.0}\n")
    assert not cfg.ConfigManager.from_file(str(p)).config.training.weight_factorization.enabled
    p.write_text("training:\n  N_f: 100\n")
    assert not cfg.ConfigManager.from_file(str(p)).config.training.weight_factorization.enabled
    p.write_text("training:\n  weight_factorization: {std: -0.1}\n")
    with pytest.raises(ValueError, match="weight_factorization"):
        cfg.ConfigManager.from_file(str(p))
    out = io.StringIO()
    p.write_text("training:\n  weight_factorization: {seed: 2}\n")
    with contextlib.redirect_stdout(out):
        cfg.ConfigManager.from_file(str(p)).print_config()
    assert "weight fact: mean=0.5 std=0.1 seed=2" in out.getvalue()


def test_sidecar_round_trips_and_the_checkpoint_keeps_the_reference_format(monkeypatch, tmp_path):
    import rwf_fakes
    rwf_fakes.install(monkeypatch)
    from nsfnet_amd import pinn_solver as ps
    monkeypatch.chdir(tmp_path)
    case = _case()

    def solver():
        torch.manual_seed(1)
        P = ps.PysicsInformedNeuralNetwork(Re=400, layers=L, hidden_size=H, N_f=70, bc_weight=10, device="cpu")
        P.set_boundary_data(X=(case["xb"], case["yb"], case["ub"], case["vb"]))
        P.set_eq_training_data(X=(case["x"], case["y"]))
        P.log_every = P.save_every = 0
        return P

    A = solver()
    A.save("off.pth", N_HLayer=L, N_neu=H, N_f=70)
    saved = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("off.pth")]
    assert len(saved) == 1                                   # no sidecar with the feature off
    A.set_weight_factorization(seed=8)
    with contextlib.redirect_stdout(io.StringIO()):
        A.train(num_epoch=3, lr=1e-3)
    A.save("on.pth", N_HLayer=L, N_neu=H, N_f=70)
    ck = [os.path.join(d, "on.pth") for d, _, fs in os.walk(str(tmp_path)) if "on.pth" in fs][0]
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    assert list(sd) == [k for k, _ in A.net.dev_net.keys_and_shapes()]            # the reference's keys, nothing else
    flat = torch.cat([sd[k].reshape(-1) for k in sd]).numpy()
    np.testing.assert_array_equal(flat, A.engine.net.params.numpy())             # the effective weights
    side = torch.load(ck + "_rwf", map_location="cpu", weights_only=True)
    s_A = torch.cat(A.engine.weight_factors()["net"]).numpy()
    assert list(side) == ["net"]
    np.testing.assert_array_equal(side["net"].numpy(), s_A)
    B = solver()                                             # the sidecar switches the feature on, with A's factors
    B.load(ck)
    np.testing.assert_array_equal(B.engine.net.params.numpy(), flat)
    np.testing.assert_array_equal(torch.cat(B.engine.weight_factors()["net"]).numpy(), s_A)
    np.testing.assert_array_equal(B.engine.net.theta.numpy(), rm.split(flat, s_A, SHAPE))
    C = solver()                                             # a feature-off run loads the checkpoint as any other
    C.net.load_state_dict(sd)
    assert C.engine.weight_factors() is None
    np.testing.assert_array_equal(C.engine.net.params.numpy(), flat)
