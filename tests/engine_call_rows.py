"""The rows of tests/golden/engine_call_logs.json (TEST INFRASTRUCTURE): one PinnEngine per row on the oracle-backed
fakes, driven through step / loss_and_grad + adam_step / lbfgs_step, with every device entry point it reaches logged
together with its launch arguments (names, counts and floats: no computed result), and of
tests/golden/engine_state_headers.json: what a training-state file of the driven engine would say of itself.
scripts/record_engine_calls.py writes the fixtures from these rows and tests/test_engine_call_logs.py rebuilds them.
Nothing here is reachable from the product path."""
import hashlib
import json

import numpy as np
import pytest
import torch

import confgrad_fakes
import ptime_model
import visc_fakes
from nsfnet_amd import engine as eng
from nsfnet_amd.schedule import LrSchedule

L, H, RE, N, NB, LR = 2, 8, 400.0, 300, 40, 2.0 ** -10
SPIED = ("grad_reduce", "grad_reduce_terms", "balance_stats", "balance_update", "balance_combine", "confgrad_gram",
         "confgrad_coef", "confgrad_combine", "batch_draw", "batch_scatter", "rba_stats", "rba_apply", "rba_fill",
         "grad_sqnorm", "ptime_advance", "val_stats", "val_keep", "monitor_vis_stats", "monitor_observe", "visc_grad",
         "visc_update")
CONFGRAD = ("grad_reduce_terms", "confgrad_partials", "confgrad_gram", "confgrad_coef", "confgrad_combine")

_BAL = dict(balance=dict(every=2, beta=0.1))
_ALL = dict(_BAL, batch=100, attention=dict(eta=0.01, gamma=0.999), clip=0.5, rwf=3)
OPTIONS = [("plain", {}), ("balance", _BAL), ("confgrad", dict(confgrad=True)), ("batch", dict(batch=100)),
           ("attention", dict(attention=dict(eta=0.01, gamma=0.999))),
           ("sched_clip", dict(schedule=dict(kind="cosine", t_max=10, eta_min=1e-5), clip=0.5)), ("rwf", dict(rwf=3)),
           ("all_balance", _ALL), ("confgrad_clip_rwf", dict(confgrad=True, clip=0.5, rwf=3))]
ROWS = [dict(name="%s-%s" % (flavour, name), flavour=flavour, opts=opts)
        for name, opts in OPTIONS for flavour in ("nsfnet", "ev")]
for _name, _opts in OPTIONS[:3]:
    ROWS.append(dict(name="chunked-" + _name, flavour="nsfnet", opts=_opts, chunk=128))
    ROWS.append(dict(name="supervised-" + _name, flavour="nsfnet", opts=_opts, sup=True))
_VAL, _MON = dict(validation=dict(n=16, every=2)), dict(monitor=dict(every=1, window=2))
LATER = [("ptime", dict(ptime=dict(dtau=0.5, every=2, pressure_dtau=2.0))), ("validation", _VAL), ("monitor", _MON),
         ("visc", dict(visc={})), ("attention_sched_clip_validation_monitor", dict(OPTIONS[4][1], **OPTIONS[5][1], **_VAL, **_MON))]
ROWS += [dict(name="%s-%s" % (flavour, name), flavour=flavour, opts=opts)
         for name, opts in LATER for flavour in ("nsfnet", "ev")]


def _brief(a):
    """A launch argument as the fixture holds it: scalars as they are, a tensor as its size, an object as its class."""
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if isinstance(a, torch.Tensor):
        return "t%d" % a.numel()
    if isinstance(a, (list, tuple)):
        return [_brief(v) for v in a]
    if isinstance(a, dict):
        return [[k, _brief(a[k])] for k in sorted(a)]
    return type(a).__name__


def _entry(name, a, k):
    return [name] + [_brief(v) for v in a] + [[key, _brief(k[key])] for key in sorted(k)]


def _spy(log, name, fn):
    def wrapper(*a, **k):
        log.append(_entry(name, a, k))
        return fn(*a, **k)
    return wrapper


def _spy_plan(log, base, name):
    class Spy(base):
        def forward(self, *a, **k):
            log.append(_entry(name + ".forward", (self.n,) + a, k))
            return super().forward(*a, **k)

        def backward(self, *a, **k):
            log.append(_entry(name + ".backward", (self.n,) + a, k))
            return super().backward(*a, **k)
    Spy.__name__ = name
    return Spy


class PtimeResidualPlan(visc_fakes.ViscResidualPlan):
    """The residual plan of the fakes stack with the anchors and the rates of the pseudo-time stepping.  Its sums and
    gradient stay the steady term's: the rows pin which launches the engine makes, not what they compute."""
    anchor = None

    def __init__(self, net, x, y, weights=None, with_backward=True, ws=None, pseudo_time=False):
        super().__init__(net, x, y, weights, with_backward, ws)
        self.is_pseudo_time = pseudo_time

    def set_pseudo_time(self, sigma, sigma_p):
        assert self.is_pseudo_time
        if self.anchor is None:
            self.anchor = torch.zeros(3, self.npad)
        self.rates = (float(sigma), float(sigma_p))


def _ptime_advance(plan, every, force, scratch, record):
    anchor, rec = ptime_model.advance(plan.fields.numpy(), plan.n, plan.anchor.numpy(), every, force,
                                      None if plan.w is None else plan.w.numpy(), record.numpy())
    plan.anchor.copy_(torch.tensor(anchor))
    record.copy_(torch.tensor(rec))


def install(mp):
    """The whole fakes stack (visc_fakes: monitor, training state and validation on the factorization, the optimiser
    options and the rest) with the conflict-free-gradient entry points of confgrad_fakes and a pseudo-time plan and
    advance on top (all log into one list), logging plans, and a spy with the launch arguments around every entry point
    of SPIED.  Returns the log."""
    visc_fakes.install(mp)
    log = visc_fakes.CALLS
    mp.setattr(confgrad_fakes, "CALLS", log)
    for name in CONFGRAD:
        mp.setattr(eng, name, getattr(confgrad_fakes, "fake_" + name))
    mp.setattr(eng, "ptime_scratch", lambda n, device: torch.zeros(8, dtype=torch.float64))
    mp.setattr(eng, "ptime_advance", _ptime_advance)
    mp.setattr(eng, "ResidualPlan", _spy_plan(log, PtimeResidualPlan, "FakeResidualPlan"))
    mp.setattr(eng, "ValuePlan", _spy_plan(log, eng.ValuePlan, "FakeValuePlan"))
    for name in SPIED:
        mp.setattr(eng, name, _spy(log, name, getattr(eng, name)))
    return log


def engine(row):
    """The row's engine (install() first): a 2x8 net, 300 collocation and 40 boundary points, the options set."""
    from oracle import autograd_ref as ar
    o = row["opts"]
    ev = row["flavour"] == "ev"
    kw = dict(flavour="ev", n_hidden_e=2, hidden_e=6, alpha_evm=0.05) if ev else {}
    e = eng.PinnEngine("cpu", L, H, RE, alpha_b=10.0, alpha_e=1.0, alpha_s=2.0 if row.get("sup") else 0.0, **kw)
    rng = np.random.RandomState(5)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.3, dtype=torch.float32))
    if ev:
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.3, dtype=torch.float32))
        e.e_trainable = True
    x, y = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    xb, yb, ub, vb = (a.reshape(-1)[::51][:NB] for a in ar.cavity_boundary())
    if "ptime" in o:
        e.set_pseudo_time(**o["ptime"])
    e.set_collocation(x, y, chunk_points=row.get("chunk"))
    e.set_boundary(xb, yb, ub, vb)
    if row.get("sup"):
        xs, ys = rng.rand(9).astype(np.float32), rng.rand(9).astype(np.float32)
        e.set_supervised(xs, ys, np.sin(xs), np.cos(ys), xs * ys)
    if "attention" in o:
        e.set_residual_attention(**o["attention"])
    if "batch" in o:
        e.set_batching(o["batch"], seed=7)
    if "balance" in o:
        e.set_loss_balancing(**o["balance"])
    if o.get("confgrad"):
        e.set_conflict_free_gradients()
    if "schedule" in o:
        e.set_lr_schedule(LrSchedule(**o["schedule"]))
    if "clip" in o:
        e.set_grad_clipping(o["clip"])
    if "rwf" in o:
        e.set_weight_factorization(seed=o["rwf"])
    if "validation" in o:       # (the later rows draw after everything the earlier ones drew)
        xv, yv = (rng.rand(o["validation"]["n"]).astype(np.float32) for _ in range(2))
        e.set_validation(xv, yv, np.sin(xv), np.cos(yv), every=o["validation"]["every"])
    if "monitor" in o:
        e.set_convergence_monitor(**o["monitor"])
    if "visc" in o:
        e.set_viscosity_identification(**o["visc"])
    return e


def drive(e):
    for _ in range(3):
        e.step(LR)
    e.loss_and_grad(full_batch=True)
    e.adam_step(LR)
    e.lbfgs_step(max_iter=2, line_search_fn="strong_wolfe")
    e.step(LR)


def graph_key(mp, e):
    """The graph key step() looks up (the probe of test_rwf_cpu.py)."""
    keys = []

    class Stop(Exception):
        pass

    class Probe(dict):
        def get(self, key, default=None):
            keys.append(key)
            raise Stop

        def clear(self):
            pass

    old = e._graphs
    with mp.context() as m:
        m.setattr(e, "_graphs_enabled", lambda: True)
        e._graphs = Probe()
        with pytest.raises(Stop):
            e.step(LR)
        e._graphs = old
    return keys[0]


def graph_keys(mp, e):
    """The key of the next step; with balancing on, the keys of an update step and of a plain one."""
    if e._bal is None:
        return [graph_key(mp, e)]
    keys = []
    for n in (e._bal.every, e._bal.every + 1):
        e._bal.n, e._bal.done = n, -1
        keys.append(graph_key(mp, e))
    return keys


def _sha(t):
    return None if t is None else hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]


def state_hashes(e):
    """Hashes of the parameters and of every option's record tensors (for a by-hand comparison of two commits)."""
    recs = [getattr(st, k, None) for st in (e._bal, e._cfg, e._rba, e._opt) if st is not None
            for k in ("rec", "lam", "coef", "w")]
    return dict(params=_sha(e.net.params), params_e=_sha(None if e.net_e is None else e.net_e.params),
                flat=_sha(e.flat), records=[_sha(t) for t in recs])


def state_header(e):
    """What save_training_state would put into the file's header: the fingerprint, the settings, the host mirrors
    (without the two floats of the L-BFGS state) and per segment [name, dtype, shape, bytes, stored].  No digests: they
    hash floating-point results of the host's BLAS.  The offsets follow from the bytes (state_file.layout)."""
    host = e._state_host()
    if host["lbfgs"] is not None:
        host["lbfgs"] = host["lbfgs"][:2]
    segs = [[name, str(t.dtype).replace("torch.", ""), list(t.shape), t.numel() * t.element_size(), stored]
            for name, t, stored in e._state_segments()]
    return dict(fingerprint=e._state_fingerprint(), info=e._state_info(), host=host, segments=segs)


def run(row, hashes=False):
    """(call log, graph keys, state header[, state hashes]) of one row, as JSON gives them back."""
    with pytest.MonkeyPatch.context() as mp:
        log = install(mp)
        e = engine(row)
        del log[:]
        drive(e)
        out = [list(log), None, state_header(e)]
        h = state_hashes(e) if hashes else None
        out[1] = graph_keys(mp, e)
    out = json.loads(json.dumps(out))
    return tuple(out) + ((h,) if hashes else ())
