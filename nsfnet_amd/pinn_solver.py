"""Drop-in ``pinn_solver.PysicsInformedNeuralNetwork`` (sic) for the plain NSFnet flavour.

Same constructor keywords, methods and attributes as the reference class
(NSFnet/pinn_solver.py:26-389) so NSFnet/train.py and NSFnet/test.py run unchanged; the
per-step work (``fwd_computing_loss_2d`` + ``loss.backward()`` + ``opt.step()``,
pinn_solver.py:197-278) is executed by the HIP pipeline through nsfnet_amd.engine.
There is no torch-autograd or CPU fallback.
"""
import math
import os

import numpy as np
import scipy.io
import torch

from . import engine as _eng
from . import schedule as _schedule
from .net import FCNet


class AdamHandle:
    """What the scripts touch of torch.optim.Adam: ``param_groups[0]['lr']``
    (NSFnet/pinn_solver.py:235, ev-NSFnet/pinn_solver.py:437,497)."""

    def __init__(self, lr, betas=(0.9, 0.999), eps=1e-8):
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=0)]

    @property
    def lr(self):
        return self.param_groups[0]["lr"]


def is_lbfgs(opt):
    return isinstance(opt, torch.optim.LBFGS)


def lbfgs_knobs(opt):
    """PinnEngine.lbfgs_step keywords from a torch.optim.LBFGS (its param group carries every knob)."""
    g = opt.param_groups[0]
    return dict(lr=float(g["lr"]), max_iter=int(g["max_iter"]), max_eval=g["max_eval"],
                tolerance_grad=float(g["tolerance_grad"]), tolerance_change=float(g["tolerance_change"]),
                history_size=int(g["history_size"]), line_search_fn=g["line_search_fn"])


def _col(a):
    """numpy (N,1)/(N,) array or tensor -> contiguous float32 numpy vector."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))


def default_device():
    if not torch.cuda.is_available():
        raise RuntimeError("nsfnet_amd needs an MI355X (ROCm) device: the PINN hot path is a HIP pipeline "
                           "with no CPU fallback")
    return torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))


class SolverBase:
    """What the plain and the ev drop-in classes share: the knobs of the features the reference does not have
    (resampling, loss balancing) and the methods whose bodies are the same in both reference classes."""
    _balancing = False
    _confgrad = False
    _batching = False
    _attention = False
    _lr_schedule = None         # set_lr_schedule: the LrSchedule of every Adam stage without a scheduler= of its own
    _clipping = False
    _lr0 = None                 # the base rate of the running Adam stage while a device schedule is on
    _validation = False
    _val_patience = 0           # set_validation_data(patience=k): a stage ends at a log point with stale >= k
    _pseudo_time = False
    _early_stop = False         # set_early_stopping: solve_Adam leaves the stage at a log point once the monitor says so

    def set_resampling(self, every=0, k=1.0, c=1.0, seed=0):
        """every > 0: solve_Adam resamples before steps every, 2 every, ... of each train() call."""
        if int(every) < 0:
            raise ValueError("every must be >= 0")
        self._resampling = dict(every=int(every), k=float(k), c=float(c), seed=int(seed))

    def _maybe_resample(self, epoch_id):
        """The resampling cadence of solve_Adam / solve_LBFGS (set_resampling)."""
        rs = self._resampling
        if rs["every"] > 0 and epoch_id > 0 and epoch_id % rs["every"] == 0:
            self.resample_collocation(rs["k"], rs["c"], rs["seed"])

    def set_loss_balancing(self, every=0, beta=0.1):
        """every > 0: the boundary (and supervised) weight follows the learning-rate-annealing rule every `every` Adam
        updates (PinnEngine.set_loss_balancing).  alpha_b stays the configured weight (it names
        the checkpoint directory); the weight in use is lam_b().  every = 0: off."""
        self.engine.set_loss_balancing(every, beta)
        self._balancing = int(every) > 0

    def set_conflict_free_gradients(self, enabled=True):
        """enabled: every Adam update combines the per-term gradients (equations, boundary, supervised) by the ConFIG
        rule - equal positive projection on every term's unit gradient - instead of adding them
        (PinnEngine.set_conflict_free_gradients).  The configured weights stay in the terms and
        in the logged loss; print_log adds the term norms, their cosine and the coefficients.  An L-BFGS stage uses the
        plain sum.  Not together with set_loss_balancing.  False: off."""
        self.engine.set_conflict_free_gradients(enabled)
        self._confgrad = bool(enabled)

    def _confgrad_log(self):
        """The print_log suffix of the conflict-free combination (one host read, at log points only)."""
        i = self.engine.conflict_info()
        return "conflict-free: |g_r|=%.3e |g_b|=%.3e |g_s|=%.3e cos_rb=%+.3f k=(%.3e, %.3e, %.3e) fallbacks=%d/%d" % (
            i["n_r"], i["n_b"], i["n_s"], i["cos_rb"], i["k_r"], i["k_b"], i["k_s"], i["fallbacks"], i["steps"])

    def set_batching(self, batch_points=0, seed=0):
        """batch_points = B > 0: every Adam update evaluates the collocation term on a fresh random batch of B of this
        rank's collocation points, drawn on the device (PinnEngine.set_batching); call it after
        set_eq_training_data.  The loss terms published and logged are then those of the last batch, and eq*_pred (and
        evm / vis_t of the ev class) have the batch's length B after a batch step; x_f, y_f stay the whole store.  An
        L-BFGS stage ignores it (full batch).  The `batchsize` arguments of train / solve_Adam stay accepted and
        ignored.  batch_points = 0: off."""
        self.engine.set_batching(batch_points, seed)
        self._batching = int(batch_points) > 0

    def set_residual_attention(self, eta=0.0, gamma=0.999, init=1.0):
        """eta > 0: residual-based attention weights on this rank's collocation points (PinnEngine.
        set_residual_attention): every point carries a multiplier lam that follows
        lam <- gamma lam + eta |r| / max|r| after each Adam evaluation, and its loss weight is (SDF weight) lam^2; call
        it after set_eq_training_data.  The loss terms published and logged are then the weighted ones Adam minimises;
        print_log adds the range of lam and the unweighted equation loss.  An L-BFGS stage keeps the weights fixed.
        lam is not saved: checkpoints stay in the reference's format and a restored run restarts lam at init.
        eta = 0: off."""
        self.engine.set_residual_attention(eta, gamma, init)
        self._attention = float(eta) > 0.0

    def _attention_log(self):
        """The print_log suffix of the residual attention: the lam range and the unweighted equation loss."""
        a = self.engine.attention_info()
        return "attention lam: min=%.3e mean=%.3e max=%.3e  unweighted loss_e=%.3e" % (
            a["lam_min"], a["lam_mean"], a["lam_max"], a["loss_e"])

    def set_pseudo_time_stepping(self, dtau=None, every=0, pressure_dtau=None):
        """dtau > 0 and every >= 1: pseudo-time stepping of the equation loss (PinnEngine.set_pseudo_time; DESIGN.md
        section 7.11).  Every collocation point of this rank carries an anchor (u*, v*, p*) on the device, the
        momentum residuals gain (u - u*) / dtau and (v - v*) / dtau, the continuity residual (p - p*) / pressure_dtau
        (None: nothing), and after every `every` optimiser updates (Adam steps, L-BFGS calls) the anchors are refreshed
        from the current field.  Call it before set_eq_training_data (ValueError afterwards).  The loss terms published
        and logged are those the optimiser minimises; print_log adds the steady equation loss and the drift.  The
        anchors are not saved: load() re-anchors at the loaded weights.  Not together with mini-batching, resampling or
        chunked passes.  By default the collocation plan runs the 8-wave kernel families; PINN_PTIME_SPLIT=1 in the
        environment when the data are attached keeps the role-split, wide role-split and fused sweeps, in their
        pseudo-time variants.  dtau, every and pressure_dtau have no measured defaults.  dtau None or every 0: off."""
        self.engine.set_pseudo_time(dtau, every, pressure_dtau)
        self._pseudo_time = self.engine.pseudo_time_info() is not None

    def _pseudo_time_log(self):
        """The print_log suffix of the pseudo-time stepping (one host read, at log points only): this rank's record of
        the last update."""
        i = self.engine.pseudo_time_info()
        if i["steady_sums"] is None:
            return "pseudo-time: no collocation set yet"
        n = max(self.engine.n_f_global, 1)
        return ("pseudo-time (dtau=%g every=%d): steady loss_e(eq1..3)=%.3e drift_uv=%.3e drift_p=%.3e max|du|=%.3e "
                "since refresh=%d refreshes=%d" % (i["dtau"], i["every"], sum(i["steady_sums"]) / n, i["drift_uv"] / n,
                                                   i["drift_p"] / n, i["max_drift"], i["since_refresh"], i["refreshes"]))

    def set_lr_schedule(self, spec=None):
        """spec = an nsfnet_amd.schedule.LrSchedule: every Adam stage (train / solve_Adam) that is not given a
        scheduler= of its own runs under it, computed on the device (PinnEngine.set_lr_schedule; DESIGN.md section
        7.6): update e of the stage uses spec.value(lr, e) with lr the stage's rate, and every stage starts at e = 0.
        An L-BFGS stage ignores it.  None: off."""
        if spec is not None and not isinstance(spec, _schedule.LrSchedule):
            raise TypeError("set_lr_schedule: an LrSchedule or None (got %r)" % (spec,))
        self._lr_schedule = spec
        self.engine.set_lr_schedule(spec)

    def set_grad_clipping(self, max_norm=0.0):
        """max_norm > 0: every Adam update scales its gradient to a global 2-norm of at most max_norm, on the device
        (PinnEngine.set_grad_clipping; the formula of torch.nn.utils.clip_grad_norm_).  print_log adds the norm and
        the number of clipped updates.  An L-BFGS stage ignores it.  0: off."""
        self.engine.set_grad_clipping(max_norm)
        self._clipping = float(max_norm) > 0.0

    def set_weight_factorization(self, mean=0.5, std=0.1, seed=0, factors=None):
        """Random weight factorization of every Linear layer, W = diag(exp(s)) V with s and V trainable
        (PinnEngine.set_weight_factorization): s ~ Normal(mean, std) from a generator of its own
        seeded with `seed`, or the given `factors`.  Adam and L-BFGS then act on (V, b, s).  Checkpoints keep the
        reference's format - state_dict() is the effective weights - and save() adds the scale factors as a sidecar
        <checkpoint>_rwf, which load() reads back.  mean = None: off."""
        self.engine.set_weight_factorization(mean, std, seed, factors)

    def set_hard_boundary_constraints(self, enabled=True, lift_power=2, lid_sharpness=10.0, dataloader=None,
                                      origin=None, inv_len=None):
        """The cavity's wall values hold exactly, by the output transform u = g + D N_u, v = D N_v
        (PinnEngine.set_hard_boundary) instead of by the boundary penalty alone.  Call it before
        set_boundary_data / set_eq_training_data (ValueError once a point set is attached).  Where the unit cavity lies
        in the net's input coordinates comes from the data loader's coordinate map (dataloader.coord_transform:
        origin (-1, -1), inv_len 1/2; else origin (0, 0), inv_len 1), without a loader from this solver's coordinate
        scale, or from origin / inv_len where given.  lift_power's default 2 is a guess, not a measured optimum.  The
        boundary term keeps running and loss_b becomes a check of the constraint.  save() adds the descriptor as a
        sidecar <checkpoint>_hardbc, which load() reads back."""
        if origin is None or inv_len is None:
            if dataloader is not None:
                mapped = bool(getattr(dataloader, "coord_transform", False))
            else:
                scale = float(getattr(self, "coord_scale", 1.0))
                if scale not in (1.0, 2.0):
                    raise ValueError("hard boundary: coordinate scale %g is neither the plain cavity's nor the "
                                     "[-1, 1] map's; give origin and inv_len" % scale)
                mapped = scale == 2.0
            o, il = ((-1.0, -1.0), 0.5) if mapped else ((0.0, 0.0), 1.0)
            origin = o if origin is None else origin
            inv_len = il if inv_len is None else inv_len
        self.engine.set_hard_boundary(enabled, lift_power=lift_power, lid_sharpness=lid_sharpness, origin=origin,
                                      inv_len=inv_len)

    def set_fourier_features(self, sigma=1.0, seed=0, frequencies=None):
        """Random Fourier features as the main net's first layer, frozen (PinnEngine.set_fourier_features; DESIGN.md
        section 7.13): B ~ Normal(0, sigma^2) from a generator of its own seeded with `seed`, or the given
        `frequencies`.  Call it before set_boundary_data / set_eq_training_data (ValueError once a point set is
        attached).  Checkpoints keep the reference's format - layer 0's weights hold B - and save() adds the sidecar
        <checkpoint>_fourier (kind, sigma, seed), which load() reads back.  sigma's default 1.0 is a guess."""
        self.engine.set_fourier_features(sigma, seed, frequencies)

    def save_fourier_features(self, path):
        """Write the sidecar of the checkpoint at `path`: dict(kind, sigma, seed) as path + '_fourier' (torch.save).  With
        the option off nothing is written."""
        info = self.engine.fourier_info()
        if info is not None:
            torch.save(dict(kind=info["kind"], sigma=info["sigma"], seed=info["seed"]), path + '_fourier')

    def save_hard_boundary(self, path):
        """Write the sidecar of the checkpoint at `path`: the descriptor dict(lift_power, lid_sharpness, origin,
        inv_len) as path + '_hardbc' (torch.save).  With the constraint off nothing is written."""
        info = self.engine.hard_boundary_info()
        if info is not None:
            torch.save(dict(info, origin=tuple(info["origin"])), path + '_hardbc')

    def set_validation_data(self, x, y, u, v, p=None, every=1000, metric="uv", keep_best=True, patience=0,
                            history=4096):
        """Reference fields u, v (and p) at the points x, y - the DNS grid the run is judged on: after every `every`
        optimizer updates the relative L2 error against them is recorded on the device, and with keep_best the weights
        of the best validation so far are kept there too (PinnEngine.set_validation).  Nothing
        synchronises: validation_log(), validation_history() and best_state_dict() read when asked.  print_log adds
        the validation line; save() also writes the best weights (<filename>_best).  patience = k > 0: a training
        stage ends at a log point when the last k validations brought no improvement - the only place the loops read
        the monitor.  every = 0 or x = None: off."""
        if int(patience) < 0:
            raise ValueError("validation: patience must be >= 0")
        col = lambda a: None if a is None else _col(a)
        self.engine.set_validation(col(x), col(y), col(u), col(v), col(p), every=every, metric=metric,
                                   keep_best=keep_best, history=history)
        self._validation = self.engine.validation_info() is not None
        self._val_patience = int(patience) if self._validation else 0

    def validation_log(self):
        """One line on the validation monitor (one host read)."""
        i = self.engine.validation_info()
        if i is None or i["last"] is None:
            return "validation: no record yet"
        r = i["last"]
        return ("validation (t=%d): e_u=%.4e e_v=%.4e e_p=%.4e e_p0=%.4e  best %s=%.4e at t=%d  stale=%d nonfinite=%d "
                "records=%d" % (r["t"], r["e_u"], r["e_v"], r["e_p"], r["e_p0"], i["metric"], i["best_metric"],
                                i["best_t"], i["stale"], i["nonfinite"], i["records"]))

    def validation_history(self):
        """The recorded rows [t, e_u, e_v, e_p, e_p0, metric, improved, n_p] in time order (one host read)."""
        return self.engine.validation_history()

    def best_state_dict(self):
        """The main net's weights at the best validation so far (checkpoint format); None before the first."""
        return self.engine.best_state_dict()

    def load_best(self):
        """Put the best weights so far back into the nets (PinnEngine.restore_best); RuntimeError without any."""
        self.engine.restore_best()

    def _save_best(self, path):
        """Next to the checkpoint at `path`: <path>_best (and _best_evm, and the scale factors as <path>_best_rwf)
        when a best exists."""
        sd = self.engine.best_state_dict() if self._validation else None
        if sd is None:
            return
        torch.save(sd, path + '_best')
        sd_e = self.engine.best_state_dict_e()
        if sd_e is not None:
            torch.save(sd_e, path + '_best_evm')
        f = self.engine.best_factors()
        if f is not None:
            torch.save({name: torch.cat([a.detach().reshape(-1) for a in layers]).cpu() for name, layers in f.items()},
                       path + '_best_rwf')

    def _patience_out(self):
        """True when the stage should end: patience is set and that many validations brought no improvement (one
        host read; the loops ask at their log cadence only, on every rank - the records are identical)."""
        if not self._validation or self._val_patience <= 0:
            return False
        return self.engine.validation_info()["stale"] >= self._val_patience

    def set_early_stopping(self, every=1, window=1000, min_rel_improvement=1e-3, patience=3, re_eff_tol=None,
                           min_updates=0, quantity="loss", mode="any", history=4096):
        """End an Adam stage that has stopped making progress (PinnEngine.set_convergence_monitor; DESIGN.md section
        7.14): the device compares the means of `quantity` (and, with re_eff_tol, of Re_eff) over consecutive windows
        of `window` observed updates and sets a stop bit after `patience` windows in a row that improved by less than
        min_rel_improvement (changed by less than re_eff_tol); a non-finite loss stops at once.  solve_Adam reads the
        bits where it logs - on every rank, which all hold the same bits - and leaves the stage there with one line
        naming the reason and the update that set it; print_log adds the monitor line.  Every stage start resets the
        monitor (a resumed stage, start_epoch > 0, keeps it); solve_LBFGS neither observes nor asks.  The defaults are
        guesses: no value has been compared in training.  every = 0: off."""
        self.engine.set_convergence_monitor(every=every, window=window, min_rel_improvement=min_rel_improvement,
                                            patience=patience, re_eff_tol=re_eff_tol, min_updates=min_updates,
                                            quantity=quantity, mode=mode, history=history)
        self._early_stop = self.engine.monitor_info() is not None

    def _early_stop_begin(self, resume=False):
        """A stage start: the monitor starts over (not on a resumed stage, whose state load_training_state restored)."""
        if self._early_stop and not resume:
            self.engine.reset_convergence_monitor()

    def early_stop_log(self):
        """One line on the convergence monitor (one host read)."""
        i = self.engine.monitor_info()
        if i is None or i["last"] is None:
            return "early stop: no observation yet"
        return ("early stop (t=%d): %s window mean=%.4e Re_eff window mean=%.1f  windows=%d stale=%d settled=%d/%d "
                "nonfinite=%d  reasons=%s" % (i["last"]["t"], i["quantity"], i["window_mean"], i["window_mean_re"],
                                              i["windows"], i["stale"], i["settled"], i["patience"], i["nonfinite"],
                                              ",".join(i["reasons"]) or "-"))

    def monitor_history(self):
        """The observed rows [t, loss, loss_e, loss_b, loss_s, eq1..eq4, vis_mean, Re_eff, stop] in time order (one host
        read)."""
        return self.engine.monitor_history()

    def _early_stop_out(self, epoch_id=None):
        """True when the convergence monitor ends the stage (one host read; solve_Adam asks at its log cadence only, on
        every rank - the bits are identical).  Prints the reason and the update that set it."""
        if not self._early_stop:
            return False
        i = self.engine.monitor_info()
        if not i["should_stop"]:
            return False
        if getattr(self, "rank", 0) == 0:
            print("early stop%s: %s" % ("" if epoch_id is None else " after epoch %d" % (epoch_id + 1), "; ".join(
                "%s (set by update %d)" % (r, i["t_" + r]) for r in i["reasons"])))
        return True

    # ---- identification of the viscosity from data ----
    _identify = False           # set_viscosity_identification: print_log adds Re_est, save() writes the _visc sidecar

    def set_viscosity_identification(self, re0=None, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, re_bounds=(1e-2, 1e6),
                                     enabled=True):
        """Learn the Reynolds number along with the field (PinnEngine.set_viscosity_identification): nu = 1 / Re becomes
        a device scalar with its own Adam (rate `lr`) on ln nu, started at re0 (None: this solver's Re) and clamped to
        re_bounds.  It needs data that pin the flow down - supervised samples (the ev class's set_supervision_data) or
        boundary data that do - since the residual alone is minimised by any Re with a matching field.  self.Re keeps
        the configured value (checkpoint folders, vis_t0); print_log adds Re_est, save() writes the sidecar
        <checkpoint>_visc (the settings, the optimiser state and nu) and load() takes it up.  Held fixed during
        solve_LBFGS.  lr None or enabled False: off."""
        self.engine.set_viscosity_identification(re0=re0, lr=lr, betas=betas, eps=eps, re_bounds=re_bounds, enabled=enabled)
        self._identify = self.engine.viscosity_info() is not None

    def viscosity_log(self):
        """One line on the identified viscosity (one host read)."""
        i = self.engine.viscosity_info()
        return "Re_est=%.4f (nu=%.6e, d loss / d nu=%.3e, updates=%d, skipped=%d)" % (
            i["Re"], i["nu"], i["grad"], i["updates"], i["skipped"])

    # ---- continuation in the Reynolds number ----
    _recont = False             # set_reynolds_continuation: print_log adds Re_t

    def set_reynolds_continuation(self, re_start, updates, hold=0, shape="geometric", stairs=0, follow_vis_t0=True,
                                  enabled=True):
        """Ramp the viscosity from 1 / re_start down (or up) to that of this solver's Re over `updates` Adam updates,
        after `hold` updates at the start (PinnEngine.set_reynolds_continuation): the net follows the solution branch
        from a viscous, easy flow.  The position counts Adam updates on the device; it is not reset at a stage start
        and survives a re-created Adam, as the lr schedule position does.  Held during solve_LBFGS.  print_log adds
        Re_t; the training-state file carries the ramp, a finished ramp needs nothing.  enabled False: off."""
        self.engine.set_reynolds_continuation(re_start, updates, hold=hold, shape=shape, stairs=stairs,
                                              follow_vis_t0=follow_vis_t0, enabled=enabled)
        self._recont = self.engine.continuation_info() is not None

    def continuation_log(self):
        """One line on the ramp (one host read)."""
        i = self.engine.continuation_info()
        return "Re_t=%.4f (nu=%.6e%s, s=%.4f, updates=%d%s)" % (
            i["Re_t"], i["nu_t"], "" if i["cap_t"] is None else ", vis_t0=%.6e" % i["cap_t"], i["s"], i["t"],
            ", done" if i["done"] else "")

    # ---- flow diagnostics on the device ----
    _flow_diag = False          # set_flow_diagnostics: print_log adds the vortex line

    def set_flow_diagnostics(self, nx=257, ny=257, every=1000, eps=1e-3, history=4096, xs=None, ys=None, domain=None):
        """Record the primary vortex, the counter-rotating area of every quadrant, the mass defect and the kinetic
        energy, enstrophy and divergence of the net's field on an nx x ny tensor grid after every `every` optimizer
        updates, on the device (PinnEngine.set_flow_diagnostics): the numbers that tell the steady solutions apart
        without a reference field.  Nothing synchronises: flow_log() and flow_history() read when asked; print_log adds
        the vortex line.  every = 0: off."""
        self.engine.set_flow_diagnostics(nx=nx, ny=ny, every=every, eps=eps, history=history, xs=xs, ys=ys, domain=domain)
        self._flow_diag = self.engine.flow_info() is not None

    def flow_log(self):
        """One line on the flow diagnostics (one host read)."""
        i = self.engine.flow_info()
        if i is None or i["last"] is None:
            return "vortex: no record yet"
        r = i["last"]
        return "vortex (%.4f, %.4f) psi_min %.4f counter-area %.3f mass %.1e%s" % (
            r["x_c"], r["y_c"], r["psi_min"], r["counter_area"], r["mass_defect"],
            " nonfinite=%d" % r["nonfinite"] if r["nonfinite"] else "")

    def flow_history(self):
        """The recorded rows (engine.FLOW_ROW) in time order (one host read)."""
        return self.engine.flow_history()

    def save_viscosity(self, path):
        """Write the sidecar of the checkpoint at `path`: dict(re0, lr, betas, eps, re_bounds, state, nu) as path +
        '_visc' (torch.save).  With the identification off nothing is written."""
        vs = self.engine._visc
        if vs is not None:
            torch.save(dict(re0=vs.re0, lr=vs.lr, betas=tuple(vs.betas), eps=vs.eps, re_bounds=tuple(vs.re_bounds),
                            state=vs.state.cpu().tolist(), nu=float(vs.nu.cpu()[0])), path + '_visc')

    def _load_viscosity(self, path):
        """Take up the sidecar <path>_visc, if there is one: the identification is switched on with the saved settings
        and continues from the saved optimiser state and nu."""
        if not os.path.exists(path + '_visc'):
            return
        s = torch.load(path + '_visc', map_location="cpu", weights_only=True)
        self.set_viscosity_identification(re0=float(s["re0"]), lr=float(s["lr"]), betas=tuple(float(b) for b in s["betas"]),
                                          eps=float(s["eps"]), re_bounds=tuple(float(b) for b in s["re_bounds"]))
        vs = self.engine._visc
        vs.state.copy_(torch.tensor([float(v) for v in s["state"]], dtype=torch.float64))
        vs.nu.fill_(float(s["nu"]))

    def save_weight_factors(self, path):
        """Write the sidecar of the checkpoint at `path`: {net name: flat fp32 s} as path + '_rwf' (torch.save).  With
        the factorization off nothing is written."""
        f = self.engine.weight_factors()
        if f is not None:
            torch.save({name: torch.cat([a.detach().reshape(-1) for a in layers]).cpu() for name, layers in f.items()},
                       path + '_rwf')

    # ---- training-state checkpoints that resume bit for bit ----
    _ckpt_path, _ckpt_every = None, 0

    def set_checkpointing(self, path=None, every=0):
        """path and every > 0: after the update of every epoch with (epoch_id + 1) % every == 0, and after the last
        epoch of a train() call, write a non-blocking training-state snapshot to `path` whose `next_epoch` is
        epoch_id + 1 (save_training_state).  Off by default; path None or every 0: off."""
        every = int(every)
        if every < 0:
            raise ValueError("checkpointing: every must be >= 0")
        self._ckpt_path, self._ckpt_every = (path, every) if path and every else (None, 0)

    @staticmethod
    def _end_epoch(num_epoch, stop_epoch):
        """Where this call's loop ends: num_epoch, or stop_epoch when train() is told to cut the stage there."""
        return num_epoch if stop_epoch is None else min(num_epoch, int(stop_epoch))

    def _maybe_checkpoint(self, epoch_id, num_epoch, stop_epoch=None):
        last = epoch_id == self._end_epoch(num_epoch, stop_epoch) - 1
        if self._ckpt_path is not None and ((epoch_id + 1) % self._ckpt_every == 0 or last):
            self.save_training_state(self._ckpt_path, wait=False, next_epoch=epoch_id + 1, num_epoch=num_epoch)

    def save_training_state(self, path, wait=True, next_epoch=None, num_epoch=None):
        """PinnEngine.save_training_state with the loop position as `extra`: next_epoch and num_epoch (what
        train(start_epoch=...) continues from), stage / current_stage, global_step, the optimizer handle's lr, the
        running stage's base rate and alpha_evm."""
        opt = getattr(self, "opt", None)
        lr = None if opt is None or is_lbfgs(opt) else float(opt.param_groups[0]['lr'])
        extra = dict(next_epoch=next_epoch, num_epoch=num_epoch, stage=getattr(self, "stage", None),
                     current_stage=getattr(self, "current_stage", None), global_step=getattr(self, "global_step", None),
                     lr=lr, lr0=self._lr0, alpha_evm=getattr(self, "alpha_evm", None))
        self.engine.save_training_state(path, extra=extra, wait=wait)

    def load_training_state(self, path, strict=True):
        """PinnEngine.load_training_state, after every option and point set is attached as in the saving run.  Applies
        global_step, the handle's lr, the stage's base rate, alpha_evm and stage / current_stage from the file's `extra`
        and returns it: train(..., start_epoch=extra['next_epoch']) then continues the stage where it was cut."""
        fp = _eng._state_file.read_header(self.engine._state_path(path))["fingerprint"]
        if fp.get("schedule_or_clipping") and self.engine._opt is None:
            # the cut stage ran under a schedule given to its train() call: the device position needs its tensors now,
            # train(scheduler=..., start_epoch=k) installs the schedule itself and keeps the position
            self.engine.set_lr_schedule(_schedule.LrSchedule())
        extra = self.engine.load_training_state(path, strict=strict)["extra"]
        if extra.get("global_step") is not None:
            self.global_step = int(extra["global_step"])
        opt = getattr(self, "opt", None)
        if extra.get("lr") is not None and opt is not None and not is_lbfgs(opt):
            opt.param_groups[0]['lr'] = extra["lr"]
        self._lr0 = extra.get("lr0")
        if extra.get("alpha_evm") is not None and hasattr(self, "set_alpha_evm"):
            self.set_alpha_evm(extra["alpha_evm"])
        for key in ("stage", "current_stage"):
            if extra.get(key) is not None and hasattr(self, key):
                setattr(self, key, extra[key])
        return extra

    def load(self, path, path_evm=None):
        """Load a checkpoint written by save(): the main net's state_dict at `path` and, for the ev class, the entropy
        net's at path_evm (default <path>_evm when that file exists).  When the sidecar <path>_rwf is present the
        weight factorization is turned on with its scale factors (the effective weights are the checkpoint's exactly);
        without it the factorization state of this solver is left as it is.  The sidecar <path>_hardbc turns the hard
        wall conditions on with its descriptor: the checkpoint's weights are those of the net INSIDE the transform.  An
        engine that already holds plans must carry the same descriptor (ValueError otherwise)."""
        self.net.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
        net_1 = getattr(self, "net_1", None)
        if net_1 is not None:
            if path_evm is None and os.path.exists(path + '_evm'):
                path_evm = path + '_evm'
            if path_evm is not None:
                net_1.load_state_dict(torch.load(path_evm, map_location="cpu", weights_only=True))
        if os.path.exists(path + '_rwf'):
            self.engine.set_weight_factorization(factors=torch.load(path + '_rwf', map_location="cpu", weights_only=True))
        if os.path.exists(path + '_hardbc'):
            bc = torch.load(path + '_hardbc', map_location="cpu", weights_only=True)
            bc = dict(lift_power=int(bc["lift_power"]), lid_sharpness=float(bc["lid_sharpness"]),
                      origin=tuple(float(c) for c in bc["origin"]), inv_len=float(bc["inv_len"]))
            if self.engine.hard_boundary_info() != bc:
                try:
                    self.engine.set_hard_boundary(True, **bc)
                except ValueError as err:
                    raise ValueError("checkpoint %s was trained with hard wall conditions %r, this solver holds %r: %s"
                                     % (path, bc, self.engine.hard_boundary_info(), err))
        if os.path.exists(path + '_fourier'):
            ff = torch.load(path + '_fourier', map_location="cpu", weights_only=True)
            if ff.get("kind") != "sine":
                raise ValueError("checkpoint %s: unknown first-layer kind %r in its _fourier sidecar" % (path, ff.get("kind")))
            if self.engine.fourier_info() is None:
                # the checkpoint's layer 0 holds 2 pi B in its even rows: taken up as the frequencies, which rewrites
                # layer 0 with the values it has
                w0 = self.net.state_dict()["layers.layer_0.weight"].to(torch.float64)
                try:
                    self.engine.set_fourier_features(frequencies=w0[0::2] / (2.0 * math.pi))
                except ValueError as err:
                    raise ValueError("checkpoint %s was trained with a Fourier-feature first layer: %s" % (path, err))
                self.net.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))      # (bit for bit)
                self.engine._ff.update(sigma=ff.get("sigma"), seed=ff.get("seed"))
        if self._pseudo_time and self.engine.plan_f is not None:       # anchors are not checkpointed
            self.engine.reset_pseudo_time()
        self._load_viscosity(path)

    def _begin_adam_stage(self, scheduler, resume=False):
        """Resolve solve_Adam's scheduler= argument.  resume (train(start_epoch > 0)): the schedule object is installed
        but the device position is left where load_training_state put it.  An LrSchedule, or a torch.optim.lr_scheduler object of type
        MultiStepLR, StepLR, ExponentialLR or CosineAnnealingLR (translated once, from its own attributes), becomes
        the device schedule of this stage: an LrSchedule starts at e = 0 with the stage's rate as lr0, a torch object
        at e = its last_epoch with its base_lrs[0].  Returns the object whose step() the loop still calls - the torch
        one, so that its param_groups[0]['lr'] stays right, although the engine no longer consumes that value - or
        None.  Anything else is returned as it is and works as it always did: the loop reads the rate it sets."""
        lr0, e0, spec, stepper = self.opt.param_groups[0]['lr'], 0, self._lr_schedule, scheduler
        if isinstance(scheduler, _schedule.LrSchedule):
            spec, stepper = scheduler, None
        elif scheduler is not None:
            tr = _schedule.from_torch(scheduler)
            if tr is not None:
                spec, lr0, e0 = tr
            else:
                spec = None         # a host schedule the device does not know: the old path
        o = self.engine._opt
        if resume:
            if spec != (o.user_spec if o is not None else None):
                e0 = 0 if o is None else int(o.epoch.item())
                self.engine.set_lr_schedule(spec)
                self.engine.reset_lr_schedule(e0)
            self._lr0 = lr0 if spec is not None else None
            return stepper
        if spec is not (o.user_spec if o is not None else None):
            self.engine.set_lr_schedule(spec)
        self.engine.reset_lr_schedule(e0)
        self._lr0 = lr0 if spec is not None else None      # None: the loop passes the handle's current rate through
        return stepper

    def _adam_lr(self):
        """The rate solve_Adam hands to the engine: the stage's base rate under a device schedule, else the optimizer
        handle's current one (with clipping alone that one is the base rate of a constant schedule)."""
        return self._lr0 if self._lr0 is not None else self.opt.param_groups[0]['lr']

    def _optimizer_log(self):
        """The print_log suffix of the device schedule / clipping: lr_e of the last update and, with clipping on, the
        gradient norm and the clipped count (one host read, at log points only)."""
        i = self.engine.optimizer_info()
        out = "device lr=%.6e (epoch %d)" % (i["lr"], i["epoch"])
        if self._clipping:
            out += "  grad_norm=%.3e clip_coef=%.3e clipped=%d/%d" % (i["grad_norm"], i["clip_coef"], i["clipped"],
                                                                     i["updates"])
        return out

    def lam_b(self):
        """The boundary weight in use (one host read when balancing is on)."""
        if not self._balancing:
            return self.alpha_b
        return float(self.engine.loss_weights()[0])

    def set_optimizers(self, opt):
        self.opt = opt

    def set_eq_training_func(self, train_data_func):
        self.train_data_func = train_data_func

    def predict(self, net_params, X):
        x, y = X
        return self.neural_net_u(x, y)

    def divergence(self, x_star, y_star):
        return self.neural_net_equations(x_star, y_star)[2]


class PysicsInformedNeuralNetwork(SolverBase):
    # training_type:  'unsupervised' | 'half-supervised'  (kept for signature compatibility)
    def __init__(self,
                 opt=None,
                 Re=1000,
                 layers=4,
                 hidden_size=120,
                 N_f=40000,
                 stage=0,
                 learning_rate=0.001,
                 weight_decay=0.9,          # accepted and ignored, as in the reference (:76-79)
                 outlet_weight=1,
                 bc_weight=1,
                 eq_weight=1,
                 ic_weight=1,
                 num_ins=2,
                 num_outs=3,
                 supervised_data_weight=1,
                 training_type='unsupervised',
                 net_params=None,
                 checkpoint_freq=10000,
                 checkpoint_path='./checkpoint/',
                 device=None):
        self.device = torch.device(device) if device is not None else default_device()
        self.Re = Re
        self.vis_t0 = 5.0 / self.Re
        self.checkpoint_freq = checkpoint_freq
        self.checkpoint_path = checkpoint_path
        self.layers = layers
        self.hidden_size = hidden_size
        self.N_f = N_f
        self.training_type = training_type
        self.stage = stage
        self.alpha_b = bc_weight
        self.alpha_e = eq_weight
        self.alpha_i = ic_weight
        self.alpha_o = outlet_weight
        self.alpha_s = supervised_data_weight
        self.loss_i = self.loss_o = self.loss_b = self.loss_e = self.loss_s = 0.0
        if num_outs != 3:
            raise ValueError("num_outs must be 3 (u, v, p)")

        self.net = self.initialize_NN(num_ins=num_ins, num_outs=num_outs, num_layers=layers,
                                      hidden_size=hidden_size)
        if net_params:
            self.net.load_state_dict(torch.load(net_params, map_location="cpu", weights_only=True))
        self.engine = _eng.PinnEngine(self.device, layers, hidden_size, Re, alpha_b=bc_weight, alpha_e=eq_weight,
                                      flavour="nsfnet", net=self.net.dev_net)
        self.opt = AdamHandle(learning_rate) if not opt else opt
        self.x_f = self.y_f = self.x_b = self.y_b = self.u_b = self.v_b = None
        self._terms = None
        self.log_every, self.save_every = 1000, 10000
        self._resampling = dict(every=0, k=1.0, c=1.0, seed=0)

    # ---------------------------------------------------------------- data
    def set_boundary_data(self, X=None, time=False):
        """X = (x_b, y_b, u_b, v_b), numpy (N,1) float64 (NSFnet/train.py:47-48; solver :82-90)."""
        self.x_b, self.y_b, self.u_b, self.v_b = (torch.as_tensor(_col(a)).reshape(-1, 1).to(self.device)
                                                  for a in X[:4])
        self.engine.set_boundary(_col(X[0]), _col(X[1]), _col(X[2]), _col(X[3]))

    def set_eq_training_data(self, X=None, time=False):
        """X = (x_f, y_f) collocation points (solver :92-99)."""
        self.x_f = torch.as_tensor(_col(X[0])).reshape(-1, 1).to(self.device)
        self.y_f = torch.as_tensor(_col(X[1])).reshape(-1, 1).to(self.device)
        self.engine.set_collocation(_col(X[0]), _col(X[1]))

    # ---------------------------------------------------------------- residual-based resampling
    def set_resample_pool(self, X, weights=None):
        """X = (x, y) candidate points for resample_collocation (e.g. a larger LHS draw than the collocation set)."""
        self.engine.set_resample_pool(_col(X[0]), _col(X[1]), None if weights is None else _col(weights))

    def resample_collocation(self, k=1.0, c=1.0, seed=None):
        """Redraw the collocation points from the pool with density |r|^k / mean|r|^k + c (PinnEngine.resample);
        seed None: the one given to set_resampling.  Returns the selected pool indices."""
        idx = self.engine.resample(k, c, self._resampling["seed"] if seed is None else seed)
        x, y, _ = self.engine.collocation_points()
        self.x_f, self.y_f = x.reshape(-1, 1), y.reshape(-1, 1)
        return idx

    def set_validation_data(self, x, y, u, v, every=1000, metric="uv", keep_best=True, patience=0, history=4096):
        """SolverBase.set_validation_data without pressure targets (the plain flavour's DNS comparison has none)."""
        super().set_validation_data(x, y, u, v, None, every=every, metric=metric, keep_best=keep_best,
                                    patience=patience, history=history)

    def set_stage(self, stage):
        self.stage = stage

    def initialize_NN(self, num_ins=2, num_outs=4, num_layers=6, hidden_size=160):
        return FCNet(num_ins=num_ins, num_outs=num_outs, num_layers=num_layers, hidden_size=hidden_size,
                     activation=torch.nn.Tanh, device=self.device)

    # ---------------------------------------------------------------- model evaluation
    def neural_net_u(self, x, y):
        """u, v, p as (N,1) device tensors (solver :124-130)."""
        u, v, p = self.engine.predict(_col(x), _col(y))
        return u.reshape(-1, 1), v.reshape(-1, 1), p.reshape(-1, 1)

    def neural_net_equations(self, x, y):
        """eq1, eq2, eq3 at arbitrary points (solver :132-163), forward only.  With viscosity identification on they are
        formed at the identified viscosity, the one training minimises them at, not at self.Re."""
        plan = _eng.ResidualPlan(self.engine.net, _col(x), _col(y), with_backward=False)
        if self.engine._visc is not None:
            plan.set_viscosity(self.engine._visc.nu, with_lap=False)
        plan.forward(self.Re, save=False)
        return tuple(plan.field(k).reshape(-1, 1).clone() for k in ("eq1", "eq2", "eq3"))

    # ---------------------------------------------------------------- loss / step
    def _publish_terms(self, loss_mode="MSE"):
        t = self.engine.loss_terms(loss_mode)
        f, _ = self.engine.eval_plans()        # the batch plan after a batch step (set_batching)
        self.loss_eq1, self.loss_eq2, self.loss_eq3 = t["loss_eq1"], t["loss_eq2"], t["loss_eq3"]
        self.loss_e, self.loss_b, self.loss = t["loss_e"], t["loss_b"], t["loss"]
        self.eq1_pred, self.eq2_pred, self.eq3_pred = (f.field(k).reshape(-1, 1) for k in ("eq1", "eq2", "eq3"))
        b = self.engine.plan_b
        self.u_pred_b, self.v_pred_b = b.pred[0].reshape(-1, 1), b.pred[1].reshape(-1, 1)
        return t

    def fwd_computing_loss_2d(self, loss_mode='MSE', full_batch=False):
        """Loss of the current parameters AND its parameter gradient (the HIP pipeline fuses
        what the reference splits into this call and ``loss.backward()``, solver :197-226,252).
        Returns (loss, [loss_e, loss_b]) as 0-dim device tensors."""
        assert self.x_f is not None and self.y_f is not None
        # 'L2' (solver :202-204, :214-217; no script of the reference selects it): 2-norms of the residual and
        # boundary-misfit vectors instead of mean squares - same kernels, other adjoint coefficients (an unknown
        # mode raises ValueError)
        self.engine.loss_and_grad(loss_mode, full_batch=full_batch)     # full_batch: the store although set_batching is on
        self._publish_terms(loss_mode)
        return self.loss, [self.loss_e, self.loss_b]

    def train(self, num_epoch=1, lr=1e-4, optimizer=None, scheduler=None, batchsize=None, start_epoch=0, stop_epoch=None):
        """start_epoch = k > 0 (after load_training_state): the stage's loop runs epochs k .. num_epoch - 1 and does
        none of its stage-start resets; the per-epoch cadences keep keying on epoch_id.  stop_epoch: cut the stage
        there (the loop ends before that epoch; with set_checkpointing on, the last epoch run writes a snapshot)."""
        if is_lbfgs(optimizer):
            self.opt = optimizer
        self.opt.param_groups[0]['lr'] = lr
        if is_lbfgs(self.opt):
            return self.solve_LBFGS(self.fwd_computing_loss_2d, num_epoch, batchsize, scheduler, start_epoch, stop_epoch)
        return self.solve_Adam(self.fwd_computing_loss_2d, num_epoch, batchsize, scheduler, start_epoch, stop_epoch)

    def solve_LBFGS(self, loss_func, num_epoch=1, batchsize=None, scheduler=None, start_epoch=0, stop_epoch=None):
        """One epoch = one torch.optim.LBFGS.step(closure) of self.opt's knobs on the device (PinnEngine.lbfgs_step);
        logging, checkpoints and resampling keep solve_Adam's per-epoch cadence (a resample resets the history)."""
        print('--------')
        print(num_epoch)
        print('--------')
        log_now = save_now = False
        for epoch_id in range(int(start_epoch), self._end_epoch(num_epoch, stop_epoch)):
            self._maybe_resample(epoch_id)
            self.engine.lbfgs_step(owner=self.opt, **lbfgs_knobs(self.opt))   # a new LBFGS object starts fresh
            if scheduler is not None and not isinstance(scheduler, _schedule.LrSchedule):
                scheduler.step()
            self._maybe_checkpoint(epoch_id, num_epoch, stop_epoch)
            log_now = self.log_every and epoch_id % self.log_every == 0
            save_now = self.save_every and epoch_id % self.save_every == 0
            if log_now or save_now:
                # the field planes are the last TRIAL point's after a line search: evaluate the accepted one
                self.fwd_computing_loss_2d(full_batch=True)
            if log_now:
                self.print_log(self.loss, [self.loss_e, self.loss_b], epoch_id, num_epoch)
            if save_now:
                self.save('model_cavity_loop_%d.pth' % epoch_id, N_HLayer=self.layers, N_neu=self.hidden_size,
                          N_f=self.N_f)
            if log_now and self._patience_out():
                break
        if num_epoch > 0 and not (log_now or save_now):
            self.fwd_computing_loss_2d(full_batch=True)         # terms and fields of the accepted point

    def solve_Adam(self, loss_func, num_epoch=1000, batchsize=None, scheduler=None, start_epoch=0, stop_epoch=None):
        """The reference loop (solver :240-278): loss -> backward -> Adam step; log every 1000,
        checkpoint every 10000 (incl. step 0).  Adam moments persist across calls."""
        fused = getattr(loss_func, "__func__", None) is PysicsInformedNeuralNetwork.fwd_computing_loss_2d
        scheduler = self._begin_adam_stage(scheduler, resume=start_epoch > 0)
        self._early_stop_begin(resume=start_epoch > 0)
        epoch_id, end_epoch = int(start_epoch), self._end_epoch(num_epoch, stop_epoch)
        print('--------')
        print(num_epoch)
        print('--------')
        while epoch_id < end_epoch:
            self._maybe_resample(epoch_id)
            lr = self._adam_lr()
            log_now = self.log_every and epoch_id % self.log_every == 0
            save_now = self.save_every and epoch_id % self.save_every == 0
            if fused and not (log_now or save_now):
                self.engine.step(lr)                 # no host sync; one hipGraph replay on a single GPU
            else:
                loss, losses = loss_func()
                self.engine.adam_step(lr)
            if scheduler:
                scheduler.step()
            self._maybe_checkpoint(epoch_id, num_epoch, stop_epoch)
            if log_now:
                self.print_log(self.loss, [self.loss_e, self.loss_b], epoch_id, num_epoch)
            if save_now:
                self.save('model_cavity_loop_%d.pth' % epoch_id, N_HLayer=self.layers, N_neu=self.hidden_size,
                          N_f=self.N_f)
            if log_now and (self._patience_out() or self._early_stop_out(epoch_id)):
                break
            epoch_id += 1
        self._publish_terms()

    def print_log(self, loss, losses, epoch_id, num_epoch):
        print("current lr is: %.6f " % (self.opt.param_groups[0]['lr']),
              "epoch/num_epoch: ", epoch_id + 1, "/", num_epoch,
              "eq1_loss: %.3e " % (self.loss_eq1.item()),
              "eq2_loss: %.3e " % (self.loss_eq2.item()),
              "eq4_loss: %.3e \n" % (self.loss_eq3.item()),
              *(("lambda_b: %.4e" % self.lam_b(),) if self._balancing else ()),
              *(("(losses of the last batch of %d points)" % self.engine.batch_info()["batch_points"],)
                if self._batching and self.engine.evaluated_batch else ()),
              *(("\n" + self._attention_log(),) if self._attention else ()),
              *(("\n" + self._pseudo_time_log(),) if self._pseudo_time else ()),
              *(("\n" + self._confgrad_log(),) if self._confgrad else ()),
              *(("\n" + self._optimizer_log(),) if self.engine._opt is not None else ()),
              *(("\n" + self.validation_log(),) if self._validation else ()),
              *(("\n" + self.early_stop_log(),) if self._early_stop else ()),
              *(("\n" + self.viscosity_log(),) if self._identify else ()),
              *(("\n" + self.continuation_log(),) if self._recont else ()),
              *(("\n" + self.flow_log(),) if self._flow_diag else ()))

    # ---------------------------------------------------------------- evaluation / io
    def _errors(self, x, y, u, v):
        u_pred, v_pred, p_pred = (t.cpu().numpy().reshape(-1, 1) for t in self.neural_net_u(x, y))
        u_test, v_test = np.asarray(u).reshape(-1, 1), np.asarray(v).reshape(-1, 1)
        error_u = np.linalg.norm(u_test - u_pred, 2) / np.linalg.norm(u_test, 2)
        error_v = np.linalg.norm(v_test - v_pred, 2) / np.linalg.norm(v_test, 2)
        return error_u, error_v, u_pred, v_pred, p_pred

    def evaluate(self, x, y, u, v):
        """Relative L2 errors on the DNS grid (solver :308-325)."""
        error_u, error_v, *_ = self._errors(x, y, u, v)
        print('------------------------')
        print('Error u: %e' % (error_u))
        print('Error v: %e' % (error_v))
        return error_u, error_v

    def test(self, x, y, u, v, loop=None):
        """Errors + savemat of the predicted fields (solver :327-357).  The grid shape is taken
        from the inputs (the reference hard-codes 257x257, which breaks on the 385^2 Re4000 file)."""
        error_u, error_v, u_pred, v_pred, p_pred = self._errors(x, y, u, v)
        print('------------------------')
        print('Error u: %e' % (error_u))
        print('Error v: %e' % (error_v))
        print('------------------------')
        shape = np.asarray(x).shape if np.asarray(x).ndim == 2 and np.asarray(x).shape[1] > 1 else None
        if shape is None:
            side = int(round(np.sqrt(u_pred.size)))
            shape = (side, side) if side * side == u_pred.size else (u_pred.size, 1)
        scipy.io.savemat('cavity_result_loop_%d.mat' % (loop),
                         {'U_pred': u_pred.reshape(shape), 'V_pred': v_pred.reshape(shape),
                          'P_pred': p_pred.reshape(shape), 'lam_bcs': self.lam_b(), 'lam_equ': self.alpha_e})
        return error_u, error_v

    def save(self, filename, directory=None, N_HLayer=None, N_neu=None, N_f=None, lr=None):
        """Reference checkpoint layout (solver :359-380):
        results/Re{Re}/{L}x{H}_Nf{N/1000}k_lamB{alpha_b}{stage}/<filename> = net.state_dict()."""
        Re_folder = 'Re' + str(self.Re)
        NNsize = str(N_HLayer) + 'x' + str(N_neu) + '_Nf' + str(np.int32(N_f / 1000)) + 'k'
        lambdas = 'lamB' + str(self.alpha_b)
        relative_path = '/results/' + Re_folder + '/' + NNsize + '_' + lambdas + str(self.stage) + '/'
        if not directory:
            directory = os.getcwd()
        save_results_to = directory + relative_path
        os.makedirs(save_results_to, exist_ok=True)
        torch.save(self.net.state_dict(), save_results_to + filename)
        self.save_weight_factors(save_results_to + filename)
        self.save_hard_boundary(save_results_to + filename)
        self.save_fourier_features(save_results_to + filename)
        self.save_viscosity(save_results_to + filename)
        self._save_best(save_results_to + filename)
        save_matlab_to = directory + '/loss/'
        os.makedirs(save_matlab_to, exist_ok=True)
        if getattr(self, "loss_eq1", None) is not None:
            scipy.io.savemat(save_matlab_to + 'eq_losses.mat',
                             {'eq1': self.loss_eq1.item(), 'eq2': self.loss_eq2.item(), 'eq3': self.loss_eq3.item()})
