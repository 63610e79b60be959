"""YAML-backed run configuration with the attribute tree ev-NSFnet/train.py reads
(config.py:9-178: cfg.physics / cfg.network / cfg.training{.sdf_weighting,.training_stages} /
cfg.supervision, ConfigManager.from_file / print_config / validate_config)."""
from dataclasses import dataclass, field, fields, is_dataclass
from typing import List, Optional

import yaml


@dataclass
class PhysicsConfig:
    Re: int = 5000
    alpha_evm: float = 0.05
    bc_weight: float = 10.0
    eq_weight: float = 1.0


@dataclass
class FourierFeaturesConfig:
    """Random Fourier features as the main net's first layer, frozen (PinnEngine.set_fourier_features):
    `network.fourier_features: {sigma: 1.0, seed: 0}`.  Absent (the default): off.  sigma's default is a guess."""
    sigma: float = 1.0
    seed: int = 0


@dataclass
class NetworkConfig:
    layers: int = 6
    layers_1: int = 4
    hidden_size: int = 80
    hidden_size_1: int = 40
    fourier_features: Optional[FourierFeaturesConfig] = None      # absent = off


@dataclass
class TrainingStage:
    alpha: float
    epochs: int
    lr: float
    name: str
    optimizer: str = "adam"             # adam | lbfgs (lbfgs: epochs = L-BFGS iterations, lr = step scale)
    history_size: int = 100             # lbfgs only
    line_search: str = "strong_wolfe"   # lbfgs only: strong_wolfe | none
    # adam only: the learning-rate schedule of the stage, computed on the device (PinnEngine.set_lr_schedule).  lr is
    # its base rate and the stage's first update is epoch 0.
    scheduler: str = "constant"         # constant | multistep | step | exponential | cosine
    milestones: List[int] = field(default_factory=list)    # multistep: at most 16, ascending
    gamma: float = 0.1                  # multistep / step / exponential
    step_size: int = 1                  # step
    t_max: int = 0                      # cosine; 0 = the stage's epochs
    eta_min: float = 0.0                # cosine
    warmup_epochs: int = 0              # > 0: linear warm-up from warmup_start * lr over that many updates
    warmup_start: float = 0.0

    def schedule_args(self, epochs_scale=1.0):
        """Keyword arguments of nsfnet_amd.schedule.LrSchedule for this stage, every count scaled like epochs."""
        n = lambda v, lo: max(lo, int(v * epochs_scale))
        epochs = n(self.epochs, 1)
        return dict(kind=self.scheduler, milestones=tuple(n(m, 0) for m in self.milestones), gamma=self.gamma,
                    step_size=n(self.step_size, 1), t_max=n(self.t_max, 1) if self.t_max > 0 else epochs,
                    eta_min=self.eta_min, warmup_epochs=n(self.warmup_epochs, 0), warmup_start=self.warmup_start)


@dataclass
class SupervisionConfig:
    enabled: bool = False
    num_samples: int = 0
    loss_weight: float = 1.0


@dataclass
class SDFWeightConfig:
    enabled: bool = False
    min_weight: float = 0.2
    decay: float = 5.0


@dataclass
class ResamplingConfig:
    """Residual-based redraw of the collocation points from a larger pool (PinnEngine.resample), off by default."""
    enabled: bool = False
    every: int = 5000
    pool_points: int = 1000000
    k: float = 1.0
    c: float = 1.0
    seed: int = 0


@dataclass
class LossBalancingConfig:
    """Adaptive boundary / supervised loss weights (PinnEngine.set_loss_balancing), off by default."""
    enabled: bool = False
    every: int = 100
    beta: float = 0.1


@dataclass
class ConflictFreeGradientsConfig:
    """Conflict-free combination of the per-term gradients, ConFIG (PinnEngine.set_conflict_free_gradients), off by
    default.  Not together with loss_balancing; an L-BFGS stage uses the plain sum."""
    enabled: bool = False


@dataclass
class BatchingConfig:
    """Stochastic mini-batching of the collocation term (PinnEngine.set_batching), off by default.  batch_points is
    per rank; an L-BFGS stage ignores it."""
    enabled: bool = False
    batch_points: int = 12000
    seed: int = 0


@dataclass
class GradClipConfig:
    """Global-norm gradient clipping of the Adam updates (PinnEngine.set_grad_clipping), off by default: max_norm = 0
    is off.  An L-BFGS stage ignores it."""
    max_norm: float = 0.0


@dataclass
class ResidualAttentionConfig:
    """Residual-based attention weights on the collocation points (PinnEngine.set_residual_attention), off by
    default: eta = 0 is off, eta > 0 switches it on (the paper's values: eta 0.01, gamma 0.999).  lam starts at init
    and is not saved in checkpoints; an L-BFGS stage keeps the weights fixed."""
    eta: float = 0.0
    gamma: float = 0.999
    init: float = 1.0


@dataclass
class WeightFactorizationConfig:
    """Random weight factorization of every Linear layer of both nets, W = diag(exp(s)) V with s ~ Normal(mean, std)
    drawn from a generator of its own seeded with `seed` (PinnEngine.set_weight_factorization).  The key is absent by
    default; `training.weight_factorization: {mean, std, seed}` (any subset, or an empty mapping) switches it on.  The
    paper recommends mean 0.5 or 1.0 with std 0.1."""
    enabled: bool = False
    mean: float = 0.5
    std: float = 0.1
    seed: int = 0


@dataclass
class HardBoundaryConfig:
    """The cavity's wall values by an output transform, u = g + D N_u, v = D N_v (PinnEngine.set_hard_boundary), off by
    default: `training.hard_boundary: {enabled: true, lift_power: 2}`.  lift_power (1..8) is the exponent of the lid's
    lift g = l(X) Y^lift_power; its default is a guess, not a measured optimum."""
    enabled: bool = False
    lift_power: int = 2


@dataclass
class PseudoTimeConfig:
    """Pseudo-time stepping of the equation loss with device-held anchors (PinnEngine.set_pseudo_time), off by default:
    `training.pseudo_time: {enabled: true, dtau: 0.5, every: 100}`.  dtau: the pseudo-time step of the momentum
    equations; every: optimiser updates between anchor refreshes; pressure_dtau: that of the continuity equation
    (artificial compressibility), 0 = none.  None of them has a measured default.  Not together with resampling or
    batching."""
    enabled: bool = False
    dtau: float = 1.0
    every: int = 100
    pressure_dtau: float = 0.0


VALIDATION_METRICS = ("uv", "u", "v", "p", "p0")


@dataclass
class ValidationConfig:
    """Validation error against the DNS fields on the device, with the best weights kept
    (PinnEngine.set_validation), off by default.  every: optimizer updates between validations; metric: what
    `best` means; patience: > 0 ends a stage at a log point after that many validations without improvement."""
    enabled: bool = False
    every: int = 1000
    metric: str = "uv"
    keep_best: bool = True
    patience: int = 0


EARLY_STOP_QUANTITIES = ("loss", "loss_e", "loss_b")
EARLY_STOP_MODES = ("any", "all")


@dataclass
class EarlyStopConfig:
    """The device convergence monitor that ends an Adam stage early (solver.set_early_stopping);
    the key's absence means off.  window: observed updates per window mean; min_rel_improvement: a window that improves
    the mean of `quantity` by less than this fraction is stale (null: criterion off); re_eff_tol: a window whose mean
    Re_eff moves by less than this fraction is settled (null, the default: criterion off); patience: windows in a row;
    min_updates: no stop bit before this update of the stage; mode: any | all criteria; every: updates per observation.
    The defaults are guesses: no value has been compared in training."""
    window: int = 1000
    min_rel_improvement: Optional[float] = 1e-3
    patience: int = 3
    re_eff_tol: Optional[float] = None
    min_updates: int = 0
    quantity: str = "loss"
    mode: str = "any"
    every: int = 1


@dataclass
class IdentifyViscosityConfig:
    """The Reynolds number learned from the supervised data (solver.set_viscosity_identification; DESIGN.md section
    7.15); the key's absence means off.  re0: the starting estimate (null: physics.Re); lr: the rate of the scalar's own
    Adam on ln nu; re_min, re_max: the bounds of the estimate."""
    re0: Optional[float] = None
    lr: float = 1e-2
    re_min: float = 1e-2
    re_max: float = 1e6


RE_CONTINUATION_SHAPES = ("geometric", "linear_re", "linear_nu")


@dataclass
class ReContinuationConfig:
    """Continuation in the Reynolds number (solver.set_reynolds_continuation); the key's absence
    means off.  The viscosity is ramped from 1 / re_start to 1 / physics.Re over `updates` Adam updates after `hold`
    updates at the start; shape: geometric | linear_re | linear_nu; stairs = K > 0: in K equal stairs."""
    re_start: float = 0.0
    updates: int = 0
    hold: int = 0
    shape: str = "geometric"
    stairs: int = 0


@dataclass
class FlowDiagnosticsConfig:
    """Flow diagnostics on the device (solver.set_flow_diagnostics); the key's absence means off.
    After every `every` optimizer updates the primary vortex, the counter-rotating area (nodes with psi > eps |psi_min|)
    and the mass defect of the net's field on an nx x ny grid of the cavity are recorded."""
    nx: int = 257
    ny: int = 257
    every: int = 1000
    eps: float = 1e-3


@dataclass
class CheckpointConfig:
    """Training-state snapshots that resume bit for bit (solver.set_checkpointing), off by default: path of the file
    (one per rank) and the optimizer updates between two non-blocking snapshots."""
    path: str = ""
    every: int = 0

    @property
    def enabled(self):
        return bool(self.path) and self.every > 0


SCHEDULERS = ("constant", "multistep", "step", "exponential", "cosine")


def _default_stages():
    table = [(0.05, 1e-3), (0.03, 2e-4), (0.01, 4e-5), (0.005, 1e-5), (0.002, 2e-6), (0.002, 2e-6)]
    return [TrainingStage(a, 500000, lr, "Stage %d" % (i + 1)) for i, (a, lr) in enumerate(table)]


@dataclass
class TrainingConfig:
    N_f: int = 120000
    log_interval: int = 1000
    enable_tensorboard: bool = True
    tb_log_dir: str = "runs"
    sort_training_points: bool = True
    sdf_weighting: SDFWeightConfig = field(default_factory=SDFWeightConfig)
    coordinate_transform: bool = False
    resampling: ResamplingConfig = field(default_factory=ResamplingConfig)
    loss_balancing: LossBalancingConfig = field(default_factory=LossBalancingConfig)
    conflict_free_gradients: ConflictFreeGradientsConfig = field(default_factory=ConflictFreeGradientsConfig)
    batching: BatchingConfig = field(default_factory=BatchingConfig)
    residual_attention: ResidualAttentionConfig = field(default_factory=ResidualAttentionConfig)
    grad_clip: GradClipConfig = field(default_factory=GradClipConfig)
    weight_factorization: WeightFactorizationConfig = field(default_factory=WeightFactorizationConfig)
    validation: ValidationConfig = field(default_factory=ValidationConfig)
    hard_boundary: HardBoundaryConfig = field(default_factory=HardBoundaryConfig)
    pseudo_time: PseudoTimeConfig = field(default_factory=PseudoTimeConfig)
    checkpoint: CheckpointConfig = field(default_factory=CheckpointConfig)
    early_stop: Optional[EarlyStopConfig] = None
    identify_viscosity: Optional[IdentifyViscosityConfig] = None
    re_continuation: Optional[ReContinuationConfig] = None
    flow_diagnostics: Optional[FlowDiagnosticsConfig] = None
    training_stages: List[TrainingStage] = field(default_factory=_default_stages)


@dataclass
class AppConfig:
    experiment_name: str = "NSFnet_MI355X"
    description: str = ""
    physics: PhysicsConfig = field(default_factory=PhysicsConfig)
    network: NetworkConfig = field(default_factory=NetworkConfig)
    training: TrainingConfig = field(default_factory=TrainingConfig)
    supervision: SupervisionConfig = field(default_factory=SupervisionConfig)


def _fill(obj, data):
    """Copy known keys of a (nested) dict onto a dataclass instance; unknown keys are ignored."""
    if not isinstance(data, dict):
        return obj
    known = {f.name: f for f in fields(obj)}
    for key, val in data.items():
        if key not in known:
            continue
        cur = getattr(obj, key)
        if key == "training_stages":
            setattr(obj, key, [TrainingStage(float(s["alpha"]), int(s["epochs"]), float(s["lr"]), str(s["name"]),
                                             str(s.get("optimizer", "adam")), int(s.get("history_size", 100)),
                                             str(s.get("line_search", "strong_wolfe")),
                                             scheduler=str(s.get("scheduler", "constant")),
                                             milestones=[int(m) for m in (s.get("milestones") or [])],
                                             gamma=float(s.get("gamma", 0.1)), step_size=int(s.get("step_size", 1)),
                                             t_max=int(s.get("t_max", 0)), eta_min=float(s.get("eta_min", 0.0)),
                                             warmup_epochs=int(s.get("warmup_epochs", 0)),
                                             warmup_start=float(s.get("warmup_start", 0.0)))
                               for s in (val or [])])
        elif key == "fourier_features":          # absent, null or false: off
            if val is not None and val is not False:
                setattr(obj, key, _fill(FourierFeaturesConfig(), val))
        elif key == "early_stop":                # absent, null or false: off
            if val is not None and val is not False:
                es = EarlyStopConfig()
                for k, v in (val.items() if isinstance(val, dict) else ()):
                    if k in ("min_rel_improvement", "re_eff_tol"):
                        setattr(es, k, None if v is None else float(v))
                    elif k in ("quantity", "mode"):
                        setattr(es, k, str(v))
                    elif k in ("window", "patience", "min_updates", "every"):
                        setattr(es, k, int(v))
                setattr(obj, key, es)
        elif key == "identify_viscosity":        # absent, null or false: off
            if val is not None and val is not False:
                iv = IdentifyViscosityConfig()
                for k, v in (val.items() if isinstance(val, dict) else ()):
                    if k in ("re0", "lr", "re_min", "re_max"):
                        setattr(iv, k, None if v is None and k == "re0" else float(v))
                setattr(obj, key, iv)
        elif key == "re_continuation":           # absent, null or false: off
            if val is not None and val is not False:
                rc = ReContinuationConfig()
                for k, v in (val.items() if isinstance(val, dict) else ()):
                    if k == "re_start":
                        rc.re_start = float(v)
                    elif k == "shape":
                        rc.shape = str(v)
                    elif k in ("updates", "hold", "stairs"):
                        setattr(rc, k, int(v))
                setattr(obj, key, rc)
        elif key == "flow_diagnostics":          # absent, null or false: off
            if val is not None and val is not False:
                fd = FlowDiagnosticsConfig()
                for k, v in (val.items() if isinstance(val, dict) else ()):
                    if k in ("nx", "ny", "every"):
                        setattr(fd, k, int(v))
                    elif k == "eps":
                        fd.eps = float(v)
                setattr(obj, key, fd)
        elif key == "weight_factorization":      # the key's presence switches it on (`enabled: false` still wins)
            if val is not None and val is not False:
                cur.enabled = True
                _fill(cur, val)
        elif is_dataclass(cur):
            _fill(cur, val)
        else:
            setattr(obj, key, type(cur)(val) if cur is not None and not isinstance(cur, str) else val)
    return obj


class ConfigManager:
    def __init__(self, config=None):
        self.config = config or AppConfig()

    @classmethod
    def from_file(cls, path):
        with open(path, "r", encoding="utf-8") as fh:
            raw = yaml.safe_load(fh) or {}
        mgr = cls(_fill(AppConfig(), raw))
        mgr.validate_config()
        return mgr

    def validate_config(self):
        c = self.config
        problems = []
        if c.physics.Re <= 0:
            problems.append("physics.Re must be positive")
        if min(c.network.layers, c.network.layers_1, c.network.hidden_size, c.network.hidden_size_1) < 1:
            problems.append("network sizes must be >= 1")
        if c.training.N_f < 1:
            problems.append("training.N_f must be >= 1")
        rs = c.training.resampling
        if rs.enabled and (rs.every < 1 or rs.pool_points < 1 or rs.k < 0 or rs.c < 0 or rs.seed < 0):
            problems.append("training.resampling: every, pool_points >= 1 and k, c, seed >= 0 required")
        lb = c.training.loss_balancing
        if lb.enabled and (lb.every < 1 or not 0.0 < lb.beta <= 1.0):
            problems.append("training.loss_balancing: every >= 1 and 0 < beta <= 1 required")
        if lb.enabled and c.training.conflict_free_gradients.enabled:
            problems.append("training.conflict_free_gradients and training.loss_balancing both decide how the term "
                            "gradients are combined: enable one of them")
        bt = c.training.batching
        if bt.enabled and (bt.batch_points < 1 or bt.seed < 0):
            problems.append("training.batching: batch_points >= 1 and seed >= 0 required")
        ra = c.training.residual_attention
        if not (0.0 <= ra.eta < float("inf") and 0.0 < ra.gamma <= 1.0 and 0.0 <= ra.init < float("inf")):
            problems.append("training.residual_attention: eta >= 0, 0 < gamma <= 1 and init >= 0 required")
        gc = c.training.grad_clip
        if not 0.0 <= gc.max_norm < float("inf"):
            problems.append("training.grad_clip: max_norm >= 0 and finite required")
        wf = c.training.weight_factorization
        if wf.enabled and not (abs(wf.mean) < float("inf") and 0.0 <= wf.std < float("inf") and wf.seed >= 0):
            problems.append("training.weight_factorization: finite mean, finite std >= 0 and seed >= 0 required")
        ff = c.network.fourier_features
        if ff is not None and not (0.0 < ff.sigma < float("inf") and ff.seed >= 0 and c.network.hidden_size % 2 == 0 and
                                   c.network.layers >= 2):
            problems.append("network.fourier_features: finite sigma > 0, seed >= 0, an even hidden_size and layers >= 2 required")
        if ff is not None and (c.training.hard_boundary.enabled or c.training.pseudo_time.enabled):
            problems.append("network.fourier_features does not go together with training.hard_boundary or training.pseudo_time")
        hb = c.training.hard_boundary
        if hb.enabled and not 1 <= hb.lift_power <= 8:
            problems.append("training.hard_boundary: lift_power in 1..8 required")
        pt = c.training.pseudo_time
        if pt.enabled and not (0.0 < pt.dtau < float("inf") and pt.every >= 1 and 0.0 <= pt.pressure_dtau < float("inf")):
            problems.append("training.pseudo_time: finite dtau > 0, every >= 1 and finite pressure_dtau >= 0 required")
        if pt.enabled and (c.training.resampling.enabled or c.training.batching.enabled):
            problems.append("training.pseudo_time does not go together with training.resampling or training.batching")
        va = c.training.validation
        if va.enabled and (va.every < 1 or va.patience < 0 or va.metric not in VALIDATION_METRICS):
            problems.append("training.validation: every >= 1, patience >= 0 and metric one of %s required"
                            % " | ".join(VALIDATION_METRICS))
        es = c.training.early_stop
        if es is not None:
            tol_ok = lambda v: v is None or 0.0 <= v < float("inf")
            if (es.window < 1 or es.patience < 1 or es.every < 1 or es.min_updates < 0 or not tol_ok(es.min_rel_improvement)
                    or not tol_ok(es.re_eff_tol) or es.quantity not in EARLY_STOP_QUANTITIES
                    or es.mode not in EARLY_STOP_MODES):
                problems.append("training.early_stop: window, patience, every >= 1, min_updates >= 0, finite tolerances >= 0 "
                                "(or null), quantity one of %s and mode one of %s required"
                                % (" | ".join(EARLY_STOP_QUANTITIES), " | ".join(EARLY_STOP_MODES)))
            if es.min_rel_improvement is None and es.re_eff_tol is None:
                problems.append("training.early_stop: at least one of min_rel_improvement and re_eff_tol must be set")
        iv = c.training.identify_viscosity
        if iv is not None:
            if not (0.0 < iv.re_min <= iv.re_max < float("inf") and 0.0 <= iv.lr < float("inf")
                    and (iv.re0 is None or iv.re_min <= iv.re0 <= iv.re_max)):
                problems.append("training.identify_viscosity: 0 < re_min <= re0 <= re_max < inf and a finite lr >= 0 required")
            if es is not None or pt.enabled or c.training.conflict_free_gradients.enabled:
                problems.append("training.identify_viscosity does not go together with training.early_stop, "
                                "training.pseudo_time or training.conflict_free_gradients")
        fd = c.training.flow_diagnostics
        if fd is not None and not (fd.nx >= 3 and fd.ny >= 3 and fd.every >= 1 and 0.0 <= fd.eps < float("inf")):
            problems.append("training.flow_diagnostics: nx, ny >= 3, every >= 1 and a finite eps >= 0 required")
        rc = c.training.re_continuation
        if rc is not None:
            if not (0.0 < rc.re_start < float("inf") and rc.updates >= 1 and rc.hold >= 0 and rc.stairs >= 0
                    and rc.shape in RE_CONTINUATION_SHAPES):
                problems.append("training.re_continuation: finite re_start > 0, updates >= 1, hold >= 0, stairs >= 0 and "
                                "shape one of %s required" % " | ".join(RE_CONTINUATION_SHAPES))
            if es is not None or iv is not None:
                problems.append("training.re_continuation does not go together with training.early_stop or "
                                "training.identify_viscosity")
        ck = c.training.checkpoint
        if ck.every < 0 or (ck.every > 0 and not ck.path):
            problems.append("training.checkpoint: every >= 0, and a path when every > 0, required")
        for st in c.training.training_stages:
            if st.scheduler not in SCHEDULERS:
                problems.append("stage %s: scheduler must be one of %s (got %r)" % (st.name, " | ".join(SCHEDULERS),
                                                                                   st.scheduler))
            elif st.scheduler != "constant" and st.optimizer == "lbfgs":
                problems.append("stage %s: an lbfgs stage takes no scheduler (got %r)" % (st.name, st.scheduler))
            if st.scheduler in ("multistep", "step", "exponential") and not 0.0 < st.gamma < float("inf"):
                problems.append("stage %s: gamma must be finite and > 0" % st.name)
            if st.scheduler == "multistep" and (len(st.milestones) > 16 or any(m < 0 for m in st.milestones) or any(
                    b < a for a, b in zip(st.milestones, st.milestones[1:]))):
                problems.append("stage %s: milestones must be at most 16, >= 0 and ascending" % st.name)
            if st.scheduler == "step" and st.step_size < 1:
                problems.append("stage %s: step_size must be >= 1" % st.name)
            if st.scheduler == "cosine" and (st.t_max < 0 or not abs(st.eta_min) < float("inf")):
                problems.append("stage %s: t_max >= 0 (0 = the stage's epochs) and a finite eta_min required" % st.name)
            if st.warmup_epochs < 0 or not 0.0 <= st.warmup_start <= 1.0:
                problems.append("stage %s: warmup_epochs >= 0 and 0 <= warmup_start <= 1 required" % st.name)
            if st.warmup_epochs > 0 and st.optimizer == "lbfgs":
                problems.append("stage %s: an lbfgs stage takes no warm-up" % st.name)
            if st.epochs < 0 or st.lr <= 0:
                problems.append("stage %s: epochs >= 0 and lr > 0 required" % st.name)
            if st.optimizer not in ("adam", "lbfgs"):
                problems.append("stage %s: optimizer must be adam or lbfgs (got %r)" % (st.name, st.optimizer))
            if st.line_search not in ("strong_wolfe", "none"):
                problems.append("stage %s: line_search must be strong_wolfe or none (got %r)" % (st.name, st.line_search))
            if not 1 <= st.history_size <= 1024:
                problems.append("stage %s: history_size must be 1..1024" % st.name)
        if problems:
            raise ValueError("invalid configuration: " + "; ".join(problems))
        return True

    def print_config(self):
        c = self.config
        print("experiment : %s" % c.experiment_name)
        print("physics    : Re=%s alpha_evm=%s bc_weight=%s eq_weight=%s"
              % (c.physics.Re, c.physics.alpha_evm, c.physics.bc_weight, c.physics.eq_weight))
        print("network    : %dx%d (u,v,p) + %dx%d (e)"
              % (c.network.layers, c.network.hidden_size, c.network.layers_1, c.network.hidden_size_1))
        if c.network.fourier_features is not None:
            print("fourier    : sigma=%s seed=%d (first layer frozen)" % (c.network.fourier_features.sigma, c.network.fourier_features.seed))
        t = c.training
        print("training   : N_f=%d log_interval=%d sort=%s sdf=%s coord_transform=%s stages=%d"
              % (t.N_f, t.log_interval, t.sort_training_points, t.sdf_weighting.enabled, t.coordinate_transform,
                 len(t.training_stages)))
        if t.resampling.enabled:
            print("resampling : every=%d pool_points=%d k=%s c=%s seed=%d"
                  % (t.resampling.every, t.resampling.pool_points, t.resampling.k, t.resampling.c, t.resampling.seed))
        if t.loss_balancing.enabled:
            print("balancing  : every=%d beta=%s" % (t.loss_balancing.every, t.loss_balancing.beta))
        if t.conflict_free_gradients.enabled:
            print("conflict-free gradients: on (ConFIG)")
        if t.batching.enabled:
            print("batching   : batch_points=%d (per rank) seed=%d" % (t.batching.batch_points, t.batching.seed))
        if t.residual_attention.eta > 0:
            print("attention  : eta=%s gamma=%s init=%s" % (t.residual_attention.eta, t.residual_attention.gamma,
                                                            t.residual_attention.init))
        if t.grad_clip.max_norm > 0:
            print("grad clip  : max_norm=%s" % t.grad_clip.max_norm)
        if t.weight_factorization.enabled:
            print("weight fact: mean=%s std=%s seed=%d" % (t.weight_factorization.mean, t.weight_factorization.std,
                                                            t.weight_factorization.seed))
        if t.hard_boundary.enabled:
            print("hard walls : lift_power=%d" % t.hard_boundary.lift_power)
        if t.pseudo_time.enabled:
            print("pseudo-time: dtau=%s every=%d pressure_dtau=%s" % (t.pseudo_time.dtau, t.pseudo_time.every,
                                                                      t.pseudo_time.pressure_dtau or None))
        if t.validation.enabled:
            print("validation : every=%d metric=%s keep_best=%s patience=%d"
                  % (t.validation.every, t.validation.metric, t.validation.keep_best, t.validation.patience))
        if t.early_stop is not None:
            es = t.early_stop
            print("early stop : window=%d min_rel_improvement=%s patience=%d re_eff_tol=%s min_updates=%d quantity=%s "
                  "mode=%s every=%d" % (es.window, es.min_rel_improvement, es.patience, es.re_eff_tol, es.min_updates,
                                        es.quantity, es.mode, es.every))
        if t.identify_viscosity is not None:
            iv = t.identify_viscosity
            print("identify Re: re0=%s lr=%g bounds=[%g, %g]" % (iv.re0, iv.lr, iv.re_min, iv.re_max))
        if t.re_continuation is not None:
            rc = t.re_continuation
            print("Re ramp    : re_start=%g updates=%d hold=%d shape=%s stairs=%d"
                  % (rc.re_start, rc.updates, rc.hold, rc.shape, rc.stairs))
        if t.checkpoint.enabled:
            print("checkpoint : path=%s every=%d" % (t.checkpoint.path, t.checkpoint.every))
        for st in t.training_stages:
            if st.scheduler != "constant" or st.warmup_epochs > 0:
                a = st.schedule_args()
                print("scheduler  : %s: %s%s" % (st.name, st.scheduler, "".join(
                    " %s=%s" % (k, a[k]) for k in {"multistep": ("milestones", "gamma"), "step": ("step_size", "gamma"),
                                                   "exponential": ("gamma",), "cosine": ("t_max", "eta_min"),
                                                   "constant": ()}[st.scheduler]
                    + (("warmup_epochs", "warmup_start") if st.warmup_epochs > 0 else ()))))
        print("supervision: enabled=%s samples=%d weight=%s"
              % (c.supervision.enabled, c.supervision.num_samples, c.supervision.loss_weight))
