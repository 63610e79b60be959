"""Learning-rate schedules of the Adam stages.

An LrSchedule is the host description of what the update kernel computes from its device epoch counter e
(include/nsfnet_pinn.h, pinn_lr_schedule_t): the closed forms of torch.optim.lr_scheduler's MultiStepLR, StepLR,
ExponentialLR and CosineAnnealingLR, times an optional linear warm-up.  value() is the same fp64 formula on the host.
"""
import math
from dataclasses import dataclass

KINDS = ("constant", "multistep", "step", "exponential", "cosine")      # index = PINN_LR_*
MAX_MILESTONES = 16                                                     # PINN_LR_MAX_MILESTONES


@dataclass(frozen=True)
class LrSchedule:
    kind: str = "constant"
    milestones: tuple = ()          # multistep: epochs at which lr is multiplied by gamma (non-decreasing)
    gamma: float = 0.1              # multistep / step / exponential
    step_size: int = 1              # step
    t_max: int = 1                  # cosine
    eta_min: float = 0.0            # cosine
    warmup_epochs: int = 0          # W > 0: times warmup_start + (1 - warmup_start) min(e, W) / W
    warmup_start: float = 0.0

    def __post_init__(self):
        set_ = object.__setattr__
        if self.kind not in KINDS:
            raise ValueError("lr schedule: kind must be one of %s (got %r)" % ("|".join(KINDS), self.kind))
        set_(self, "milestones", tuple(int(m) for m in self.milestones))
        for name in ("step_size", "t_max", "warmup_epochs"):
            v = getattr(self, name)
            if int(v) != v:
                raise ValueError("lr schedule: %s must be an integer (got %r)" % (name, v))
            set_(self, name, int(v))
        for name in ("gamma", "eta_min", "warmup_start"):
            set_(self, name, float(getattr(self, name)))
        if self.kind in ("multistep", "step", "exponential") and not (self.gamma > 0.0 and math.isfinite(self.gamma)):
            raise ValueError("lr schedule: gamma must be finite and > 0 (got %r)" % self.gamma)
        if self.kind == "multistep":
            if len(self.milestones) > MAX_MILESTONES:
                raise ValueError("lr schedule: at most %d milestones (got %d)" % (MAX_MILESTONES, len(self.milestones)))
            if any(m < 0 for m in self.milestones) or any(b < a for a, b in zip(self.milestones, self.milestones[1:])):
                raise ValueError("lr schedule: milestones must be >= 0 and ascending (got %r)" % (self.milestones,))
        if self.kind == "step" and self.step_size < 1:
            raise ValueError("lr schedule: step_size must be >= 1 (got %r)" % self.step_size)
        if self.kind == "cosine":
            if self.t_max < 1:
                raise ValueError("lr schedule: t_max must be >= 1 (got %r)" % self.t_max)
            if not math.isfinite(self.eta_min):
                raise ValueError("lr schedule: eta_min must be finite")
        if self.warmup_epochs < 0:
            raise ValueError("lr schedule: warmup_epochs must be >= 0 (got %r)" % self.warmup_epochs)
        if not (0.0 <= self.warmup_start <= 1.0):
            raise ValueError("lr schedule: warmup_start must be in [0, 1] (got %r)" % self.warmup_start)

    def key(self):
        """The launch constants as a hashable tuple (part of a captured step's key)."""
        return (self.kind, self.milestones, self.gamma, self.step_size, self.t_max, self.eta_min, self.warmup_epochs,
                self.warmup_start)

    def value(self, lr0, e):
        """lr_e in fp64: the operations, and their order, of the kernel."""
        lr0, e = float(lr0), int(e)
        lr = lr0
        if self.kind == "multistep":
            lr = lr0 * math.pow(self.gamma, float(sum(1 for m in self.milestones if m <= e)))
        elif self.kind == "step":
            lr = lr0 * math.pow(self.gamma, float(e // self.step_size))
        elif self.kind == "exponential":
            lr = lr0 * math.pow(self.gamma, float(e))
        elif self.kind == "cosine":
            lr = self.eta_min + (lr0 - self.eta_min) * (1.0 + math.cos(math.pi * float(e) / float(self.t_max))) / 2.0
        if self.warmup_epochs > 0:
            w = float(min(e, self.warmup_epochs)) / float(self.warmup_epochs)
            lr = lr * (self.warmup_start + (1.0 - self.warmup_start) * w)
        return lr

    def c_struct(self):
        """The pinn_lr_schedule_t of this schedule."""
        from ._lib import LrScheduleStruct
        s = LrScheduleStruct()
        s.kind, s.n_milestones = KINDS.index(self.kind), len(self.milestones)
        for i, m in enumerate(self.milestones):
            s.milestones[i] = m
        s.step_size, s.t_max, s.warmup_epochs = self.step_size, self.t_max, self.warmup_epochs
        s.gamma, s.eta_min, s.warmup_start = self.gamma, self.eta_min, self.warmup_start
        return s


def from_torch(scheduler):
    """(LrSchedule, lr0, e) of a torch.optim.lr_scheduler object of type MultiStepLR, StepLR, ExponentialLR or
    CosineAnnealingLR, from its own attributes (lr0 = its first base_lr, e = its last_epoch); None for anything
    else - subclasses included, whose get_lr may be another formula."""
    from torch.optim import lr_scheduler as ls
    t = type(scheduler)
    if t is ls.MultiStepLR:
        spec = LrSchedule("multistep", milestones=sorted(scheduler.milestones.elements()), gamma=scheduler.gamma)
    elif t is ls.StepLR:
        spec = LrSchedule("step", step_size=scheduler.step_size, gamma=scheduler.gamma)
    elif t is ls.ExponentialLR:
        spec = LrSchedule("exponential", gamma=scheduler.gamma)
    elif t is ls.CosineAnnealingLR:
        spec = LrSchedule("cosine", t_max=scheduler.T_max, eta_min=scheduler.eta_min)
    else:
        return None
    return spec, float(scheduler.base_lrs[0]), int(scheduler.last_epoch)
