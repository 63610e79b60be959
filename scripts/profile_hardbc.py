"""Cost of the hard wall conditions on one GPU:

    python scripts/profile_hardbc.py [--rounds 5 --steps 20] [--shape headline|ev|8x400] [--graph]

Three engines with the same parameters and points, timed by CUDA events in alternating rounds (off, hard, split, off,
...) so that clock drift hits all alike: `off` (an engine that never heard of the feature), `hard`
(set_hard_boundary at the defaults before the point sets are attached: the constrained 8-wave kernels) and `split`
(the same with PINN_HBC_SPLIT=1 while its plans are created: the constrained role-split / fused sweeps where the shape
has them).  A step is PinnEngine.step, eager, or replayed from a hipGraph with --graph.  --shape headline: 6x256,
360 000 points, bf16x3 - there `off` and `split` run the fused role-split sweeps and `hard` the 8-wave kernels, so
hard - off is the schedule fallback plus the transform and split - off the transform alone; run it again under
PINN_FUSE=0 for the constrained two launches, or under PINN_SCHED=0 PINN_FUSE=0, where all three run the 8-wave
kernels.  --shape ev: 6x80 + 4x40 entropy net, 120 000 points with the [-1, 1] coordinate map, where all always run
the same family.  --shape 8x400: 8x400 + 4x40, 500 000 points with the map (the wide role-split sweeps).  Prints the
kernels each engine's collocation plan launches, the median ms per step of each mode and the differences."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"headline": (6, 256, 360000, False), "ev": (6, 80, 120000, True), "8x400": (8, 400, 500000, True)}
SWITCH = "PINN_HBC_SPLIT"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--points", type=int, default=0, help="default: 360000 (headline) / 120000 (ev) / 500000 (8x400)")
    ap.add_argument("--lift-power", type=int, default=2)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    os.environ["NSFNET_GRAPH"] = "1" if a.graph else "0"
    from nsfnet_amd import engine as eng
    from oracle import autograd_ref as ar
    dev = torch.device("cuda:0")
    L, H, n, ev = SHAPES[a.shape]
    n = a.points or n
    rng = np.random.RandomState(0)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    bc = [v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary()]
    w, kw, where = None, {}, {}
    if ev:
        x, y, bc[0], bc[1] = 2 * x - 1, 2 * y - 1, 2 * bc[0] - 1, 2 * bc[1] - 1
        w = (0.5 + rng.rand(n)).astype(np.float32)
        kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05, coord_scale=2.0)
        where = dict(origin=(-1.0, -1.0), inv_len=0.5)
    ambient = os.environ.pop(SWITCH, None)      # the arms set the switch themselves: it is read when a plan is created
    engines = {}
    for mode in ("off", "hard", "split"):
        if mode == "split":
            os.environ[SWITCH] = "1"
        E = eng.PinnEngine(dev, L, H, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3", **kw)
        if mode != "off":
            E.set_hard_boundary(True, lift_power=a.lift_power, **where)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=0)))
        if ev:
            E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=1)))
            E.e_trainable = True
        E.set_collocation(x, y, weights=w)
        E.set_boundary(*bc)
        os.environ.pop(SWITCH, None)
        engines[mode] = E
    if ambient is not None:
        os.environ[SWITCH] = ambient
    times = {m: [] for m in engines}
    for _ in range(a.rounds):
        for mode, E in engines.items():
            for _ in range(3):
                E.step(1e-4)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                E.step(1e-4)
            t1.record()
            torch.cuda.synchronize()
            times[mode].append(t0.elapsed_time(t1) / a.steps)
    med = {m: float(np.median(v)) for m, v in times.items()}
    sw = " ".join("%s=%s" % (k, os.environ[k]) for k in ("PINN_SCHED", "PINN_WSPLIT", "PINN_FUSE") if k in os.environ)
    tag = "%s %dx%d %d pts %s%s" % (a.shape, L, H, n, "graph" if a.graph else "eager", " " + sw if sw else "")
    for m, E in engines.items():
        print("[%s] %-5s %.4f ms/step  %s  (rounds: %s)" % (tag, m, med[m], "/".join(E.plan_f.kernel_names()),
                                                           " ".join("%.4f" % t for t in times[m])))
    for m in ("hard", "split"):
        print("[%s] %s - off = %+.1f us per step (%+.2f %%)" % (tag, m, 1e3 * (med[m] - med["off"]),
                                                               100.0 * (med[m] / med["off"] - 1.0)))
    for m in ("hard", "split"):
        lt = engines[m].loss_terms()
        print("[%s] loss_b of the %s engine: %.3e  graphs: %d" % (tag, m, float(lt["loss_b"]), len(engines[m]._graphs)))


if __name__ == "__main__":
    main()
