"""Cost of the hard wall conditions on one GPU:

    python scripts/profile_hardbc.py [--rounds 5 --steps 20] [--shape headline|ev] [--graph]

Two engines with the same parameters and points, timed by CUDA events in alternating rounds (off, hard, off, ...) so
that clock drift hits both alike: `off` (an engine that never heard of the feature) and `hard` (set_hard_boundary at
the defaults before the point sets are attached).  A step is PinnEngine.step, eager, or replayed from a hipGraph with
--graph.  --shape headline: 6x256, 360 000 points, bf16x3 - there `off` runs the fused role-split sweeps and `hard` the
8-wave kernels, so the difference is the schedule fallback plus the transform; run it again under
PINN_SCHED=0 PINN_FUSE=0, where both run the 8-wave kernels, to see the transform alone.  --shape ev: 6x80 + 4x40
entropy net, 120 000 points with the [-1, 1] coordinate map, where both always run the same family.  Prints the kernels
each engine's collocation plan launches, the median ms per step of each mode and the difference."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=("headline", "ev"), default="headline")
    ap.add_argument("--points", type=int, default=0, help="default: 360000 (headline) / 120000 (ev)")
    ap.add_argument("--lift-power", type=int, default=2)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    os.environ["NSFNET_GRAPH"] = "1" if a.graph else "0"
    from nsfnet_amd import engine as eng
    from oracle import autograd_ref as ar
    dev = torch.device("cuda:0")
    ev = a.shape == "ev"
    L, H, n = (6, 80, a.points or 120000) if ev else (6, 256, a.points or 360000)
    rng = np.random.RandomState(0)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    bc = [v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary()]
    w, kw, where = None, {}, {}
    if ev:
        x, y, bc[0], bc[1] = 2 * x - 1, 2 * y - 1, 2 * bc[0] - 1, 2 * bc[1] - 1
        w = (0.5 + rng.rand(n)).astype(np.float32)
        kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05, coord_scale=2.0)
        where = dict(origin=(-1.0, -1.0), inv_len=0.5)
    engines = {}
    for mode in ("off", "hard"):
        E = eng.PinnEngine(dev, L, H, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3", **kw)
        if mode == "hard":
            E.set_hard_boundary(True, lift_power=a.lift_power, **where)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=0)))
        if ev:
            E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=1)))
            E.e_trainable = True
        E.set_collocation(x, y, weights=w)
        E.set_boundary(*bc)
        engines[mode] = E
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
        print("[%s] %-4s %.4f ms/step  %s  (rounds: %s)" % (tag, m, med[m], "/".join(E.plan_f.kernel_names()),
                                                           " ".join("%.4f" % t for t in times[m])))
    print("[%s] hard - off = %+.1f us per step (%+.2f %%)" % (tag, 1e3 * (med["hard"] - med["off"]),
                                                             100.0 * (med["hard"] / med["off"] - 1.0)))
    lt = engines["hard"].loss_terms()
    print("[%s] loss_b of the constrained engine: %.3e  graphs: %d" % (tag, float(lt["loss_b"]), len(engines["hard"]._graphs)))


if __name__ == "__main__":
    main()
