"""Cost of the frozen Fourier-feature first layer on one GPU, and what PINN_FF_SPLIT=1 gives
back:

    python scripts/profile_fourier.py [--rounds 6 --steps 20] [--shape headline|8x400] [--graph] [--sigma 2.0]

Engines with the same points in one process, timed by CUDA events in alternating rounds (tanh, ff8, split, split2, tanh,
...) so that clock drift hits all alike:
  tanh    the default plan of a tanh net (fused role-split sweeps at the headline shape, the wide role-split sweeps at
          8x400): the yardstick;
  ff8     set_fourier_features with the switch unset: the 8-wave kernels, layer 0 stored;
  split   the same with PINN_FF_SPLIT=1 while its plans are created: the frozen-sine variants of the role-split, fused
          and wide role-split sweeps, whose reverse sweep ends at layer 1;
  split2  split under PINN_FUSE=0: the two role-split launches (headline shape only: nothing fuses at 8x400).
A step is PinnEngine.step, eager, or replayed from a hipGraph with --graph.  --shape headline: 6x256, 360 000 points,
bf16x3; --shape 8x400: 8x400 + 4x40 entropy net, 500 000 points with the [-1, 1] coordinate map and weights.  Prints the
kernels each engine's collocation plan launches, the median ms per step of each arm with its min - max over the rounds,
and the differences."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"headline": (6, 256, 360000, False), "8x400": (8, 400, 500000, True)}
SWITCH = "PINN_FF_SPLIT"
# arm -> (frozen sine first layer, the switches set while its plans are created)
ARMS = {"tanh": (False, {}), "ff8": (True, {}), "split": (True, {SWITCH: "1"}), "split2": (True, {SWITCH: "1", "PINN_FUSE": "0"})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--points", type=int, default=0, help="default: 360000 (headline) / 500000 (8x400)")
    ap.add_argument("--sigma", type=float, default=2.0)
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
    w, kw = None, {}
    if ev:
        x, y, bc[0], bc[1] = 2 * x - 1, 2 * y - 1, 2 * bc[0] - 1, 2 * bc[1] - 1
        w = (0.5 + rng.rand(n)).astype(np.float32)
        kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05, coord_scale=2.0)
    # the arms set the switches themselves: they are read when a plan is created
    ambient = {k: os.environ.pop(k, None) for k in (SWITCH, "PINN_FUSE")}
    engines = {}
    arms = {m: v for m, v in ARMS.items() if m != "split2" or a.shape == "headline"}      # (nothing fuses at 8x400)
    for mode, (ff, env) in arms.items():
        os.environ.update(env)
        E = eng.PinnEngine(dev, L, H, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3", **kw)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=0)))
        if ff:
            E.set_fourier_features(sigma=a.sigma, seed=0)
        if ev:
            E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=1)))
            E.e_trainable = True
        E.set_collocation(x, y, weights=w)
        E.set_boundary(*bc)
        for k in env:
            os.environ.pop(k, None)
        engines[mode] = E
    os.environ.update({k: v for k, v in ambient.items() if v is not None})
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
    tag = "%s %dx%d %d pts %s" % (a.shape, L, H, n, "graph" if a.graph else "eager")
    for m, E in engines.items():
        print("[%s] %-6s %.4f ms/step (%.4f - %.4f)  %s" % (tag, m, med[m], min(times[m]), max(times[m]),
                                                            "/".join(E.plan_f.kernel_names())))
    for m, base in (("ff8", "tanh"), ("split", "tanh"), ("split2", "tanh"), ("split", "ff8"), ("split", "split2")):
        if m not in med or base not in med:
            continue
        print("[%s] %s - %s = %+.1f us per step (%+.2f %%)" % (tag, m, base, 1e3 * (med[m] - med[base]),
                                                               100.0 * (med[m] / med[base] - 1.0)))
    for m, E in engines.items():
        print("[%s] %s: loss %.6e, graphs %d" % (tag, m, float(E.loss_terms()["loss"]), len(E._graphs)))


if __name__ == "__main__":
    main()
