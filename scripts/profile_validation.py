"""Cost of one device validation at the headline shape (6x256, 360 k points, bf16x3, one GPU):

    python scripts/profile_validation.py [--rounds 5 --steps 20] [--flavour ev] [--batch 36000] [--graph] [--val 66049]

Two engines with the same parameters and points, timed by CUDA events in alternating rounds (A/B, A/B, ...) so that
clock drift hits both alike: `off` (the feature off: the launches of a tree without it) and `on` (set_validation
with every = 1 on --val points, the 257 x 257 DNS grid by default: a value forward, pinn_val_stats and pinn_val_keep
after every update).  A step is PinnEngine.step, eager, or replayed from a hipGraph with --graph.  --flavour ev adds
the entropy net and SDF-like static weights; --batch B runs both engines on mini-batches of B points.  Prints the
median ms per step of each mode, on - off = the cost of one validation, and its share at every = 1000."""
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
    ap.add_argument("--points", type=int, default=360000)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--flavour", choices=("nsfnet", "ev"), default="nsfnet")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--val", type=int, default=257 * 257)
    a = ap.parse_args()
    os.environ["NSFNET_GRAPH"] = "1" if a.graph else "0"
    from nsfnet_amd import engine as eng
    from oracle import autograd_ref as ar
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    x, y = rng.rand(a.points).astype(np.float32), rng.rand(a.points).astype(np.float32)
    w = (0.5 + rng.rand(a.points)).astype(np.float32) if a.flavour == "ev" else None
    bc = tuple(v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary())
    ev = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05) if a.flavour == "ev" else {}
    engines = {}
    for mode in ("off", "on"):
        E = eng.PinnEngine(dev, 6, 256, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3", **ev)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=0)))
        if a.flavour == "ev":
            E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=1)))
        E.set_collocation(x, y, weights=w)
        E.set_boundary(*bc)
        if a.batch:
            E.set_batching(a.batch, seed=0)
        if mode == "on":
            xv, yv = rng.rand(a.val).astype(np.float32), rng.rand(a.val).astype(np.float32)
            E.set_validation(xv, yv, np.sin(xv), np.cos(yv), xv * yv, every=1, metric="uv")
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
    tag = "%s %s%s" % (a.flavour, "graph" if a.graph else "eager", " batch=%d" % a.batch if a.batch else "")
    for m in engines:
        print("[%s] %-3s %.4f ms/step  (rounds: %s)" % (tag, m, med[m], " ".join("%.4f" % t for t in times[m])))
    d = med["on"] - med["off"]
    print("[%s] on - off = %+.1f us per validation of %d points (%+.2f %% of a step; %+.4f %% at every = 1000)"
          % (tag, 1e3 * d, a.val, 100.0 * d / med["off"], 0.1 * d / med["off"]))
    info = engines["on"].validation_info()
    print("[%s] validation info: %s" % (tag, {k: v for k, v in info.items() if k != "last"}))


if __name__ == "__main__":
    main()
