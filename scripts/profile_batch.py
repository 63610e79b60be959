"""Cost of the stochastic mini-batching at the headline shape (6x256, store of 360 k points, B = 36 k, bf16x3, one GPU):

    python scripts/profile_batch.py [--rounds 5 --steps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/profile_batch.py --rounds 1 --steps 10

Three engines with the same parameters, timed by CUDA events in alternating rounds (A/B/C, A/B/C, ...) so that clock
drift hits all three alike: `full` steps on the whole store, `plain` steps on a plain collocation set of B points
(batching off: the launches of a tree without the feature), `batch` draws B of the store's points every step.  A step
is PinnEngine.step (eager: [draw +] loss + gradient + Adam).  --flavour ev adds the entropy net and the scatter.
Prints the median ms per step of each mode and the ratios batch / plain and batch / full."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsfnet_amd import engine as eng  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--points", type=int, default=360000)
    ap.add_argument("--batch", type=int, default=36000)
    ap.add_argument("--flavour", choices=("nsfnet", "ev"), default="nsfnet")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    x, y = rng.rand(a.points).astype(np.float32), rng.rand(a.points).astype(np.float32)
    bc = tuple(v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary())
    ev = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05) if a.flavour == "ev" else {}
    engines = {}
    for mode in ("full", "plain", "batch"):
        E = eng.PinnEngine(dev, 6, 256, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3", **ev)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=0)))
        if a.flavour == "ev":
            E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=1)))
        n = a.batch if mode == "plain" else a.points
        E.set_collocation(x[:n], y[:n])
        E.set_boundary(*bc)
        if mode == "batch":
            E.set_batching(a.batch, seed=0)
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
    for m in engines:
        print("%-6s %.4f ms/step  (rounds: %s)" % (m, med[m], " ".join("%.4f" % t for t in times[m])))
    print("batch / plain = %.4f   batch / full = %.4f   plain / full = %.4f"
          % (med["batch"] / med["plain"], med["batch"] / med["full"], med["plain"] / med["full"]))
    print("batch info: %s" % engines["batch"].batch_info())


if __name__ == "__main__":
    main()
