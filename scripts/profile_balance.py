"""Cost of the adaptive loss-weight balancing at the headline shape (6x256, 360 k points, bf16x3, one GPU):

    python scripts/profile_balance.py [--rounds 5 --steps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/profile_balance.py --rounds 1 --steps 10

Three modes of one engine, timed by CUDA events in alternating rounds (A/B/C, A/B/C, ...) so that clock drift hits
all three alike: balancing off, on with plain steps only (every = 10^9 after the first, balancing, step) and on with
a balance step every step (every = 1).  A step is PinnEngine.step (eager: loss + gradient + Adam).  Prints the median
ms per step of each mode and the two ratios to the off mode."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsfnet_amd import engine as eng  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402

MODES = (("off", 0), ("plain", 10 ** 9), ("balance", 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--points", type=int, default=360000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    E = eng.PinnEngine(dev, 6, 256, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3")
    E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=0)))
    rng = np.random.RandomState(0)
    E.set_collocation(rng.rand(a.points).astype(np.float32), rng.rand(a.points).astype(np.float32))
    E.set_boundary(*(v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary()))
    times = {m: [] for m, _ in MODES}
    for _ in range(a.rounds):
        for mode, every in MODES:
            E.set_loss_balancing(every, 0.1)
            for _ in range(3):                   # warm-up; with every = 10^9 the first step is the balance step
                E.step(1e-4)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                E.step(1e-4)
            t1.record()
            torch.cuda.synchronize()
            times[mode].append(t0.elapsed_time(t1) / a.steps)
    med = {m: float(np.median(v)) for m, v in times.items()}
    for m, _ in MODES:
        print("%-8s %.4f ms/step  (rounds: %s)" % (m, med[m], " ".join("%.4f" % t for t in times[m])))
    print("plain / off = %.4f   balance / off = %.4f" % (med["plain"] / med["off"], med["balance"] / med["off"]))
    print("balance record: %s" % E.balance_info())


if __name__ == "__main__":
    main()
