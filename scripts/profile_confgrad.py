"""Cost of the conflict-free gradient combination at the headline shape (6x256, 360 k points, bf16x3, one GPU):

    python scripts/profile_confgrad.py [--rounds 5 --steps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/profile_confgrad.py --rounds 1 --steps 10

One engine, feature off and on, eager and graph-replayed steps, timed by CUDA events in alternating rounds (off / on,
off / on, ...) so that clock drift hits both alike.  A step is PinnEngine.step (loss + gradient + Adam).  Prints the
median ms per step of each arm and the difference to the off arm of the same launch mode."""
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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    E = eng.PinnEngine(dev, 6, 256, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3")
    E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=0)))
    rng = np.random.RandomState(0)
    E.set_collocation(rng.rand(a.points).astype(np.float32), rng.rand(a.points).astype(np.float32))
    E.set_boundary(*(v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary()))
    arms = [(launch, on) for launch in ("eager", "graph") for on in (False, True)]
    times = {arm: [] for arm in arms}
    for _ in range(a.rounds):
        for launch, on in arms:
            os.environ["NSFNET_GRAPH"] = "1" if launch == "graph" else "0"
            E.set_conflict_free_gradients(on)
            for _ in range(3):                   # warm-up (graph: the eager run, the capture and one replay)
                E.step(1e-4)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                E.step(1e-4)
            t1.record()
            torch.cuda.synchronize()
            times[(launch, on)].append(t0.elapsed_time(t1) / a.steps)
        print("record: %s" % E.conflict_info(), flush=True)
    med = {arm: float(np.median(v)) for arm, v in times.items()}
    for launch, on in arms:
        print("%-5s %-3s %.4f ms/step  (rounds: %s)" % (launch, "on" if on else "off", med[(launch, on)],
                                                       " ".join("%.4f" % t for t in times[(launch, on)])))
    for launch in ("eager", "graph"):
        off, on = med[(launch, False)], med[(launch, True)]
        print("%-5s on - off = %+.1f us  (%+.2f %%)" % (launch, 1e3 * (on - off), 100.0 * (on - off) / off))


if __name__ == "__main__":
    main()
