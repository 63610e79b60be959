"""Cost of the convergence monitor on one GPU:

    python scripts/profile_monitor.py [--rounds 5 --steps 20] [--shape headline|headline-ev|ev] [--batch-points 36000]

Two engines with the same parameters and points, timed by CUDA events in alternating rounds (off, on, off, ...) so that
clock drift hits both alike: `off` (an engine that never heard of the feature) and `on` (set_convergence_monitor with
windows of 1000 updates, and re_eff_tol on the ev shapes).  A step is PinnEngine.step, first eager, then - the same
engines - replayed from a hipGraph.  --shape headline: 6x256, 360 000 points, bf16x3, the plain flavour: the monitor is
the one-workgroup observation launch alone.  --shape headline-ev: the same net and points on the ev flavour with a 4x40
entropy net: the vis_t statistics launch reads the 1.4 MB plane as well.  --shape ev: 6x80 + 4x40, 120 000 points.
--batch-points B: both engines draw a mini-batch of B points per step (the statistics then read the batch plan's plane).
Prints the median ms per step of each arm and mode, the difference, and the bytes the two launches move."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"headline": (6, 256, 360000, False), "headline-ev": (6, 256, 360000, True), "ev": (6, 80, 120000, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="headline")
    ap.add_argument("--points", type=int, default=0)
    ap.add_argument("--batch-points", type=int, default=0)
    a = ap.parse_args()
    from nsfnet_amd import engine as eng
    from oracle import autograd_ref as ar
    dev = torch.device("cuda:0")
    L, H, n, ev = SHAPES[a.shape]
    n = a.points or n
    rng = np.random.RandomState(0)
    x, y = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    bc = [v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary()]
    kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05) if ev else {}
    engines = {}
    for mode in ("off", "on"):
        E = eng.PinnEngine(dev, L, H, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3", **kw)
        E.net.set_flat(ar.flat_params(ar.seeded_net(3, L, H, seed=0)))
        if ev:
            E.net_e.set_flat(ar.flat_params(ar.seeded_net(1, 4, 40, seed=1)))
        E.set_collocation(x, y)
        E.set_boundary(*bc)
        if a.batch_points:
            E.set_batching(batch_points=a.batch_points, seed=0)
        if mode == "on":
            E.set_convergence_monitor(window=1000, re_eff_tol=1e-3 if ev else None)
        engines[mode] = E
    tag = "%s %dx%d %d pts%s" % (a.shape, L, H, n, " batch %d" % a.batch_points if a.batch_points else "")
    for graph in (False, True):
        os.environ["NSFNET_GRAPH"] = "1" if graph else "0"
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
        how = "graph" if graph else "eager"
        for m in engines:
            print("[%s %s] %-3s %.4f ms/step  (rounds: %s)" % (tag, how, m, med[m], " ".join("%.4f" % t for t in times[m])))
        spread = max(times["off"]) - min(times["off"])
        print("[%s %s] on - off = %+.1f us per step (%+.3f %%); spread of the off rounds %.1f us" % (
            tag, how, 1e3 * (med["on"] - med["off"]), 100.0 * (med["on"] / med["off"] - 1.0), 1e3 * spread))
    E = engines["on"]
    plane = 4 * (a.batch_points or n) if ev else 0
    obs = 4 * 24 + 8 * (2 * eng.MON_STATE + eng.MON_RECORD)
    i = E.monitor_info()
    print("[%s] bytes per step: vis_t statistics %d read (+ %d of partials), observation about %d; updates %d, "
          "observations %d, graphs %d" % (tag, plane, 0 if not ev else 8 * 3 * min(512, -(-(a.batch_points or n) // 1024)),
                                          obs, i["updates"], i["observations"], len(E._graphs)))
    print("[%s] kernels: %s" % (tag, "/".join(E.plan_f.kernel_names())))


if __name__ == "__main__":
    main()
