"""L-BFGS iterations at the headline shape (6x256, 360 k points, bf16x3) for a kernel-trace profile:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/profile_lbfgs.py --history 20 --iters 20

No line search (one loss + gradient evaluation per iteration), so the per-iteration direction kernels (lb_*) and
the evaluation kernels appear in a 1 : 1 ratio.  With --iters > --history the history is full for the last
iterations.  Prints the wall time per iteration, then the evaluation and the direction call timed by CUDA events
(scripts/lbfgs_trace_summary.py breaks a trace down per kernel).  Kernel spans in a trace overlap: the boundary
chain runs on a second stream beside the collocation sweep, and its small kernels (loss_sums_kernel) wait there for
free CUs, so summing their spans over-counts an evaluation; the event times do not."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsfnet_amd import engine as eng  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=360000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    E = eng.PinnEngine(dev, 6, 256, 100.0, alpha_b=10.0, alpha_e=1.0, precision="bf16x3")
    E.net.set_flat(ar.flat_params(ar.seeded_net(3, 6, 256, seed=0)))
    rng = np.random.RandomState(0)
    E.set_collocation(rng.rand(a.points).astype(np.float32), rng.rand(a.points).astype(np.float32))
    E.set_boundary(*(v.reshape(-1).astype(np.float32) for v in ar.cavity_boundary()))
    for _ in range(20):
        E.step(1e-3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    E.lbfgs_step(lr=1e-2, max_iter=a.iters, tolerance_change=0.0, tolerance_grad=0.0, history_size=a.history)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("history %d: %d iterations, %.3f ms per iteration, pairs held %d, %s" % (
        a.history, a.iters, 1e3 * dt / a.iters, int(E._lbfgs.result[5].item()), E.lbfgs_info))
    # the two costs side by side, by CUDA events (wall time on the stream, overlap of the two streams included):
    # one loss + gradient evaluation, and one direction call at the held history (g = g_prev: y = 0, so the pair
    # is rejected - the passes over the history and the solve are those of an accepted step)
    def timed(fn, reps=20):
        fn()
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for _ in range(reps):
            fn()
        b0.record()
        torch.cuda.synchronize()
        return a0.elapsed_time(b0) / reps
    t_eval = timed(E.loss_and_grad)
    t_dir = timed(lambda: E._lbfgs.direction(E.grads, 1e-2))
    print("history %d: evaluation %.3f ms, direction %.1f us (%d pairs) = %.2f %% of an evaluation" % (
        a.history, t_eval, 1e3 * t_dir, int(E._lbfgs.result[5].item()), 100.0 * t_dir / t_eval))


if __name__ == "__main__":
    main()
