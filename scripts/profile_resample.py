"""Cost of one collocation-point resample (PinnEngine.resample) at a production shape.

    python scripts/profile_resample.py [--layers 6 --hidden 256 --precision bf16x3 --points 360000 --pool 4000000]

Times, with device events after a warm-up resample: one training step, the pool forward (entropy net and residual
plan, forward only) and the select + gather calls; prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel times (rs_partial_kernel, rs_scan_kernel, rs_emit_kernel,
rs_gather_kernel, rs_wsum_kernel)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsfnet_amd import engine as eng  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--points", type=int, default=360000)
    ap.add_argument("--pool", type=int, default=4000000)
    ap.add_argument("--every", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    E = eng.PinnEngine(dev, a.layers, a.hidden, 2000.0, alpha_b=10.0, precision=a.precision)
    E.net.set_flat(torch.randn(E.net.num_params) * 0.1)
    rng = np.random.default_rng(0)
    E.set_collocation(rng.random(a.points).astype(np.float32), rng.random(a.points).astype(np.float32))
    t = np.linspace(0, 1, 513, dtype=np.float32)
    E.set_boundary(t, np.ones_like(t), np.ones_like(t), np.zeros_like(t))
    E.set_resample_pool(rng.random(a.pool).astype(np.float32), rng.random(a.pool).astype(np.float32))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        out = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            out.append(ev[0].elapsed_time(ev[1]))
        return float(np.median(out))

    E.step(1e-4)
    E.resample()                                             # warm-up
    step_ms = timed(lambda: E.step(1e-4))
    pool_ms = timed(lambda: E._pool.forward(E.Re, save=False))
    resample_ms = timed(lambda: E.resample())
    # the select call alone, on the evaluated pool and on a pool whose mass sits on one point (c = 0, k = 2: that point
    # takes ~all M copies, which its block writes together)
    pool, scratch, M = E._pool, E._pool_scratch, E.plan_f.n
    select_ms = timed(lambda: eng.resample_select(pool, 0.0, 1.0, 1.0, 0.5, M, scratch))
    pool.fields[6:10] *= 1e-3
    pool.fields[6, pool.n // 3] = 1e4
    idx, _ = eng.resample_select(pool, 0.0, 2.0, 0.0, 0.5, M, scratch)
    share = float((idx == pool.n // 3).double().mean())
    select_conc_ms = timed(lambda: eng.resample_select(pool, 0.0, 2.0, 0.0, 0.5, M, scratch))
    print(json.dumps(dict(shape="%dx%d %s" % (a.layers, a.hidden, a.precision), points=a.points, pool=a.pool,
                          step_ms=step_ms, pool_forward_ms=pool_ms, resample_ms=resample_ms,
                          select_and_gather_ms=resample_ms - pool_ms, select_ms=select_ms,
                          select_concentrated_ms=select_conc_ms, concentrated_top_share=share,
                          amortised_ms_per_step=resample_ms / a.every, every=a.every)))


if __name__ == "__main__":
    main()
