"""How far the fp32 autograd reference of the factorised trajectory ends from its own fp64 run (DESIGN.md section 7.7;
the bars of tests/test_rwf_gpu.py::test_short_factorised_training_tracks_the_autograd_oracle are 4 x these figures):

    python scripts/rwf_reference_divergence.py [--steps 300]

CPU only, about a minute.  The shape, seeds and data of that test - 3x24, 512 points of RandomState(5), weights of
seeded_net(seed=77), Re 100, alpha_b 10, lr 1e-3, scale factors of set_weight_factorization(seed=0) - through
tests/rwf_model.RwfNet (W = diag(exp(s)) V under torch autograd, torch's Adam over (V, b, s)), once in fp32 and once in
fp64 from the same fp32 theta.  Prints the relative L2 distance of u, v, p at the collocation points and the relative
difference of the final loss."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    import rwf_model as rm
    from oracle import autograd_ref as ar
    L, H, N, Re = 3, 24, 512, 100.0
    shape = (3, L, H)
    rng = np.random.RandomState(5)
    x, y = rng.rand(N, 1), rng.rand(N, 1)
    flat0 = ar.flat_params(ar.seeded_net(3, L, H, seed=77)).numpy().copy()
    s0 = rm.draw(0, 0.5, 0.1, [shape])[0]
    theta0 = rm.split(flat0, s0, shape)
    out = {}
    for dtype in (torch.float32, torch.float64):
        net = rm.RwfNet(theta0, shape, dtype=dtype)
        o = ar.NSFnetOracle(net, Re, alpha_b=10.0, alpha_e=1.0, lr=1e-3)
        o.set_data(x, y, *ar.cavity_boundary())
        first = last = o.step()
        for _ in range(a.steps - 1):
            last = o.step()
        with torch.no_grad():
            uvp = net(torch.tensor(np.hstack([x, y]), dtype=dtype)).double().numpy()
        s = torch.cat([p.detach().reshape(-1) for p in net.s]).double().numpy()
        out[dtype] = (uvp, float(o.loss().detach()), s)
        print("%s: loss %.6e -> %.6e, scale factors moved by at most %.3e" % (
            str(dtype).split(".")[1], first, last, np.abs(s - s0).max()))
    (f32, l32, _), (f64, l64, _) = out[torch.float32], out[torch.float64]
    rel = [np.linalg.norm(f32[:, c] - f64[:, c]) / np.linalg.norm(f64[:, c]) for c in range(3)]
    rel.append(abs(l32 - l64) / abs(l64))
    print("fp32 against fp64 after %d steps, relative: u %.3e  v %.3e  p %.3e  loss %.3e" % (a.steps, *rel))
    print("4 x: u %.3e  v %.3e  p %.3e  loss %.3e" % tuple(4 * r for r in rel))


if __name__ == "__main__":
    main()
