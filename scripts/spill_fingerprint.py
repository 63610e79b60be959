#!/usr/bin/env python3
"""Fingerprint what the kernels of a plan compute, case by case, on the device: one sha256 per case over the field
planes, the loss sums, the full gradient (pinn_grad_reduce) and, where there is an entropy input, ebar and the
entropy net's gradient.

  python scripts/spill_fingerprint.py [--out FILE]          one line per case: name, kernels, sha256
  python scripts/spill_fingerprint.py --only 4x400 --parts  the cases whose name contains 4x400, a digest per output too
  NSFNET_PINN_LIB=/path/to/other/libnsfnet_pinn.so python scripts/spill_fingerprint.py --out other.txt

For comparing two builds of the library on one machine by hand (a refactor of the kernels must leave every line
equal); the hashes are not a fixture.  The cases cover the four layouts of the S / Z-bar spill (nsfnet_amd/csrc/spill.h)
with every kernel that writes or reads them, and the geometries of the 8-wave bf16 sweeps (fwd_bf16.hip, bwd_bf16.hip
and their _wide variants).  N = 69 collocation points give an odd tile count and a ragged last tile at
32 and at 16 points per tile; one case per layout has N = 20001, where the tile index exceeds the grid, so that the
persistent loops and the dummy partner tile of the paired sweeps run; the value-mode cases carry supervised targets at
N = 197 (two ragged tiles at 128 points per tile, four at 64)."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_TILE_COLS", "PINN_STAGGER",
            "PINN_FUSE", "PINN_S0_SKIP32", "NSFNET_CHUNK_POINTS")
X3, F32 = "bf16x3", "fp32"


def case(name, L, H, prec, env=(), n=69, ev=False, sup=0):
    return dict(name=name, L=L, H=H, prec=prec, env=dict(env), n=n, ev=ev, sup=sup)


CASES = [
    case("4x50 fp32", 4, 50, F32),
    case("4x50 fp32 S0_SKIP32=0", 4, 50, F32, {"PINN_S0_SKIP32": "0"}),
    case("6x256 fp32", 6, 256, F32),
    case("6x256 bf16x3", 6, 256, X3),
    case("6x256 bf16x3 FUSE=0", 6, 256, X3, {"PINN_FUSE": "0"}),
    case("6x256 bf16x3 SCHED=1", 6, 256, X3, {"PINN_SCHED": "1"}),
    case("6x256 bf16x3 SCHED=0", 6, 256, X3, {"PINN_SCHED": "0"}),
    case("6x256 bf16x3 SCHED=0 TILE_COLS=64", 6, 256, X3, {"PINN_SCHED": "0", "PINN_TILE_COLS": "64"}),
    case("6x256 (1,1,0)", 6, 256, "bf16x3,bf16x3,fp32"),
    case("6x256 (0,0,1)", 6, 256, "fp32,fp32,bf16x3"),
    case("6x256 bf16", 6, 256, "bf16"),
    case("4x400 fp32", 4, 400, F32),
    case("4x400 bf16x3", 4, 400, X3),
    case("4x400 bf16x3 WSPLIT=0", 4, 400, X3, {"PINN_WSPLIT": "0"}),
    case("4x400 (1,1,0)", 4, 400, "bf16x3,bf16x3,fp32"),
    case("3x480 bf16x3", 3, 480, X3),
    case("6x256+4x40 ev bf16x3", 6, 256, X3, ev=True),
    # the 8-wave bf16 sweeps (wave8_bodies.h) where the cases above do not reach them: 128-column tiles at two workgroups
    # per CU, 64-column tiles by choice, TERMS = 1, a last wave that owns one block, hidden 512
    case("4x50 bf16x3", 4, 50, X3),
    case("4x50 bf16", 4, 50, "bf16"),
    case("6x128 bf16x3 TILE_COLS=64", 6, 128, X3, {"PINN_TILE_COLS": "64"}),
    case("6x128 bf16x3 TILE_COLS=128", 6, 128, X3, {"PINN_TILE_COLS": "128"}),
    case("6x256 bf16 SCHED=0", 6, 256, "bf16", {"PINN_SCHED": "0"}),
    case("3x288 bf16x3 WSPLIT=0", 3, 288, X3, {"PINN_WSPLIT": "0"}),
    case("4x400 bf16 WSPLIT=0", 4, 400, "bf16", {"PINN_WSPLIT": "0"}),
    case("3x512 bf16x3", 3, 512, X3),
    # one per layout where the tile index exceeds the grid
    case("4x50 fp32 S0_SKIP32=0 N=20001", 4, 50, F32, {"PINN_S0_SKIP32": "0"}, n=20001),      # classic
    case("6x256 fp32 N=20001", 6, 256, F32, n=20001),                                          # fp32, layer 0 not stored
    case("4x400 bf16x3 N=20001", 4, 400, X3, n=20001),                                         # 24-bit, classic-sized blocks
    case("6x256 bf16x3 N=20001", 6, 256, X3, n=20001),                                         # 24-bit compact
    case("6x256 bf16x3 SCHED=0 N=20001", 6, 256, X3, {"PINN_SCHED": "0"}, n=20001),            # 8-wave sweeps, classic
    case("4x400 bf16x3 WSPLIT=0 N=20001", 4, 400, X3, {"PINN_WSPLIT": "0"}, n=20001),          # 8-wave wide sweeps, 24-bit
    # value-mode plans with targets
    case("4x50 fp32 value N=197", 4, 50, F32, sup=197),
    case("6x256 bf16x3 value N=197", 6, 256, X3, sup=197),
    case("4x400 bf16x3 value N=197", 4, 400, X3, sup=197),
    case("4x50 bf16x3 value N=197", 4, 50, X3, sup=197),
    case("6x256 bf16x3 TILE_COLS=64 value N=197", 6, 256, X3, {"PINN_TILE_COLS": "64"}, sup=197),
    case("3x480 bf16x3 value N=197", 3, 480, X3, sup=197),
]


def run(c, parts_too=False):
    from nsfnet_amd import engine as eng
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(c["env"])
    rng = np.random.RandomState(1000 + c["L"] * 7 + c["H"])
    kw = dict(flavour="ev", n_hidden_e=4, hidden_e=40, alpha_evm=0.05, coord_scale=2.0) if c["ev"] else {}
    E = eng.PinnEngine(torch.device("cuda:0"), c["L"], c["H"], 1000.0, alpha_b=10.0, alpha_e=1.0, alpha_s=1.0 if c["sup"] else 0.0,
                       precision=c["prec"], **kw)

    def flat(net, fan_in):
        return torch.tensor((rng.randn(net.num_params) / np.sqrt(fan_in)).astype(np.float32))

    E.net.set_flat(flat(E.net, c["H"]))
    if c["ev"]:
        E.net_e.set_flat(flat(E.net_e, 40))
        E.e_trainable = True
    pts = lambda m: tuple(rng.rand(m).astype(np.float32) for _ in range(2))
    x, y = pts(c["n"])
    E.set_collocation(x, y, weights=(0.3 + rng.rand(c["n"])).astype(np.float32) if c["ev"] else None)
    nb = c["sup"] or 33
    E.set_boundary(*pts(nb), *(rng.randn(nb).astype(np.float32) for _ in range(2)))
    if c["sup"]:
        p = rng.randn(c["sup"]).astype(np.float32)
        p[::5] = np.nan       # a masked pressure target
        E.set_supervised(*pts(c["sup"]), *(rng.randn(c["sup"]).astype(np.float32) for _ in range(2)), p=p)
    names = E.plan_f.kernel_names()
    E.loss_and_grad()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    fld = sorted(eng.FLD, key=eng.FLD.get)
    parts = [(k, E.plan_f.field(k)) for k in fld] + [("sums", E.sums), ("grads", E.grads)]
    if c["ev"]:
        parts += [("ebar", E.plan_f.ebar[:c["n"]]), ("grads_e", E.grads_e), ("vis_t", E.plan_f.vis_t)]
    each = []
    for k, t in parts:
        b = t.detach().cpu().contiguous().numpy().tobytes()
        h.update(b)
        each.append("%s:%s" % (k, hashlib.sha256(b).hexdigest()[:8]))
    finite = all(bool(torch.isfinite(t).all()) for t in (E.sums, E.grads))
    del E
    torch.cuda.empty_cache()
    line = "%s | %s | %s%s" % (c["name"], " ".join(names), h.hexdigest(), "" if finite else " | NOT FINITE")
    return line + (" | " + " ".join(each) if parts_too else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    ap.add_argument("--parts", action="store_true", help="append a short digest of every output to each line")
    a = ap.parse_args()
    lines = []
    for c in CASES:
        if a.only not in c["name"]:
            continue
        lines.append(run(c, a.parts))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
