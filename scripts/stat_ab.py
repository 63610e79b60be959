#!/usr/bin/env python3
"""Interleaved A/B timing of the small kernels (nsfnet_amd/csrc/fixed_fold.h users) between two builds of the library.

  python scripts/stat_ab.py --parent-lib /path/to/parent/libnsfnet_pinn.so [--rounds 5] [--out FILE]

Each round runs, for the parent's library and then for this tree's, two fresh processes chosen by $NSFNET_PINN_LIB: this
script with --time (the entry points below at the headline 6x256 + 4x40 sizes, HIP events around 200 back-to-back
calls, the median of five such batches, in microseconds per call) and bench.py (ms per training step, with the last
step's outputs dumped and compared bit for bit against the parent's of the same round).  Verdict per row: the change's
median against the spread (min..max) of the parent's runs of this session."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P_MAIN, P_E = 330499, 5161


def time_entry_points():
    import numpy as np
    import torch
    from nsfnet_amd import _lib, engine as eng
    from nsfnet_amd.schedule import LrSchedule
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import stat_fingerprint as fp
    lib, ptr, dev, DEV = _lib.load(), eng._ptr, fp.dev, fp.DEV
    items = {}

    flat = dev(fp.vec(P_MAIN + P_E, 1))
    sq_scratch = eng.grad_sqnorm_scratch(DEV)
    items["pinn_grad_sqnorm"] = lambda: eng.grad_sqnorm(flat[:P_MAIN], flat[P_MAIN:], sq_scratch)

    p, m, v = (dev(fp.vec(P_MAIN, 2 + k)) for k in range(3))
    v.abs_()
    t, epoch = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    rec = torch.zeros(eng.OPTIM_RECORD, dtype=torch.float64, device=DEV)
    spec = LrSchedule("cosine", t_max=2500, eta_min=1e-6).c_struct()
    g = flat[:P_MAIN]
    items["pinn_adam_step_sched"] = lambda: lib.pinn_adam_step_sched(
        ptr(p), ptr(g), ptr(m), ptr(v), P_MAIN, ctypes.byref(spec), 1e-3, 0.9, 0.999, 1e-8, ptr(t), ptr(epoch), 1,
        ptr(sq_scratch), 1.0, ptr(rec), fp.stream())

    n = 360000
    plan = fp.planes(n, 3)
    lam, w = torch.ones(n, device=DEV), torch.ones(n, device=DEV)
    rba_scratch = eng.rba_scratch(n, DEV)
    rba_rec = torch.zeros(eng.RBA_RECORD, dtype=torch.float64, device=DEV)

    def rba():
        eng.rba_stats(plan, 0.1, rba_scratch)
        eng.rba_apply(plan, 0.1, 0.999, 0.01, None, None, lam, w, rba_scratch, rba_rec)
    items["pinn_rba_stats + pinn_rba_apply (360000)"] = rba

    nv = 257 * 257
    rng = np.random.RandomState(4)
    tgt, pred = eng.val_planes(nv, DEV), eng.val_planes(nv, DEV)
    tgt[:, :nv], pred[:, :nv] = dev(rng.randn(3, nv).astype(np.float32)), dev(rng.randn(3, nv).astype(np.float32))
    val_scratch = eng.val_scratch(DEV)
    st = torch.zeros(eng.VAL_STATE, dtype=torch.float64, device=DEV)
    ring = torch.zeros(64, eng.VAL_RECORD, dtype=torch.float64, device=DEV)
    items["pinn_val_stats (257 x 257)"] = lambda: eng.val_stats(pred, tgt, nv, True, 0, -1.0, 5, val_scratch, st, ring)

    vecs = [dev(fp.vec(P_MAIN, 5 + k)) for k in range(3)]
    parts = eng.confgrad_partials(P_MAIN, DEV)
    eng.confgrad_gram(vecs, P_MAIN, parts)
    coef = torch.zeros(3, device=DEV)
    cf_rec = torch.zeros(eng.CONFGRAD_RECORD, dtype=torch.float64, device=DEV)
    items["pinn_confgrad_coef"] = lambda: eng.confgrad_coef(parts, P_MAIN, 3, coef, cf_rec)

    hist = eng.LbfgsHistory(P_MAIN, 7, DEV)
    hist.reset()
    cdiag, x = 1.0 + dev(fp.vec(P_MAIN, 20)).abs(), dev(fp.vec(P_MAIN, 21))
    for k in range(9):                                  # a convex quadratic: every pair is accepted, the history fills
        gk = cdiag * x
        hist.direction(gk, 0.0 if k == 0 else 0.5)
        x = x + 0.5 * hist.d
    assert hist.result[5].item() == 7.0, hist.result
    items["pinn_lbfgs_direction (m = 7)"] = lambda: hist.direction(gk, 0.5)      # y = 0: rejected, the 7 pairs stay

    out = {}
    for name, fn in items.items():
        for _ in range(20):
            fn()
        batches = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(200):
                fn()
            b.record()
            torch.cuda.synchronize()
            batches.append(a.elapsed_time(b) * 1e3 / 200)
        out[name] = statistics.median(batches)
    print(json.dumps(out), flush=True)


def child(lib, argv, timeout):
    env = dict(os.environ)
    env.pop("NSFNET_PINN_LIB", None)
    if lib:
        env["NSFNET_PINN_LIB"] = lib
    r = subprocess.run([sys.executable] + argv, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:       # a fault ends the session: nothing more is started on the device
        sys.exit("child %s failed (%d):\n%s" % (argv, r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="(child) time the entry points of $NSFNET_PINN_LIB, print one JSON line")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.time:
        return time_entry_points()
    import numpy as np
    runs = {"parent": {}, "change": {}}
    dumps_equal = []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            for side, lib in (("parent", os.path.abspath(a.parent_lib)), ("change", None)):
                res = child(lib, [os.path.abspath(__file__), "--time"], 300)
                d = os.path.join(tmp, "%s_%d" % (side, r))
                bench = child(lib, [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "10",
                                    "--sustain-seconds", "0", "--no-cpu-baseline", "--alt-precision", "", "--dump-outputs", d], 600)
                res["bench.py training step (ms)"] = bench["ms_per_step"]
                print("round %d %s %s" % (r, side, json.dumps(res)), file=sys.stderr, flush=True)
                for k, v in res.items():
                    runs[side].setdefault(k, []).append(v)
            pd, cd = (os.path.join(tmp, "%s_%d" % (s, r)) for s in ("parent", "change"))
            dumps_equal.append(all(np.load(os.path.join(pd, f)).tobytes() == np.load(os.path.join(cd, f)).tobytes()
                                   for f in sorted(os.listdir(pd))))
    lines = ["# us per call (the last row: ms per step), %d interleaved rounds; verdict: the change's median against the parent's min..max" % a.rounds]
    for k in runs["parent"]:
        pr, ch = runs["parent"][k], runs["change"][k]
        med = statistics.median(ch)
        verdict = "inside" if min(pr) <= med <= max(pr) else ("BELOW (faster)" if med < min(pr) else "ABOVE (slower)")
        fmt = lambda xs: " ".join("%.3f" % x for x in xs)
        lines.append("%-44s parent runs %s median %.3f spread [%.3f, %.3f] | change runs %s median %.3f  %s"
                     % (k, fmt(pr), statistics.median(pr), min(pr), max(pr), fmt(ch), med, verdict))
    lines.append("bench.py --dump-outputs of the last step, change against parent, per round: %s"
                 % " ".join("identical" if e else "DIFFERS" for e in dumps_equal))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
