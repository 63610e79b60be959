#!/usr/bin/env python3
"""Fingerprint what the small kernels compute (the fixed-order fp64 reductions of nsfnet_amd/csrc/fixed_fold.h and the
Adam update), case by case, on the device: one sha256 per case over the raw bytes of every output, records, scratch
words and ticket words included.

  python scripts/stat_fingerprint.py [--out FILE] [--only TEXT]
  NSFNET_PINN_LIB=/path/to/other/libnsfnet_pinn.so python scripts/stat_fingerprint.py --out other.txt

For comparing two builds of the library on one machine by hand (a refactor of these kernels must leave every line
equal); the hashes are not a fixture.  The inputs are seeded numpy arrays at the sizes where each loop can go wrong,
not the workload's: one entry, one past a wave or a block, sizes past the grid caps (so the grid-stride loops repeat
and a thread of the last-block fold takes two partials), with a NaN and an all-zero variant where the entry point has
guards."""
import argparse
import ctypes
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsfnet_amd import _lib, engine as eng  # noqa: E402
from nsfnet_amd.schedule import LrSchedule  # noqa: E402

DEV = torch.device("cuda:0")
P_MAIN, P_E = 330499, 5161        # the 6x256 main net and the 4x40 entropy net
ptr = eng._ptr


def dev(a, dtype=None):
    return None if a is None else torch.tensor(a, dtype=dtype, device=DEV)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def vec(n, seed, variant=""):
    rng = np.random.RandomState(seed)
    v = (rng.randn(n) * 10.0 ** rng.uniform(-4, 1, size=n)).astype(np.float32)
    if variant == "zero":
        v[:] = 0.0
    if variant == "nan":
        v[n // 2] = np.nan
    return v


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- the cases: generators of (name, sha256)
def sqnorm():
    for n0, n1 in [(1, 0), (65, 0), (P_MAIN, 0), (P_MAIN, P_E)]:
        for variant in ("", "nan", "zero"):
            flat = dev(vec(n0 + n1, n0 + n1, variant))
            scratch = eng.grad_sqnorm_scratch(DEV)
            eng.grad_sqnorm(flat[:n0], flat[n0:] if n1 else None, scratch)
            yield "grad_sqnorm %d+%d %s" % (n0, n1, variant), digest(scratch)


def adam():
    lib = _lib.load()
    spec = LrSchedule("cosine", t_max=2500, eta_min=1e-6, warmup_epochs=100, warmup_start=0.1).c_struct()
    for n in (1, 257, P_MAIN):
        rng = np.random.RandomState(n)
        init = [rng.randn(n).astype(np.float32), (0.1 * rng.randn(n)).astype(np.float32),
                (0.01 * rng.rand(n)).astype(np.float32)]
        grads = [dev(vec(n, 10 * n + k)) for k in range(3)]
        for kind in ("step", "dev", "sched", "sched clip"):
            p, m, v = (dev(a) for a in init)
            t = torch.tensor([4, 0], dtype=torch.int64, device=DEV)
            epoch = torch.tensor([37], dtype=torch.int64, device=DEV)
            rec = torch.zeros(eng.OPTIM_RECORD, dtype=torch.float64, device=DEV)
            scratch = eng.grad_sqnorm_scratch(DEV)
            for k, g in enumerate(grads):
                if kind == "step":
                    rc = lib.pinn_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, 5 + k, stream())
                elif kind == "dev":
                    rc = lib.pinn_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, ptr(t), stream())
                else:
                    sq = None
                    if kind == "sched clip":
                        eng.grad_sqnorm(g, None, scratch)
                        sq = scratch
                    rc = lib.pinn_adam_step_sched(ptr(p), ptr(g), ptr(m), ptr(v), n, ctypes.byref(spec), 1e-3, 0.9, 0.999, 1e-8,
                                                  ptr(t), ptr(epoch), 1, ptr(sq), 0.05, ptr(rec), stream())
                _lib.check(rc, "pinn_adam_step " + kind)
            yield "adam %s n=%d" % (kind, n), digest(p, m, v, t, epoch, rec)


def combiners():
    for P in (1, 257, P_MAIN):
        for nterms in (2, 3):
            for variant in ("", "nan", "zero"):
                vecs = [dev(vec(P, P + 1)), dev(vec(P, P + 2, variant)), dev(vec(P, P + 3)) if nterms == 3 else None]
                name = "P=%d terms=%d %s" % (P, nterms, variant)
                parts = eng.balance_partials(P, DEV)
                lam = torch.tensor([10.0, 1.0], device=DEV)
                rec = torch.zeros(eng.BALANCE_RECORD, dtype=torch.float64, device=DEV)
                rec[9], rec[10] = 10.0, 1.0
                g = torch.zeros(P, device=DEV)
                eng.balance_stats(vecs, P, parts)
                eng.balance_update(parts, P, 3 if nterms == 3 else 1, 0.1, lam, rec)
                eng.balance_combine(g, vecs[0], vecs[1], vecs[2], lam)
                yield "balance " + name, digest(parts, lam, rec, g)
                parts = eng.confgrad_partials(P, DEV)
                coef = torch.zeros(3, device=DEV)
                rec = torch.zeros(eng.CONFGRAD_RECORD, dtype=torch.float64, device=DEV)
                eng.confgrad_gram(vecs, P, parts)
                eng.confgrad_coef(parts, P, nterms, coef, rec)
                eng.confgrad_combine(g, vecs[0], vecs[1], vecs[2], coef)
                yield "confgrad " + name, digest(parts, coef, rec, g)


def reduce_terms():
    rng = np.random.RandomState(24)
    E = eng.PinnEngine(DEV, 3, 24, 400.0, alpha_b=10.0, alpha_e=1.0, alpha_s=1.0, precision="fp32")
    E.net.set_flat(torch.tensor((rng.randn(E.net.num_params) / np.sqrt(24)).astype(np.float32)))
    pts = lambda m: tuple(rng.rand(m).astype(np.float32) for _ in range(2))
    E.set_collocation(*pts(520))
    E.set_boundary(*pts(33), *(rng.randn(33).astype(np.float32) for _ in range(2)))
    E.set_supervised(*pts(45), *(rng.randn(45).astype(np.float32) for _ in range(2)))
    E.loss_and_grad()
    groups = [[E.plan_f], [E.plan_b], [E.plan_s]]
    outs = [torch.zeros(E.P, device=DEV) for _ in range(3)]
    parts, gram = eng.balance_partials(E.P, DEV), eng.confgrad_partials(E.P, DEV)
    eng.grad_reduce_terms(E.net, groups, outs, partials=parts)
    yield "grad_reduce_terms 3x24 N=520", digest(*outs, parts)
    eng.grad_reduce_terms(E.net, groups, outs, acc_mask=2, partials=parts, gram=gram)
    yield "grad_reduce_terms_gram 3x24 N=520", digest(*outs, parts, gram)


def planes(n, seed, variant=""):
    """A stand-in for an evaluated ResidualPlan: random field planes [FLD_COUNT, npad], the padding NaN."""
    npad = (n + 31) // 32 * 32
    rng = np.random.RandomState(seed)
    f = (rng.randn(eng.FLD_COUNT, npad) * 10.0 ** rng.uniform(-3, 1, size=(1, npad))).astype(np.float32)
    if variant == "zero":
        f[:] = 0.0
    if variant == "nan":
        f[eng.FLD["eq2"], n // 2] = np.nan
    f[:, n:] = np.nan
    return SimpleNamespace(n=n, npad=npad, fields=torch.tensor(f, device=DEV))


SIZES = [1, 7, 1003, 1024, 70001, 600013]


def rba():
    for n in SIZES:
        for w4 in (0.0, 0.1):
            for variant in ("", "nan", "zero"):
                plan = planes(n, n, variant)
                for with_idx in (False, True):
                    n_store = 2 * n + 3 if with_idx else n
                    rng = np.random.RandomState(n + 2)
                    s = dev((0.2 + rng.rand(n_store)).astype(np.float32))
                    lam, w = torch.zeros(n_store, device=DEV), torch.zeros(n_store, device=DEV)
                    idx = dev(n_store - 1 - 2 * np.arange(n, dtype=np.int64)) if with_idx else None
                    rec = torch.zeros(eng.RBA_RECORD, dtype=torch.float64, device=DEV)
                    scratch = eng.rba_scratch(n, DEV)
                    eng.rba_fill(1.7, s, lam, w)
                    eng.rba_stats(plan, w4, scratch)
                    eng.rba_apply(plan, w4, 0.999, 0.01, idx, s, lam, w, scratch, rec)
                    yield "rba n=%d w4=%s idx=%d %s" % (n, w4, with_idx, variant), digest(lam, w, rec, scratch[:8])


def val():
    for n in SIZES:
        for with_p in (False, True):
            for variant in ("", "nan"):
                rng = np.random.RandomState(n + with_p)
                tgt, pred = eng.val_planes(n, DEV), eng.val_planes(n, DEV)
                t = (rng.randn(3, n) * 10.0 ** rng.uniform(-3, 1, size=(3, n))).astype(np.float32)
                p = (t + 0.1 * rng.randn(3, n)).astype(np.float32)
                if variant == "nan":
                    t[2, ::10] = np.nan                     # masked pressure targets
                    p[0, n // 2] = np.nan                   # and a NaN prediction
                tgt.fill_(float("nan")); pred.fill_(float("nan"))
                tgt[:, :n], pred[:, :n] = dev(t), dev(p)
                scratch = eng.val_scratch(DEV)
                st = torch.zeros(eng.VAL_STATE, dtype=torch.float64, device=DEV)
                st[1] = float("inf")
                ring = torch.zeros(4, eng.VAL_RECORD, dtype=torch.float64, device=DEV)
                for _ in range(2):
                    eng.val_stats(pred, tgt, n, with_p, eng.VAL_METRICS["p0" if with_p else "uv"], -1.0, 5, scratch, st, ring)
                yield "val_stats n=%d p=%d %s" % (n, with_p, variant), digest(scratch[:16], st, ring)


def resample():
    for n in (1003, 70001, 600013):
        rng = np.random.RandomState(n)
        src = {k: dev(rng.rand(n).astype(np.float32)) for k in ("x", "y", "w", "vtm")}
        for k in (0.0, 1.0, 2.0, 3.0):
            for w4, variant in ((0.1, ""), (0.0, ""), (0.1, "nan"), (0.1, "zero")):
                pool = planes(n, n + 5, variant)
                scratch = eng.resample_scratch(n, DEV)
                m = n // 2 + 1
                out, _ = eng.resample_select(pool, w4, k, 1.0, 0.375, m, scratch)
                head = scratch[:32].clone()
                name = "resample n=%d k=%g w4=%s %s" % (n, k, w4, variant)
                if variant == "nan":                        # S reports it; the selection is the caller's to discard
                    yield name, digest(head)
                    continue
                lo, hi = 3, m
                dst = {key: torch.zeros(hi - lo, device=DEV) for key in src}
                w_sum = torch.zeros(1, dtype=torch.float64, device=DEV)
                eng.resample_gather(out, lo, hi, n, src, dst, scratch, w_sum)
                yield name, digest(out, head, dst["x"], dst["y"], dst["w"], dst["vtm"], w_sum)


def lbfgs():
    for n in (1, 257, P_MAIN, 1125203):
        for m in (1, 7):
            for variant in ("", "nan") if n == 257 else ("",):
                hist = eng.LbfgsHistory(n, m, DEV)
                hist.reset()
                outs = []
                for k, t_prev in enumerate((0.0, 0.5, 0.25)):
                    g = dev(vec(n, 7 * n + k, variant if k == 2 else ""))
                    outs.append(hist.direction(g, t_prev).clone())
                    outs.append(hist.d.clone())
                outs.append(hist.probe(dev(vec(n, 7 * n + 3))).clone())
                yield "lbfgs n=%d m=%d %s" % (n, m, variant), digest(*outs)


def rwf():
    for L, H in ((3, 24), (6, 256)):
        rng = np.random.RandomState(L * H)
        net = eng.DeviceNet(3, L, H, DEV)
        net.set_flat(torch.tensor((rng.randn(net.num_params) / np.sqrt(H)).astype(np.float32)))
        net.set_factorization(np.exp(rng.normal(1.0, 0.1, size=net.rwf_rows)).astype(np.float32))
        gtheta = net.rwf_grad(dev(vec(net.num_params, L + H)))
        yield "rwf_grad %dx%d" % (L, H), digest(gtheta)


GROUPS = [sqnorm, adam, combiners, reduce_terms, rba, val, resample, lbfgs, rwf]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="print the cases whose name contains this")
    a = ap.parse_args()
    lines = []
    for group in GROUPS:
        for name, sha in group():
            if a.only in name:
                lines.append("%s | %s" % (name.strip(), sha))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
