"""fp64 numpy model of the residual-based attention update of csrc/rba.hip / pinn_rba_stats, pinn_rba_apply and
pinn_rba_fill (TEST INFRASTRUCTURE; pure numpy).  The definition (include/nsfnet_pinn.h):

    e2_j   = ((eq1^2 + eq2^2) + eq3^2) + w4 eq4^2          fp64 from the fp32 planes
    r_j    = sqrt(e2_j)
    rmax   = max_j r_j                                     NaN-propagating
    lam_i <- fp32(gamma lam_i + (eta r_j) / rmax)          i = idx[j], or j
    w_i   <- fp32(s_i (lam_i lam_i))                       of the stored fp32 lam_i; s absent = 1

numpy evaluates every one of these operations as one correctly rounded fp64 operation in the order written, which is
what the kernel's uncontracted fp64 intrinsics do."""
import numpy as np

RECORD = 12          # PINN_RBA_RECORD
R_RMAX, R_SUMS, R_MIN, R_MAX, R_SUM, R_COUNT, R_UPDATES, R_SKIPPED = 0, 1, 5, 6, 7, 8, 9, 10


def norms(eq, w4):
    """r [n] fp64 of the four residual rows eq [4, n] (fp32)."""
    q = np.asarray(eq, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
        if w4 != 0.0:
            e2 = e2 + float(w4) * (q[3] * q[3])
        return np.sqrt(e2)


def stats(eq, w4):
    """(rmax, [sum eq1^2 .. sum eq4^2]) in fp64; w4 = 0: the fourth row is not read and its sum is 0."""
    q = np.asarray(eq, dtype=np.float32).astype(np.float64)
    r = norms(eq, w4)
    rmax = float("nan") if np.isnan(r).any() else float(r.max())
    with np.errstate(all="ignore"):
        sums = [float(np.sum(q[k] * q[k])) for k in range(3)] + [float(np.sum(q[3] * q[3])) if w4 != 0.0 else 0.0]
    return rmax, sums


def ok(rmax):
    return bool(np.isfinite(rmax) and rmax > 0.0)


def weights(s, lam):
    """fp32 effective weights s lam^2 of the stored fp32 lam (s None = 1)."""
    l = np.asarray(lam, dtype=np.float32).astype(np.float64)
    s64 = 1.0 if s is None else np.asarray(s, dtype=np.float32).astype(np.float64)
    return (s64 * (l * l)).astype(np.float32)


def fill(n, init, s=None):
    lam = np.full(int(n), np.float32(init), dtype=np.float32)
    return lam, weights(s, lam)


def apply(eq, w4, gamma, eta, lam, s=None, idx=None, rmax=None, w=None, record=None):
    """One update.  eq [4, n]; lam / s / w [n_store] fp32 (w None: s lam^2); idx None or [n] int64 (entries outside
    [0, n_store) are skipped); rmax None: this call's own.  Returns (lam, w, record) as new arrays."""
    lam = np.array(lam, dtype=np.float32)
    w = weights(s, lam) if w is None else np.array(w, dtype=np.float32)
    rec = np.zeros(RECORD) if record is None else np.array(record, dtype=np.float64)
    own, sums = stats(eq, w4)
    rmax = own if rmax is None else float(rmax)
    rec[R_RMAX] = rmax
    rec[R_SUMS:R_SUMS + 4] = sums
    if not ok(rmax):
        rec[R_SKIPPED] += 1
        return lam, w, rec
    r = norms(eq, w4)
    n_store = lam.size
    i = np.arange(r.size) if idx is None else np.asarray(idx, dtype=np.int64)
    keep = (i >= 0) & (i < n_store)
    i, r = i[keep], r[keep]
    new = (float(gamma) * lam[i].astype(np.float64) + (float(eta) * r) / rmax).astype(np.float32)
    lam[i] = new
    s_i = None if s is None else np.asarray(s, dtype=np.float32)[i]
    w[i] = weights(s_i, new)
    n64 = new.astype(np.float64)
    rec[R_MIN] = n64.min() if n64.size else np.inf
    rec[R_MAX] = n64.max() if n64.size else -np.inf
    rec[R_SUM] = n64.sum()
    rec[R_COUNT] = n64.size
    rec[R_UPDATES] += 1
    return lam, w, rec


def bound(init, gamma, eta):
    """Upper bound of lam: max(init, eta / (1 - gamma)) (gamma = 1: unbounded)."""
    return float("inf") if gamma >= 1.0 else max(float(init), float(eta) / (1.0 - float(gamma)))
