"""numpy model of the fixed-order fp64 folds of csrc/fixed_fold.h (TEST INFRASTRUCTURE; pure numpy, vectorised).  Every
function applies the same correctly rounded fp64 operations in the same order as its device namesake, so a result is
meant to be compared bit for bit.  An operation is (identity, apply)."""
import numpy as np

SUM = (0.0, lambda a, b: a + b)
NANMAX = (0.0, lambda a, b: np.where((b > a) | (b != b), b, a))      # of non-negative values; a NaN stays
MIN = (np.inf, lambda a, b: np.where(b < a, b, a))
MAX = (-np.inf, lambda a, b: np.where(b > a, b, a))
WAVE = 64


def _quiet(f):
    def g(*a, **k):
        with np.errstate(invalid="ignore", over="ignore"):
            return f(*a, **k)
    g.__doc__ = f.__doc__
    return g


@_quiet
def wave_fold(v, op=SUM):
    """v [..., 64] -> [...]: lane i takes lane i + 32, then + 16, ... + 1; lane 0's result."""
    v = np.asarray(v, dtype=np.float64)
    off = WAVE // 2
    while off > 0:
        # lanes >= off of the device tree take garbage that never reaches lane 0: only lanes < off are kept
        v = op[1](v[..., :off], v[..., off:2 * off])
        off //= 2
    return v[..., 0]


@_quiet
def ordered_fold(init, v, op=SUM):
    """init, then v[..., 0], v[..., 1], ... in order."""
    v = np.asarray(v, dtype=np.float64)
    acc = np.array(np.broadcast_to(init, v.shape[:-1]), dtype=np.float64)
    for i in range(v.shape[-1]):
        acc = op[1](acc, v[..., i])
    return acc


def block_fold(v, op=SUM):
    """v [..., THREADS] -> [...]: wave_fold of every wave, then the wave results in wave order from wave 0's."""
    v = np.asarray(v, dtype=np.float64)
    w = wave_fold(v.reshape(v.shape[:-1] + (-1, WAVE)), op)
    return ordered_fold(w[..., 0], w[..., 1:], op)


@_quiet
def strided_tree_fold(parts, ops, threads=256):
    """parts [nblk, C], column c with ops[c] -> [C]: thread t takes rows t, t + threads, ... in order from the
    identity, then the pairwise tree (thread i takes thread i + half)."""
    p = np.asarray(parts, dtype=np.float64).reshape(-1, len(ops))
    out = np.empty(len(ops))
    rows = -(-p.shape[0] // threads) * threads
    for c, op in enumerate(ops):
        col = np.full(rows, op[0])
        col[:p.shape[0]] = p[:, c]
        acc = np.full(threads, op[0])
        for chunk in col.reshape(-1, threads):
            acc = op[1](acc, chunk)         # a padded row applies the identity to a value that is never -0.0
        half = threads // 2
        while half > 0:
            acc = op[1](acc[:half], acc[half:2 * half])
            half //= 2
        out[c] = acc[0]
    return out


def chunk_fold(parts, op=SUM, threads=256):
    """parts [nblk] -> scalar: thread t takes rows [t ch, (t + 1) ch), ch = ceil(nblk / threads), in order from the
    identity, then the thread results in thread order from the identity."""
    p = np.asarray(parts, dtype=np.float64).reshape(-1)
    ch = max(-(-p.size // threads), 1)
    col = np.full(ch * threads, op[0])
    col[:p.size] = p
    return float(ordered_fold(op[0], ordered_fold(op[0], col.reshape(threads, ch), op), op))


def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


@_quiet
def fma(a, b, c):
    """a b + c with one rounding, as the device's fma: the product and the sum held exactly as pairs of doubles, the
    low parts added with rounding to odd (Boldo & Melquiond 2008).  For finite values away from over- and underflow."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    split = lambda x: (lambda t: (t - (t - x), x - (t - (t - x))))(134217729.0 * x)       # 2^27 + 1: 26-bit halves
    (ah, al), (bh, bl) = split(a), split(b)
    uh = a * b
    ul = (((ah * bh - uh) + ah * bl) + al * bh) + al * bl
    th, tl = _two_sum(c, uh)
    v, err = _two_sum(tl, ul)
    even = (np.ascontiguousarray(v).view(np.uint64) & np.uint64(1)) == 0
    v = np.where((err != 0.0) & even, np.nextafter(v, np.where(err > 0.0, np.inf, -np.inf)), v)
    return th + v


def grid_partials(values, nblk, op=SUM, threads=256, per=4):
    """The block partials [nblk] of a grid-stride kernel over values [n] (what each entry contributes; the identity
    for an entry the kernel skips): thread t of block b takes entries ((k nblk + b) threads + t) per + j for
    k = 0, 1, ... and j = 0 .. per - 1 in that order from the identity, then block_fold.  values = (x, y): the entry
    contributes x y, taken into the sum by one fma (0 for an entry the kernel skips)."""
    prod = isinstance(values, tuple)
    n = np.asarray(values[0] if prod else values).size
    tile = nblk * threads * per
    k = max(-(-n // tile), 1)

    def lay(v, fill):                                   # [nblk, threads, k per]: a thread's entries in its order
        pad = np.full(k * tile, fill)
        pad[:n] = np.asarray(v, dtype=np.float64).reshape(-1)
        return np.moveaxis(pad.reshape(k, nblk, threads, per), (0, 3), (2, 3)).reshape(nblk, threads, k * per)

    if not prod:
        return block_fold(ordered_fold(op[0], lay(values, op[0]), op), op)
    x, y = lay(values[0], 0.0), lay(values[1], 0.0)
    acc = np.zeros((nblk, threads))
    for i in range(k * per):
        acc = fma(x[..., i], y[..., i], acc)
    return block_fold(acc, SUM)


def grid_fold(values, nblk, op=SUM, threads=256, per=4):
    """grid_partials, then strided_tree_fold of the block partials: the whole reduction of a last-block kernel."""
    return float(strided_tree_fold(grid_partials(values, nblk, op, threads, per)[:, None], [op], threads)[0])


def same_bits(a, b):
    """Bitwise equality of two fp64 arrays, any NaN equal to any NaN (the payload is the hardware's choice)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
