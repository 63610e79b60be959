"""Census of pinn_plan_create's resolution:  python scripts/plan_census.py [--out FILE]

Walks a fixed list of (net, precision, streams, points, environment switches) cases and records what the library answers
for each plan: the padded point count, the workspace bytes without / with the backward part and the three reported
kernel names, or the return code and pinn_last_error() text of a refused plan.  The workspace bytes depend on every
grid, on the dW group count, on the tile size and on the spill format, so together with the names a row fingerprints the
whole resolution.  $NSFNET_PINN_LIB selects the build (nsfnet_amd/_lib.py).  tests/golden/plan_census.json is this
script's output on a host without a device (plans sized for 256 compute units); tests/test_plan_census.py compares the
current build with it.
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWITCHES = ("PINN_SCHED", "PINN_FWD_SCHED", "PINN_BWD_SCHED", "PINN_WSPLIT", "PINN_FUSE", "PINN_STAGGER",
            "PINN_S0_SKIP32", "PINN_VERBOSE", "PINN_TILE_COLS")
HIDDEN = (7, 40, 50, 128, 160, 256, 288, 400, 448, 480, 512)
DEPTHS = (1, 2, 6, 7, 8, 12, 40)      # 40 hidden layers: refused for LDS at hidden 256 and at hidden 512
UNIFORM = ((0, 0, 0), (1, 1, 1), (2, 2, 2))
TRIPLES = tuple(itertools.product((0, 1, 2), repeat=3))
POINTS = (1, 31, 2052, 360000, 4000000)
# every switch alone at each value the code distinguishes (and one outside them), then the per-sweep schedules mixed
ENVS = ([{"PINN_SCHED": v} for v in ("-1", "0", "1", "2", "3")] +
        [{"PINN_FWD_SCHED": v} for v in ("-1", "0", "1", "2", "3")] +
        [{"PINN_BWD_SCHED": v} for v in ("-1", "0", "1", "2", "3")] +
        [{"PINN_FWD_SCHED": f, "PINN_BWD_SCHED": b} for f in "012" for b in "012"] +
        [{"PINN_SCHED": "1", "PINN_FWD_SCHED": "2"}, {"PINN_SCHED": "0", "PINN_BWD_SCHED": "2"}] +
        [{k: v} for k in ("PINN_WSPLIT", "PINN_FUSE", "PINN_STAGGER", "PINN_S0_SKIP32", "PINN_VERBOSE") for v in "01"] +
        [{"PINN_TILE_COLS": v} for v in ("0", "64", "128")])
# nets of the switch sweep: the headline shape in three precisions, a deeper one (no fused sweeps), a wide one
# (hidden > 256) and hidden 128 (the other width $PINN_TILE_COLS applies to)
ENV_NETS = ((256, 6, (1, 1, 1)), (256, 6, (0, 0, 0)), (256, 8, (2, 2, 2)), (400, 8, (1, 1, 1)), (128, 4, (1, 1, 1)))


def cases():
    """[(hidden, layers, (prec_fwd, prec_bwd, prec_dw), streams, points, env dict)], in a fixed order."""
    out = []
    for H in HIDDEN:
        for L in DEPTHS:
            for prec in UNIFORM:
                out.append((H, L, prec, 4, 360000, {}))
        for L in (1, 6):
            for prec in UNIFORM:
                out.append((H, L, prec, 1, 2052, {}))
    for prec in TRIPLES:
        for streams in (4, 1):
            out.append((256, 6, prec, streams, 360000, {}))
    for H in (50, 256):
        for n in POINTS:
            for prec in UNIFORM:
                for streams in (4, 1):
                    out.append((H, 6, prec, streams, n, {}))
    for H, L, prec in ENV_NETS:
        for env in ENVS:
            out.append((H, L, prec, 4, 360000, env))
    for env in ENVS[-3:]:                     # $PINN_TILE_COLS on the value plans too
        for H in (128, 256):
            out.append((H, 6, (0, 0, 0), 1, 2052, env))
    seen = set()                              # (the sweeps overlap in a few cases: each is walked once)
    return [c for c in out if not (key(c) in seen or seen.add(key(c)))]


def key(case):
    H, L, prec, streams, n, env = case
    return " ".join(["H%d L%d p%d%d%d s%d n%d" % ((H, L) + tuple(prec) + (streams, n))] +
                    ["%s=%s" % kv for kv in sorted(env.items())])


def run_case(lib, case):
    """The census row of one case: [key, 0, padded points, bytes forward-only, bytes in all, kernel 0, 1, 2], or
    [key, return code, last-error text] when the plan is refused.  The switches are set for the lifetime of the net:
    $PINN_TILE_COLS is read when the net is created and when its precision is set, the others at plan creation."""
    H, L, prec, streams, n, env = case
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        assert lib.pinn_net_create(3, L, H, ctypes.byref(net)) == 0, lib.pinn_last_error()
        assert lib.pinn_net_set_precision(net, *prec) == 0, lib.pinn_last_error()
        rc = lib.pinn_plan_create(net, n, streams, ctypes.byref(plan))
        if rc != 0:
            return [key(case), rc, lib.pinn_last_error().decode()]
        row = [key(case), 0, lib.pinn_plan_padded_points(plan), lib.pinn_plan_workspace_bytes(plan, 0),
               lib.pinn_plan_workspace_bytes(plan, 1)] + [lib.pinn_plan_kernel(plan, k).decode() for k in (0, 1, 2)]
        lib.pinn_plan_destroy(plan)
        return row
    finally:
        if net:
            lib.pinn_net_destroy(net)
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def census(lib):
    return [run_case(lib, c) for c in cases()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the rows here (default: stdout)")
    args = ap.parse_args()
    from nsfnet_amd import _lib
    rows = census(_lib.load())
    text = "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
        print("%d rows, %d refused -> %s" % (len(rows), sum(1 for r in rows if r[1] != 0), args.out))
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
