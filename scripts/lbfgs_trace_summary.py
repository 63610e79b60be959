"""Per-kernel breakdown of a rocprofv3 kernel trace of scripts/profile_lbfgs.py:

    python scripts/lbfgs_trace_summary.py <results.db> [<iterations>]

Prints, from the first L-BFGS kernel (lb_*) on, the calls and total time of every kernel, and the mean time of each
direction kernel over the last five iterations (pass C and finish also run once per evaluation as the probe; the
direction call is the first of each pair).  Kernel spans of the two streams overlap, so the sum of the evaluation
kernels is not an evaluation's wall time (profile_lbfgs.py prints that)."""
import collections
import sqlite3
import sys


def main(db, iters=None):
    con = sqlite3.connect(db)
    rows = con.execute("select s.kernel_name, d.start, d.end from rocpd_kernel_dispatch d "
                       "join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start").fetchall()
    i0 = next(i for i, r in enumerate(rows) if "lb_" in r[0])
    rows = rows[i0:]
    agg = collections.defaultdict(lambda: [0, 0.0])
    for n, a, b in rows:
        agg[n.split("(")[0]][0] += 1
        agg[n.split("(")[0]][1] += (b - a) * 1e-6
    for k, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print("  %-64s %5d calls %9.3f ms %9.1f us/call" % (k[:64], c, t, 1e3 * t / c))
    last = {}
    for k in ("lb_pass_a", "lb_colsum", "lb_update", "lb_pass_c", "lb_finish"):
        v = [(b - a) * 1e-3 for n, a, b in rows if k in n]
        if k in ("lb_pass_c", "lb_finish"):
            v = v[0::2]                    # direction, probe, direction, probe, ...
        last[k] = sum(v[-5:]) / len(v[-5:])
    print("  last 5 iterations: " + ", ".join("%s %.1f us" % kv for kv in last.items()) +
          ", total %.1f us" % sum(last.values()))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else None)
