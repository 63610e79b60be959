#!/usr/bin/env python3
"""Record what PinnEngine asks of the device, row by row, on the CPU fakes (tests/engine_call_rows.py).

  python scripts/record_engine_calls.py                  write tests/golden/engine_call_logs.json and
                                                         tests/golden/engine_state_headers.json
  python scripts/record_engine_calls.py --dump-params    print per row the hashes of the parameters and records

The fixture is recorded on the commit whose behaviour is to be kept and checked by tests/test_engine_call_logs.py on
every later one.  It holds the call logs as indices into one table of distinct entries (the evaluations repeat), and
the graph keys; the second file holds, per row, the header a training-state file of the driven engine would carry
(engine_call_rows.state_header).  The hashes are for comparing two commits on one machine by hand; they are not a fixture."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import engine_call_rows as rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump-params", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "engine_call_logs.json"))
    ap.add_argument("--out-headers", default=os.path.join(ROOT, "tests", "golden", "engine_state_headers.json"))
    a = ap.parse_args()
    if a.dump_params:
        for row in rows.ROWS:
            print(row["name"], json.dumps(rows.run(row, hashes=True)[3], sort_keys=True))
        return
    table, index, doc, headers = [], {}, {}, {}
    for row in rows.ROWS:
        log, keys, headers[row["name"]] = rows.run(row)
        ids = []
        for entry in log:
            k = json.dumps(entry)
            if k not in index:
                index[k] = len(table)
                table.append(entry)
            ids.append(index[k])
        doc[row["name"]] = dict(log=ids, keys=keys)
    with open(a.out, "w") as f:
        json.dump(dict(entries=table, rows=doc), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d rows, %d distinct entries, %d bytes" % (a.out, len(doc), len(table), os.path.getsize(a.out)))
    with open(a.out_headers, "w") as f:
        json.dump(headers, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%s: %d rows, %d bytes" % (a.out_headers, len(headers), os.path.getsize(a.out_headers)))


if __name__ == "__main__":
    main()
