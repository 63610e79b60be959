"""CPU test of PinnEngine's host wiring: every row of tests/engine_call_rows.py - each training option alone and
combined, both flavours, a chunked and a supervised set - makes, call for call and launch argument for launch argument,
what tests/golden/engine_call_logs.json holds, and looks its captured step up under the recorded graph key.  The
fixture was recorded (scripts/record_engine_calls.py) on the commit before the engine's term combiners, evaluation mode
and graph key were given one shape each."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import engine_call_rows as rows  # noqa: E402

with open(os.path.join(os.path.dirname(__file__), "golden", "engine_call_logs.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_has_every_row():
    assert sorted(GOLDEN["rows"]) == sorted(r["name"] for r in rows.ROWS)


@pytest.mark.parametrize("row", rows.ROWS, ids=[r["name"] for r in rows.ROWS])
def test_row_makes_the_recorded_calls(row):
    want = GOLDEN["rows"][row["name"]]
    log, keys = rows.run(row)
    want_log = [GOLDEN["entries"][i] for i in want["log"]]
    for k, (got, exp) in enumerate(zip(log, want_log)):
        assert got == exp, "call %d of %d" % (k, len(want_log))
    assert len(log) == len(want_log)
    assert keys == want["keys"]
