"""CPU test of PinnEngine's host wiring: every row of tests/engine_call_rows.py - each training option alone and
combined, both flavours, a chunked and a supervised set - makes, call for call and launch argument for launch argument,
what tests/golden/engine_call_logs.json holds, looks its captured step up under the recorded graph key, and would write
the training-state header tests/golden/engine_state_headers.json holds.  The fixtures are recorded
(scripts/record_engine_calls.py) on the commit whose behaviour is to be kept: the first rows on the commit before the
engine's term combiners, evaluation mode and graph key were given one shape each; the pseudo-time, validation, monitor
and viscosity rows and the headers on the commit before the options were given one base class."""
import functools
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import engine_call_rows as rows  # noqa: E402

_GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
with open(os.path.join(_GOLDEN_DIR, "engine_call_logs.json")) as _f:
    GOLDEN = json.load(_f)
with open(os.path.join(_GOLDEN_DIR, "engine_state_headers.json")) as _f:
    HEADERS = json.load(_f)
_BY_NAME = {r["name"]: r for r in rows.ROWS}
_PARAMS = dict(argnames="row", argvalues=rows.ROWS, ids=[r["name"] for r in rows.ROWS])


@functools.lru_cache(maxsize=None)
def _run(name):     # one run of a row serves both of its tests
    return rows.run(_BY_NAME[name])


def test_the_fixture_has_every_row():
    assert sorted(GOLDEN["rows"]) == sorted(r["name"] for r in rows.ROWS)
    assert sorted(HEADERS) == sorted(r["name"] for r in rows.ROWS)


@pytest.mark.parametrize(**_PARAMS)
def test_row_makes_the_recorded_calls(row):
    want = GOLDEN["rows"][row["name"]]
    log, keys, _ = _run(row["name"])
    want_log = [GOLDEN["entries"][i] for i in want["log"]]
    for k, (got, exp) in enumerate(zip(log, want_log)):
        assert got == exp, "call %d of %d" % (k, len(want_log))
    assert len(log) == len(want_log)
    assert keys == want["keys"]


@pytest.mark.parametrize(**_PARAMS)
def test_row_keeps_the_recorded_state_header(row):
    want, got = HEADERS[row["name"]], _run(row["name"])[2]
    for part in ("fingerprint", "info", "host"):
        assert got[part] == want[part], part
    for k, (seg, exp) in enumerate(zip(got["segments"], want["segments"])):
        assert seg == exp, "segment %d of %d" % (k, len(want["segments"]))
    assert len(got["segments"]) == len(want["segments"])
