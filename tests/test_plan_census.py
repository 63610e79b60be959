"""pinn_plan_create resolves a plan (kernel family, grid and LDS per role, spill format, workspace layout) from the
net, the point and stream counts, the compute-unit count and the environment switches.  tests/golden/plan_census.json
records what the library answered for the fixed case list of scripts/plan_census.py before the resolution was gathered
into one step, on a host without a device (plans sized for 256 compute units): the build must reproduce every row
exactly.  On a device with another compute-unit count the grids, and with them the workspace bytes, differ by design;
the kernel names, the padded points and the refusals are then still compared."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import plan_census  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


def _compute_units():
    """What pinn_plan_create sizes for: the current device's compute units, 256 without a device."""
    import torch
    if not torch.cuda.is_available():
        return 256
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def test_case_list_covers_the_resolution():
    cases = plan_census.cases()
    keys = [plan_census.key(c) for c in cases]
    assert len(set(keys)) == len(keys)
    assert {c[0] for c in cases} >= {7, 40, 50, 128, 160, 256, 288, 400, 448, 480, 512}
    assert {c[1] for c in cases} >= {1, 2, 6, 7, 8, 12}
    assert {c[2] for c in cases if c[0] == 256} == set(plan_census.TRIPLES) and len(plan_census.TRIPLES) == 27
    assert {c[3] for c in cases} == {1, 4}
    assert {c[4] for c in cases} >= {1, 31, 2052, 360000, 4000000}
    envs = [c[5] for c in cases]
    for k in plan_census.SWITCHES:
        assert len({e[k] for e in envs if list(e) == [k]}) >= 2, k
    for want in ({"PINN_SCHED": "3"}, {"PINN_SCHED": "-1"}, {"PINN_WSPLIT": "0"}, {"PINN_FUSE": "0"},
                 {"PINN_S0_SKIP32": "0"}, {"PINN_TILE_COLS": "64"}, {"PINN_TILE_COLS": "128"},
                 {"PINN_FWD_SCHED": "2", "PINN_BWD_SCHED": "0"}, {"PINN_FWD_SCHED": "1", "PINN_BWD_SCHED": "2"}):
        assert want in envs, want


def test_build_reproduces_the_recorded_census(lib, golden_dir):
    with open(os.path.join(golden_dir, "plan_census.json")) as f:
        want = json.load(f)
    cases = plan_census.cases()
    assert len(want) == len(cases) >= 300
    refused = {w[0].split(" ")[0] for w in want if w[1] != 0}
    assert {"H256", "H512"} <= refused                      # a depth refused for LDS at hidden 256 and at 512
    full = _compute_units() == 256
    bad = []
    for case, w in zip(cases, want):
        got = plan_census.run_case(lib, case)
        if not full and w[1] == 0 and got[1] == 0:
            got, w = got[:3] + got[5:], w[:3] + w[5:]       # another device: names and padded points only
        if got != w:
            bad.append((w, got))
    assert not bad, "%d of %d rows differ, first: %r" % (len(bad), len(want), bad[:3])
