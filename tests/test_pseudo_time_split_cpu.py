"""$PINN_PTIME_SPLIT=1 ("Role-split and fused sweeps"): a pseudo-time plan, with or without
hard walls, keeps the role-split, wide role-split and fused sweeps the other switches give an unconstrained plan; a
sweep that would resolve to the pipelined kernels, which have no pseudo-time variant, resolves to the 8-wave kernel.
Through the C ABI, without a device, in the manner of tests/test_hardbc_split_cpu.py.  Unset or 0 the resolution is what
tests/test_pseudo_time_cpu.py pins; a pseudo-time plan never looks at PINN_HBC_SPLIT, and no other plan looks at
PINN_PTIME_SPLIT."""
import ctypes
import os

import pytest

import hardbc_model as hm
from test_hardbc_split_cpu import (EIGHT, F32, FUSED, PLAIN, SPLIT, TWO, WIDE, WIDE8, WSPLIT, X3, lib, plan_census)  # noqa: F401
from test_hardbc_terms import _constrained_census

SWITCH = "PINN_PTIME_SPLIT"
WALLS = [None, hm.HardBc(lift_power=3, lid_sharpness=7.5, origin=(-1.0, -1.0), inv_len=0.5)]
WALL_IDS = ["no_walls", "walls"]


class _PseudoTime:
    """The library with pinn_plan_create_constrained standing for pinn_plan_create_pseudo_time, so that
    test_hardbc_terms._constrained_census writes the census row of the case created as a pseudo-time plan."""

    def __init__(self, lib, walls):
        self._lib, self._walls = lib, walls

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def pinn_plan_create_constrained(self, net, n, streams, bc, plan):
        assert streams == 4
        return self._lib.pinn_plan_create_pseudo_time(net, n, bc if self._walls else None, plan)


@pytest.fixture
def switch(monkeypatch):
    """The switch on and every other one unset (plan_census.run_case and _constrained_census set, and restore, the
    switches the census knows per case; this one and PINN_HBC_SPLIT are not among them)."""
    for k in list(os.environ):
        if k.startswith("PINN_"):
            monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(SWITCH, "1")
    return monkeypatch


def _set(mp, name, value):
    if value is None:
        mp.delenv(name, raising=False)
    else:
        mp.setenv(name, value)


def _case(H, L, n, env=(), prec=(X3, X3, X3)):
    assert SWITCH not in plan_census.SWITCHES and "PINN_HBC_SPLIT" not in plan_census.SWITCHES
    assert SWITCH not in dict(env)
    return (H, L, prec, 4, n, dict(env))


def _path(lib, case, bc, capfd):
    """The census row of the case created as a pseudo-time plan (with the walls bc, or none), and the path its
    PINN_VERBOSE line names."""
    capfd.readouterr()
    row = _constrained_census(_PseudoTime(lib, bc is not None), case[:5] + (dict(case[5], PINN_VERBOSE="1"),),
                              (bc or hm.HardBc()).struct())
    err = capfd.readouterr().err
    said = [line.split("pseudo-time sweeps: ")[1] for line in err.splitlines() if "pseudo-time sweeps: " in line]
    assert len(said) == 1 and said[0].endswith("(%s=%s)" % (SWITCH, os.environ.get(SWITCH, "0"))), err
    assert ("constrained sweeps: " in err) == (bc is not None)
    return row, said[0].rsplit(" (", 1)[0]


@pytest.mark.parametrize("bc", WALLS, ids=WALL_IDS)
@pytest.mark.parametrize("n", [360000, 69])
def test_headline_shape_keeps_the_fused_role_split_plan(lib, switch, capfd, n, bc):
    """6x256 bf16x3: the names, padded points and workspace bytes of the plain default plan, and the plan is fused."""
    case = _case(256, 6, n)
    got, said = _path(lib, case, bc, capfd)
    assert got[1] == 0 and got[5:8] == SPLIT, got
    plain = plan_census.run_case(lib, case)
    assert plain[5:8] == SPLIT and got[1:] == plain[1:], (got, plain)
    assert got[2] == -(-n // 32) * 32
    assert said == FUSED


@pytest.mark.parametrize("bc", WALLS, ids=WALL_IDS)
@pytest.mark.parametrize("n", [360000, 69])
def test_fused_limits(lib, switch, capfd, n, bc):
    case = _case(256, 6, n, {"PINN_FUSE": "0"})
    got, said = _path(lib, case, bc, capfd)
    assert got[5:8] == SPLIT and said == TWO, (got, said)
    assert got[1:] == plan_census.run_case(lib, case)[1:]
    # eight hidden layers do not fit the fused kernel's LDS: the two launches, whatever PINN_FUSE says; seven do
    got, said = _path(lib, _case(256, 8, n), bc, capfd)
    assert got[5:8] == SPLIT and said == TWO, (got, said)
    assert got[1:] == plan_census.run_case(lib, _case(256, 8, n))[1:]
    got, said = _path(lib, _case(256, 7, n), bc, capfd)
    assert got[5:8] == SPLIT and said == FUSED, (got, said)


@pytest.mark.parametrize("bc", WALLS, ids=WALL_IDS)
@pytest.mark.parametrize("H,L", [(400, 3), (330, 3), (400, 8)])
def test_wide_nets_keep_the_wide_role_split_sweeps(lib, switch, capfd, H, L, bc):
    for n in (360000, 69):
        case = _case(H, L, n)
        got, said = _path(lib, case, bc, capfd)
        assert got[1] == 0 and got[5:8] == WSPLIT and said == WIDE, (got, said)
        assert got[1:] == plan_census.run_case(lib, case)[1:]
        assert got[2] == -(-n // 16) * 16
    case = _case(H, L, 69, {"PINN_WSPLIT": "0"})
    got, said = _path(lib, case, bc, capfd)
    assert got[5:8] == WIDE8 and said == PLAIN, (got, said)
    assert got[1:] == plan_census.run_case(lib, case)[1:]


def test_hidden_480_keeps_the_8_wave_wide_kernels(lib, switch, capfd):
    """The wide role-split sweeps end at hidden 448."""
    case = _case(480, 2, 69)
    got, said = _path(lib, case, None, capfd)
    assert got[5:8] == WIDE8 and said == PLAIN, (got, said)
    assert got[1:] == plan_census.run_case(lib, case)[1:]


@pytest.mark.parametrize("env,prec,names", [
    ({"PINN_SCHED": "1"}, (X3, X3, X3), EIGHT),
    ({"PINN_FWD_SCHED": "2", "PINN_BWD_SCHED": "0"}, (X3, X3, X3), EIGHT),
    ({"PINN_FWD_SCHED": "0", "PINN_BWD_SCHED": "2"}, (X3, X3, X3), EIGHT),
    ({"PINN_FWD_SCHED": "1", "PINN_BWD_SCHED": "2"}, (X3, X3, X3), EIGHT),
    ({}, (X3, X3, F32), ["fwd_bf16_kernel", "bwd_bf16_kernel", "dw_kernel"]),
    ({}, (F32, X3, X3), ["fwd_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"]),
], ids=["sched1", "fwd2_bwd0", "fwd0_bwd2", "fwd1_bwd2", "fp32_dw", "fp32_fwd"])
def test_what_would_run_the_pipelined_kernels_runs_the_8_wave_ones(lib, switch, capfd, env, prec, names):
    """Schedule 1 has no pseudo-time variant: PINN_SCHED=1, an incomplete role-split pair and an fp32 dW resolve to
    schedule 0, and the plan is sized as the plain plan on PINN_SCHED=0 is."""
    for bc in WALLS:
        for n in (360000, 69):
            case = _case(256, 6, n, env, prec)
            got, said = _path(lib, case, bc, capfd)
            assert got[1] == 0 and got[5:8] == names and said == PLAIN, (got, said)
            assert not any("pipe" in k for k in got[5:8])
            off = plan_census.run_case(lib, _case(256, 6, n, dict(env, PINN_SCHED="0", PINN_FWD_SCHED="0", PINN_BWD_SCHED="0"), prec))
            assert got[1:] == off[1:], (got, off)
    # the plain plan of the same switches does run them: the rows above are not vacuous
    plain = plan_census.run_case(lib, _case(256, 6, 360000, env, prec))
    assert any("pipe" in k for k in plain[5:8]), plain


@pytest.mark.parametrize("value", [None, "0"])
def test_unset_or_0_a_pseudo_time_plan_resolves_to_the_8_wave_families(lib, switch, capfd, value):
    _set(switch, SWITCH, value)
    for bc in WALLS:
        for case, names in ((_case(256, 6, 360000), EIGHT), (_case(256, 6, 69, {"PINN_FUSE": "1"}), EIGHT), (_case(400, 3, 69), WIDE8)):
            got, said = _path(lib, case, bc, capfd)
            assert got[5:8] == names and said == PLAIN, (got, said)
            off = plan_census.run_case(lib, case[:5] + ({"PINN_SCHED": "0", "PINN_WSPLIT": "0", "PINN_FUSE": "0"},))
            assert got[1:] == off[1:]


@pytest.mark.parametrize("ours", [None, "0", "1"])
def test_a_pseudo_time_plan_never_looks_at_the_hard_wall_switch(lib, switch, capfd, ours):
    _set(switch, SWITCH, ours)
    cases = [_case(256, 6, 360000), _case(256, 6, 69, {"PINN_FUSE": "0"}), _case(400, 3, 69), _case(256, 6, 69, {"PINN_SCHED": "1"})]
    for bc in WALLS:
        rows = {}
        for theirs in (None, "0", "1"):
            _set(switch, "PINN_HBC_SPLIT", theirs)
            rows[theirs] = [_path(lib, c, bc, capfd) for c in cases]
        assert rows[None] == rows["0"] == rows["1"]
        want = ([SPLIT, SPLIT, WSPLIT, EIGHT], [FUSED, TWO, WIDE, PLAIN]) if ours == "1" else (
            [EIGHT, EIGHT, WIDE8, EIGHT], [PLAIN] * 4)
        assert [r[0][5:8] for r in rows["1"]] == want[0] and [r[1] for r in rows["1"]] == want[1]


def test_no_other_plan_looks_at_the_switch(lib, switch):
    """A plain plan, a constrained plan (PINN_HBC_SPLIT at either value) and a value plan; rows of the census."""
    cases = [_case(256, 6, 360000), _case(256, 6, 69), _case(256, 6, 69, {"PINN_FUSE": "0"}), _case(400, 6, 360000),
             _case(256, 6, 360000, {"PINN_SCHED": "1"}), _case(256, 6, 360000, {}, (X3, X3, F32)), _case(50, 4, 69, {}, (F32,) * 3),
             (256, 6, (X3, X3, X3), 1, 2052, {}), (400, 6, (X3, X3, X3), 1, 2052, {})]
    census = plan_census.cases()
    assert all(plan_census.key(c) in {plan_census.key(k) for k in census} for c in (cases[0], cases[3], cases[4], cases[7]))
    walls = WALLS[1].struct()

    def rows():
        out = [plan_census.run_case(lib, c) for c in cases]
        for hbc in (None, "1"):
            _set(switch, "PINN_HBC_SPLIT", hbc)
            out += [_constrained_census(lib, c, walls) for c in cases]
        switch.delenv("PINN_HBC_SPLIT", raising=False)
        return out

    on = rows()
    for value in (None, "0"):
        _set(switch, SWITCH, value)
        assert rows() == on
    k = len(cases)
    assert on[0][5:8] == SPLIT and on[3][5:8] == WSPLIT and "fwd_pipe_kernel" in on[4][5:8] and on[7][5:8] == EIGHT
    assert on[k][5:8] == EIGHT and on[2 * k][5:8] == SPLIT and on[2 * k + 3][5:8] == WSPLIT        # constrained: off, on


def test_fused_call_with_unset_anchors_is_refused_before_any_launch(lib, switch):
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pinn_net_create(3, 6, 256, ctypes.byref(net)) == 0
    assert lib.pinn_net_set_precision(net, X3, X3, X3) == 0
    assert lib.pinn_plan_create_pseudo_time(net, 640, None, ctypes.byref(plan)) == 0, lib.pinn_last_error()
    assert lib.pinn_plan_kernel(plan, 0) == b"fwd_split_kernel"
    one = ctypes.c_void_p(256)     # never dereferenced: the refusal comes before any launch
    coef = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 0.0)
    rc = lib.pinn_residual_forward_backward(plan, one, one, one, one, None, None, None, None, one, coef, 100.0, 0.0, 0.0,
                                            1.0, None, None, None)
    err = lib.pinn_last_error().decode()
    assert rc != 0 and "anchors are unset" in err and "pinn_plan_set_pseudo_time" in err, err
    assert "pinn_residual_forward_backward" in err, err
    lib.pinn_plan_destroy(plan)
    lib.pinn_net_destroy(net)
