"""$PINN_HBC_SPLIT=1: a constrained plan keeps the role-split, wide role-split and fused sweeps
the other switches give it; a sweep that would resolve to the pipelined kernels, which have no constrained variant,
resolves to the 8-wave kernel.  Through the C ABI, without a device.  Unset or 0 the resolution is what
tests/test_hardbc_cpu.py and tests/test_hardbc_terms.py pin, and an unconstrained plan never looks at the switch."""
import ctypes
import os
import sys

import pytest

import hardbc_model as hm
from test_hardbc_terms import _constrained_census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import plan_census  # noqa: E402

SWITCH = "PINN_HBC_SPLIT"
X3, F32 = 1, 0
SPLIT = ["fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel"]
WSPLIT = ["fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel"]
EIGHT = ["fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"]
WIDE8 = ["fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel"]
BCS = [hm.HardBc(), hm.HardBc(lift_power=3, lid_sharpness=7.5, origin=(-1.0, -1.0), inv_len=0.5)]
# what the verbose line of a constrained plan says of its sweeps
FUSED, TWO, WIDE, PLAIN = ("fused role-split kernel", "role-split kernels, two launches", "wide role-split kernels",
                           "8-wave kernels")


@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture
def switch(monkeypatch):
    """The switch on and every other one unset: plan_census.run_case and _constrained_census set, and restore, the
    switches the census knows per case; this one is not among them, so it is set here and never through a case."""
    for k in list(os.environ):
        if k.startswith("PINN_"):
            monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(SWITCH, "1")
    return monkeypatch


def _case(H, L, n, env=(), prec=(X3, X3, X3)):
    assert SWITCH not in plan_census.SWITCHES and SWITCH not in dict(env)
    return (H, L, prec, 4, n, dict(env))


def _path(lib, case, bc, capfd):
    """The census row of the case created constrained, and the path its PINN_VERBOSE line names."""
    capfd.readouterr()
    row = _constrained_census(lib, case[:5] + (dict(case[5], PINN_VERBOSE="1"),), bc.struct())
    err = capfd.readouterr().err
    said = [line.split("constrained sweeps: ")[1] for line in err.splitlines() if "constrained sweeps: " in line]
    assert len(said) == 1 and said[0].endswith("(PINN_HBC_SPLIT=%s)" % os.environ.get(SWITCH, "0")), err
    return row, said[0].rsplit(" (", 1)[0]


def _round_trips(lib, case, bc):
    H, L, prec, streams, n, _ = case
    from nsfnet_amd import _lib
    net, plan, got = ctypes.c_void_p(), ctypes.c_void_p(), _lib.HardBcStruct()
    assert lib.pinn_net_create(3, L, H, ctypes.byref(net)) == 0
    assert lib.pinn_net_set_precision(net, *prec) == 0
    want = bc.struct()
    assert lib.pinn_plan_create_constrained(net, n, streams, ctypes.byref(want), ctypes.byref(plan)) == 0, lib.pinn_last_error()
    assert lib.pinn_plan_hard_bc(plan, ctypes.byref(got)) == 0
    assert [getattr(got, f) for f, _ in got._fields_] == [getattr(want, f) for f, _ in want._fields_] and got.kind == 1
    lib.pinn_plan_destroy(plan)
    lib.pinn_net_destroy(net)


@pytest.mark.parametrize("bc", BCS, ids=["unit", "mapped"])
@pytest.mark.parametrize("n", [360000, 69])
def test_headline_shape_keeps_the_fused_role_split_plan(lib, switch, capfd, n, bc):
    """6x256 bf16x3: the names, padded points and workspace bytes of the unconstrained default plan - hence its spill
    format and grids - the descriptor round-trips, and the plan is a fused one."""
    case = _case(256, 6, n)
    got, said = _path(lib, case, bc, capfd)
    assert got[1] == 0 and got[5:8] == SPLIT, got
    plain = plan_census.run_case(lib, case)
    assert plain[5:8] == SPLIT and got[1:] == plain[1:], (got, plain)
    assert got[2] == -(-n // 32) * 32
    assert said == FUSED
    _round_trips(lib, case, bc)


@pytest.mark.parametrize("n", [360000, 69])
def test_fuse_0_keeps_the_two_role_split_launches(lib, switch, capfd, n):
    case = _case(256, 6, n, {"PINN_FUSE": "0"})
    got, said = _path(lib, case, BCS[0], capfd)
    assert got[5:8] == SPLIT and said == TWO, (got, said)
    assert got[1:] == plan_census.run_case(lib, case)[1:]
    # eight hidden layers do not fit the fused kernel's LDS: the two launches, whatever PINN_FUSE says
    got, said = _path(lib, _case(256, 8, n), BCS[0], capfd)
    assert got[5:8] == SPLIT and said == TWO, (got, said)
    got, said = _path(lib, _case(256, 7, n), BCS[0], capfd)
    assert got[5:8] == SPLIT and said == FUSED, (got, said)


@pytest.mark.parametrize("H,L", [(400, 3), (330, 3), (400, 8)])
def test_wide_nets_keep_the_wide_role_split_sweeps(lib, switch, capfd, H, L):
    for n in (360000, 69):
        case = _case(H, L, n)
        got, said = _path(lib, case, BCS[0], capfd)
        assert got[1] == 0 and got[5:8] == WSPLIT and said == WIDE, (got, said)
        assert got[1:] == plan_census.run_case(lib, case)[1:]
        assert got[2] == -(-n // 16) * 16
    got, said = _path(lib, _case(H, L, 69, {"PINN_WSPLIT": "0"}), BCS[0], capfd)
    assert got[5:8] == WIDE8 and said == PLAIN, (got, said)


def test_hidden_480_keeps_the_8_wave_wide_kernels(lib, switch, capfd):
    """The wide role-split sweeps end at hidden 448."""
    case = _case(480, 2, 69)
    got, said = _path(lib, case, BCS[0], capfd)
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
    """Schedule 1 has no constrained variant: PINN_SCHED=1, an incomplete role-split pair and an fp32 dW resolve to
    schedule 0, and the plan is sized as the unconstrained plan on PINN_SCHED=0 is."""
    for n in (360000, 69):
        case = _case(256, 6, n, env, prec)
        got, said = _path(lib, case, BCS[0], capfd)
        assert got[1] == 0 and got[5:8] == names and said == PLAIN, (got, said)
        assert not any("pipe" in k for k in got[5:8])
        off = plan_census.run_case(lib, _case(256, 6, n, dict(env, PINN_SCHED="0", PINN_FWD_SCHED="0", PINN_BWD_SCHED="0"), prec))
        assert got[1:] == off[1:], (got, off)
    # the unconstrained plan of the same switches does run them: the rows above are not vacuous
    plain = plan_census.run_case(lib, _case(256, 6, 360000, env, prec))
    assert any("pipe" in k for k in plain[5:8]), plain


@pytest.mark.parametrize("value", [None, "0"])
def test_unset_or_0_a_constrained_plan_resolves_to_the_8_wave_families(lib, switch, capfd, value):
    if value is None:
        switch.delenv(SWITCH)
    else:
        switch.setenv(SWITCH, value)
    for case, names in ((_case(256, 6, 360000), EIGHT), (_case(400, 3, 69), WIDE8)):
        got, said = _path(lib, case, BCS[0], capfd)
        assert got[5:8] == names and said == PLAIN, (got, said)
        off = plan_census.run_case(lib, case[:5] + ({"PINN_SCHED": "0", "PINN_WSPLIT": "0", "PINN_FUSE": "0"},))
        assert got[1:] == off[1:]


def test_an_unconstrained_plan_never_looks_at_the_switch(lib, switch):
    cases = [_case(256, 6, 360000), _case(256, 6, 69), _case(256, 6, 69, {"PINN_FUSE": "0"}), _case(400, 3, 360000),
             _case(256, 6, 360000, {"PINN_SCHED": "1"}), _case(256, 6, 360000, {}, (X3, X3, F32)), _case(50, 4, 69, {}, (F32,) * 3),
             (256, 6, (X3, X3, X3), 1, 2052, {})]
    on = [plan_census.run_case(lib, c) for c in cases]
    # kind 0 and a null descriptor are the unconstrained plan, too
    from nsfnet_amd import _lib
    none = _constrained_census(lib, cases[0], _lib.HardBcStruct(0, 0, 0.0, 0.0, 0.0, 0.0))
    assert none[1:] == on[0][1:]
    for value in (None, "0"):
        if value is None:
            switch.delenv(SWITCH)
        else:
            switch.setenv(SWITCH, value)
        assert [plan_census.run_case(lib, c) for c in cases] == on
    assert on[0][5:8] == SPLIT and on[3][5:8] == WSPLIT and "fwd_pipe_kernel" in on[4][5:8]


def test_value_plans_of_a_constrained_net_stay_on_the_8_wave_kernels(lib, switch):
    for H, names in ((256, EIGHT), (400, WIDE8)):
        got = _constrained_census(lib, (H, 3, (X3, X3, X3), 1, 150, {}), BCS[0].struct())
        assert got[1] == 0 and got[5:8] == names, got


def test_fused_constrained_call_refuses_a_scale_that_does_not_undo_inv_len(lib, switch):
    from nsfnet_amd import _lib
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pinn_net_create(3, 6, 256, ctypes.byref(net)) == 0
    assert lib.pinn_net_set_precision(net, X3, X3, X3) == 0
    bc = _lib.HardBcStruct(1, 2, -1.0, -1.0, 0.5, 10.0)
    assert lib.pinn_plan_create_constrained(net, 640, 4, ctypes.byref(bc), ctypes.byref(plan)) == 0
    assert lib.pinn_plan_kernel(plan, 0) == b"fwd_split_kernel"
    one = ctypes.c_void_p(256)     # never dereferenced: the refusal comes before any launch
    coef = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 0.0)
    for scale in (1.0, 2.000003):
        rc = lib.pinn_residual_forward_backward(plan, one, one, one, one, None, None, None, None, one, coef, 100.0, 0.0, 0.0,
                                                scale, None, None, None)
        assert rc != 0 and "coord_scale" in lib.pinn_last_error().decode()
        assert "pinn_residual_forward_backward" in lib.pinn_last_error().decode()
    lib.pinn_plan_destroy(plan)
    lib.pinn_net_destroy(net)
