"""$PINN_FF_SPLIT=1 ("Role-split and fused sweeps"): a residual plan over a net with the frozen
sine first layer keeps the role-split (hidden 256), fused and wide role-split sweeps the other switches give a tanh net,
but only as a whole: where either sweep would land on the pipelined schedule or on an 8-wave kernel the plan is, byte
for byte, today's 8-wave plan with layer 0 stored.  Through the C ABI, without a device (plans are sized for 256 compute
units there), in the manner of tests/test_pseudo_time_split_cpu.py.  Unset or 0 the resolution is what
tests/test_fourier_cpu.py pins; no other plan looks at the switch."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import plan_census  # noqa: E402

SWITCH = "PINN_FF_SPLIT"
F32, X3 = 0, 1
SPLIT = ["fwd_split_kernel", "bwd_split_kernel", "dw_bf16_kernel"]
WSPLIT = ["fwd_wsplit_kernel", "bwd_wsplit_kernel", "dw_bf16_wide_kernel"]
EIGHT = ["fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"]
WIDE8 = ["fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel"]
FUSED, TWO, WIDE, PLAIN = ("fused role-split kernel", "role-split kernels, two launches", "wide role-split kernels",
                           "8-wave kernels")
OLD_LINE = "frozen sine first layer: 8-wave kernels, layer 0 stored"
# what a sine net's plan is by default: the tanh net's plan under these (tests/test_fourier_cpu.py)
CLASSIC = {"PINN_SCHED": "0", "PINN_FWD_SCHED": "0", "PINN_BWD_SCHED": "0", "PINN_WSPLIT": "0", "PINN_FUSE": "0", "PINN_S0_SKIP32": "0"}


@pytest.fixture(scope="module")
def lib():
    from nsfnet_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture
def switch(monkeypatch):
    """The switch on and every other one unset."""
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


def _case(H, L, n, env=(), prec=(X3, X3, X3), streams=4):
    assert SWITCH not in plan_census.SWITCHES and SWITCH not in dict(env)
    return (H, L, prec, streams, n, dict(env))


def _sine_row(lib, case):
    """plan_census.run_case's row for the case over a net with the frozen sine first layer."""
    H, L, prec, streams, n, env = case
    old = {k: os.environ.pop(k, None) for k in plan_census.SWITCHES}
    os.environ.update(env)
    net, plan = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        assert lib.pinn_net_create(3, L, H, ctypes.byref(net)) == 0, lib.pinn_last_error()
        assert lib.pinn_net_set_precision(net, *prec) == 0, lib.pinn_last_error()
        assert lib.pinn_net_set_first_layer(net, 1) == 0, lib.pinn_last_error()
        rc = lib.pinn_plan_create(net, n, streams, ctypes.byref(plan))
        if rc != 0:
            return [plan_census.key(case), rc, lib.pinn_last_error().decode()]
        row = [plan_census.key(case), 0, lib.pinn_plan_padded_points(plan), lib.pinn_plan_workspace_bytes(plan, 0),
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


def _path(lib, case, capfd):
    """The sine net's row of the case, and the path its PINN_VERBOSE line names (None: the line of the switch off)."""
    capfd.readouterr()
    row = _sine_row(lib, case[:5] + (dict(case[5], PINN_VERBOSE="1"),))
    err = capfd.readouterr().err
    said = [line.split("frozen sine sweeps: ")[1] for line in err.splitlines() if "frozen sine sweeps: " in line]
    assert "pseudo-time sweeps" not in err and "constrained sweeps" not in err
    if os.environ.get(SWITCH, "0") == "0":
        assert not said and err.count(OLD_LINE) == 1, err
        return row, None
    assert len(said) == 1 and said[0].endswith("(%s=%s)" % (SWITCH, os.environ[SWITCH])) and OLD_LINE not in err, err
    return row, said[0].rsplit(" (", 1)[0]


@pytest.mark.parametrize("n", [360000, 69])
def test_headline_shape_keeps_the_fused_role_split_plan(lib, switch, capfd, n):
    """6x256 bf16x3: names, padded points and workspace bytes of the tanh net's default plan (the same compact layout,
    no slot for layer 0), and the plan is fused."""
    case = _case(256, 6, n)
    got, said = _path(lib, case, capfd)
    assert got[1] == 0 and got[5:8] == SPLIT, got
    tanh = plan_census.run_case(lib, case)
    assert tanh[5:8] == SPLIT and got[1:] == tanh[1:], (got, tanh)
    assert got[2] == -(-n // 32) * 32
    assert said == FUSED
    # and it is another plan than the one the switch leaves alone
    switch.delenv(SWITCH)
    off, _ = _path(lib, case, capfd)
    assert off[5:8] == EIGHT and off[4] > got[4]


@pytest.mark.parametrize("n", [360000, 69])
def test_fused_limits(lib, switch, capfd, n):
    case = _case(256, 6, n, {"PINN_FUSE": "0"})
    got, said = _path(lib, case, capfd)
    assert got[5:8] == SPLIT and said == TWO, (got, said)
    assert got[1:] == plan_census.run_case(lib, case)[1:]
    # eight hidden layers do not fit the fused kernel's LDS; seven do; two is the shortest sine net
    for L, path in ((8, TWO), (7, FUSED), (2, FUSED)):
        got, said = _path(lib, _case(256, L, n), capfd)
        assert got[5:8] == SPLIT and said == path, (L, got, said)
        assert got[1:] == plan_census.run_case(lib, _case(256, L, n))[1:]
    # mixed bf16 precisions of the two sweeps: the pair, not fused
    got, said = _path(lib, _case(256, 6, n, {}, (1, 2, 1)), capfd)
    assert got[5:8] == SPLIT and said == TWO, (got, said)


@pytest.mark.parametrize("H,L", [(400, 3), (330, 3), (400, 8), (288, 2), (448, 2)])
def test_wide_nets_keep_the_wide_role_split_sweeps(lib, switch, capfd, H, L):
    """The wide names and the tanh wide plan's bytes (SPILL_P24_WIDE: layer 0 has a slot, which holds the a-streams)."""
    for n in (360000, 69):
        case = _case(H, L, n)
        got, said = _path(lib, case, capfd)
        assert got[1] == 0 and got[5:8] == WSPLIT and said == WIDE, (got, said)
        assert got[1:] == plan_census.run_case(lib, case)[1:]
        assert got[2] == -(-n // 16) * 16


FALLBACKS = [
    (_case(256, 6, 360000, {"PINN_SCHED": "1"}), EIGHT),
    (_case(256, 6, 360000, {"PINN_FWD_SCHED": "2", "PINN_BWD_SCHED": "0"}), EIGHT),
    (_case(256, 6, 360000, {"PINN_FWD_SCHED": "0", "PINN_BWD_SCHED": "2"}), EIGHT),
    (_case(256, 6, 360000, {"PINN_FWD_SCHED": "1", "PINN_BWD_SCHED": "2"}), EIGHT),
    (_case(400, 3, 360000, {"PINN_WSPLIT": "0"}), WIDE8),
    (_case(256, 6, 360000, {}, (X3, X3, F32)), ["fwd_bf16_kernel", "bwd_bf16_kernel", "dw_kernel"]),
    (_case(480, 2, 360000), WIDE8),
    (_case(128, 4, 360000), EIGHT),
    (_case(256, 6, 2052, streams=1), EIGHT),
    (_case(400, 6, 2052, streams=1), WIDE8),
    (_case(256, 6, 360000, {}, (F32, F32, F32)), ["fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel"]),
    (_case(400, 3, 360000, {}, (F32, F32, F32)), ["fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel"]),
]
FALLBACK_IDS = ["sched1", "fwd2_bwd0", "fwd0_bwd2", "fwd1_bwd2", "wsplit0", "fp32_dw", "hidden480", "hidden128", "value_256",
                "value_400", "fp32", "fp32_wide"]


@pytest.mark.parametrize("case,names", FALLBACKS, ids=FALLBACK_IDS)
def test_what_is_not_a_whole_role_split_plan_is_todays_8_wave_plan_byte_for_byte(lib, switch, capfd, case, names):
    """No mixed layouts: the plan under the switch is the plan without it, which is the tanh net's SPILL_CLASSIC plan on
    the 8-wave kernels, and the line says so."""
    for n in (case[4], 69):
        c = case[:4] + (n, case[5])
        got, said = _path(lib, c, capfd)
        assert got[1] == 0 and got[5:8] == names and said == PLAIN, (got, said)
        assert not any("pipe" in k or "split" in k for k in got[5:8])
        switch.delenv(SWITCH)
        off, _ = _path(lib, c, capfd)
        switch.setenv(SWITCH, "1")
        assert got == off, (got, off)
        classic = plan_census.run_case(lib, c[:5] + (dict(c[5], **CLASSIC),))
        assert got[1:] == classic[1:], (got, classic)


def test_the_fallbacks_are_not_vacuous(lib, switch):
    """The tanh net's plan of the same switches does run the pipelined kernels, or a mixed pair."""
    for case, _ in FALLBACKS[:4] + FALLBACKS[5:6]:
        plain = plan_census.run_case(lib, case)
        assert any("pipe" in k for k in plain[5:8]), plain


@pytest.mark.parametrize("value", [None, "0"])
def test_unset_or_0_a_sine_net_resolves_as_before(lib, switch, capfd, value):
    _set(switch, SWITCH, value)
    for case, names in ((_case(256, 6, 360000), EIGHT), (_case(256, 6, 69, {"PINN_FUSE": "1", "PINN_SCHED": "2"}), EIGHT),
                        (_case(400, 3, 69), WIDE8), (_case(400, 3, 69, {"PINN_WSPLIT": "1"}), WIDE8)):
        got, said = _path(lib, case, capfd)
        assert got[5:8] == names and said is None, (got, said)
        assert got[1:] == plan_census.run_case(lib, case[:5] + (CLASSIC,))[1:]


def test_a_tanh_nets_plan_never_looks_at_the_switch(lib, switch):
    """Names, bytes and (through the bytes) every grid; rows of the census among them; constrained and pseudo-time plans
    under their own switches too."""
    from nsfnet_amd import _lib
    cases = [_case(256, 6, 360000), _case(256, 6, 69), _case(256, 6, 69, {"PINN_FUSE": "0"}), _case(400, 6, 360000),
             _case(256, 6, 360000, {"PINN_SCHED": "1"}), _case(256, 6, 360000, {}, (X3, X3, F32)), _case(50, 4, 69, {}, (F32,) * 3),
             _case(256, 6, 2052, streams=1), _case(400, 6, 2052, streams=1)]
    census = {plan_census.key(k) for k in plan_census.cases()}
    assert all(plan_census.key(c) in census for c in (cases[0], cases[3], cases[4], cases[7]))
    bc = _lib.HardBcStruct(1, 3, -1.0, -1.0, 0.5, 7.5)

    def special(create):
        out = []
        for H, n in ((256, 360000), (400, 69)):
            net, plan = ctypes.c_void_p(), ctypes.c_void_p()
            assert lib.pinn_net_create(3, 3, H, ctypes.byref(net)) == 0
            assert lib.pinn_net_set_precision(net, X3, X3, X3) == 0
            assert create(net, n, ctypes.byref(plan)) == 0, lib.pinn_last_error()
            out.append([lib.pinn_plan_padded_points(plan), lib.pinn_plan_workspace_bytes(plan, 0), lib.pinn_plan_workspace_bytes(plan, 1)] +
                       [lib.pinn_plan_kernel(plan, k) for k in (0, 1, 2)])
            lib.pinn_plan_destroy(plan); lib.pinn_net_destroy(net)
        return out

    def rows():
        out = [plan_census.run_case(lib, c) for c in cases]
        for theirs in (None, "1"):
            _set(switch, "PINN_HBC_SPLIT", theirs); _set(switch, "PINN_PTIME_SPLIT", theirs)
            out += special(lambda net, n, plan: lib.pinn_plan_create_constrained(net, n, 4, ctypes.byref(bc), plan))
            out += special(lambda net, n, plan: lib.pinn_plan_create_pseudo_time(net, n, None, plan))
        switch.delenv("PINN_HBC_SPLIT", raising=False); switch.delenv("PINN_PTIME_SPLIT", raising=False)
        return out

    on = rows()
    for value in (None, "0"):
        _set(switch, SWITCH, value)
        assert rows() == on
    assert on[0][5:8] == SPLIT and on[3][5:8] == WSPLIT and "fwd_pipe_kernel" in on[4][5:8] and on[7][5:8] == EIGHT
    k = len(cases)
    assert on[k][3:] == [s.encode() for s in EIGHT] and on[k + 4][3:] == [s.encode() for s in SPLIT]      # constrained: off, on


@pytest.mark.parametrize("ours", [None, "0", "1"])
def test_a_sine_nets_plan_never_looks_at_the_other_two_switches(lib, switch, capfd, ours):
    _set(switch, SWITCH, ours)
    cases = [_case(256, 6, 360000), _case(256, 6, 69, {"PINN_FUSE": "0"}), _case(400, 3, 69), _case(256, 6, 69, {"PINN_SCHED": "1"})]
    rows = {}
    for theirs in (None, "0", "1"):
        _set(switch, "PINN_HBC_SPLIT", theirs); _set(switch, "PINN_PTIME_SPLIT", theirs)
        rows[theirs] = [_path(lib, c, capfd) for c in cases]
    assert rows[None] == rows["0"] == rows["1"]
    want = ([SPLIT, SPLIT, WSPLIT, EIGHT], [FUSED, TWO, WIDE, PLAIN]) if ours == "1" else ([EIGHT, EIGHT, WIDE8, EIGHT], [None] * 4)
    assert [r[0][5:8] for r in rows["1"]] == want[0] and [r[1] for r in rows["1"]] == want[1]


def test_walls_and_pseudo_time_are_still_refused_by_name(lib, switch):
    from nsfnet_amd import _lib
    for H in (256, 400):
        net, h = ctypes.c_void_p(), ctypes.c_void_p()
        assert lib.pinn_net_create(3, 3, H, ctypes.byref(net)) == 0
        assert lib.pinn_net_set_precision(net, X3, X3, X3) == 0
        assert lib.pinn_net_set_first_layer(net, 1) == 0
        bc = _lib.HardBcStruct(1, 2, 0.0, 0.0, 1.0, 10.0)
        for theirs in (None, "1"):
            _set(switch, "PINN_HBC_SPLIT", theirs); _set(switch, "PINN_PTIME_SPLIT", theirs)
            assert lib.pinn_plan_create_constrained(net, 100, 4, ctypes.byref(bc), ctypes.byref(h)) != 0
            err = lib.pinn_last_error().decode()
            assert "frozen sine" in err and "hard-wall" in err, err
            assert lib.pinn_plan_create_pseudo_time(net, 100, None, ctypes.byref(h)) != 0
            err = lib.pinn_last_error().decode()
            assert "frozen sine" in err and "pseudo-time" in err, err
            assert lib.pinn_plan_create_pseudo_time(net, 100, ctypes.byref(bc), ctypes.byref(h)) != 0
            assert "frozen sine" in lib.pinn_last_error().decode()
        lib.pinn_net_destroy(net)


def test_engine_reports_the_switch_and_the_kernels(monkeypatch):
    """fourier_info()["split"] is the switch as read, ["kernels"] the collocation plan's names (None before one exists)."""
    import numpy as np
    import torch
    import fourier_fakes
    fourier_fakes.install(monkeypatch)
    from nsfnet_amd import engine as eng
    for value, want in ((None, 0), ("0", 0), ("1", 1)):
        _set(monkeypatch, SWITCH, value)
        e = eng.PinnEngine("cpu", 3, 16, 100.0, alpha_b=10.0)
        e.net.set_flat(torch.tensor(np.random.RandomState(1).randn(e.P) * 0.3, dtype=torch.float32))
        assert e.fourier_info() is None
        e.set_fourier_features(sigma=2.0, seed=7)
        i = e.fourier_info()
        assert i["kind"] == "sine" and i["split"] == want and i["kernels"] is None
