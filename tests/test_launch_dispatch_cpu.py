"""The launchers' shared dispatch (nsfnet_amd/csrc/launch_dispatch.h) on the CPU: a small stand-alone host program over
the header prints what dispatch_variant hands its callback for every launcher mask and all 8 settings of (hbc, ptime,
ff), what dispatch_width answers for every listed width, its neighbours and 0, and dispatch_ns_terms' four modes.  The
header has no HIP include, so the program is plain C++ and runs under the address and undefined-behaviour sanitizers.
The expected tables are written out here from the rules, not computed from the header: the three flags name one of
five variants, ff with walls or pseudo-time is refused, a variant outside the mask is refused - and, by a static_assert
in the callback, not instantiated either."""
import itertools
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nsfnet_amd", "csrc")
UNSUPPORTED = -1000

# every mask a launcher dispatches on, as the (hbc, ptime, ff) triples it has kernels for
TANH, HBC, PT, HBC_PT, FF = (0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1)
MASKS = {
    "VARIANTS_WAVE8": {TANH, HBC, PT, HBC_PT, FF},            # 8-wave forward and family, residual mode
    "VARIANTS_WAVE8_FWD_VALUE": {TANH, HBC, FF},              # 8-wave forward, value mode
    "VARIANTS_WAVE8_BWD": {TANH, HBC, PT, HBC_PT},            # 8-wave reverse sweep, residual mode
    "VARIANTS_WAVE8_BWD_VALUE": {TANH},                       # 8-wave reverse sweep, value mode
    "VARIANTS_SPLIT": {TANH, HBC, PT, HBC_PT, FF},            # role-split, wide role-split, fused
    "VARIANTS_PIPE": {TANH},                                  # pipelined schedule
}
# every width list of the launch files
WIDTHS = {
    "wave8": (32, 64, 96, 128, 160, 192, 224, 256),
    "wave8_lds": (32, 64, 96, 128, 160, 192, 224),
    "cols64": (128, 256),
    "fp32_wide": (128, 256, 288, 320, 352, 384, 416, 448, 480, 512),
    "bf16_wide": (288, 320, 352, 384, 416, 448, 480, 512),
    "wsplit": (288, 320, 352, 384, 416, 448),
    "hidden256": (256,),
}
OTHER_BYTES = 1 << 30       # the size_t "does not fit" answer of the wide role-split LDS functions


def probes(ws):
    return sorted({0} | {w + d for w in ws for d in (-32, 0, 32)})


PROGRAM = r"""
#include <cstddef>
#include <initializer_list>
#include <cstdio>
#include "launch_dispatch.h"
template <unsigned MASK>
static void variants(const char* name) {
  for (int i = 0; i < 8; ++i) {
    const bool hbc = i & 1, pt = i & 2, ff = i & 4;
    const int r = dispatch_variant<MASK>(hbc, pt, ff, [](auto v) {
      using V = decltype(v);
      static_assert((MASK & V::bit) != 0, "a variant outside the mask was instantiated");
      return 100 + V::hbc + 2 * V::pt + 4 * V::ff;
    });
    printf("variant %%s %%d %%d %%d %%d\n", name, (int)hbc, (int)pt, (int)ff, r);
  }
}
template <int... W>
static void widths(const char* name, const int* probe, int n) {
  for (int i = 0; i < n; ++i) {
    const int r = dispatch_width<W...>(probe[i], DISPATCH_UNSUPPORTED, [](auto hp) { return (int)decltype(hp)::value; });
    const size_t b = dispatch_width<W...>(probe[i], (size_t)1 << 30, [](auto hp) { return (size_t)decltype(hp)::value * 4; });
    printf("width %%s %%d %%d %%zu\n", name, probe[i], r, b);
  }
}
int main() {
%(variants)s
%(widths)s
  for (int ns : {4, 1, 2})
    for (int terms : {3, 1, 2})
      printf("mode %%d %%d %%d\n", ns, terms, dispatch_ns_terms(ns, terms, [](auto n, auto t) { return 10 * decltype(n)::value + decltype(t)::value; }));
  return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("launch_dispatch")
    src, exe = os.path.join(d, "launch_dispatch.cc"), os.path.join(d, "launch_dispatch")
    variants = "\n".join('  variants<%s>("%s");' % (m, m) for m in MASKS)
    widths = "\n".join('  { const int p[] = {%s}; widths<%s>("%s", p, %d); }' %
                       (", ".join(map(str, probes(ws))), ", ".join(map(str, ws)), name, len(probes(ws)))
                       for name, ws in WIDTHS.items())
    with open(src, "w") as f:
        f.write(PROGRAM % dict(variants=variants, widths=widths))
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:      # a host compiler without the sanitizer runtimes still checks the tables
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return [ln.split() for ln in run.stdout.splitlines()]


def test_the_three_flags_name_one_of_five_variants_or_are_refused(lines):
    got = {(r[1], int(r[2]), int(r[3]), int(r[4])): int(r[5]) for r in lines if r[0] == "variant"}
    assert len(got) == 8 * len(MASKS)
    for mask, have in MASKS.items():
        legal = 0
        for hbc, pt, ff in itertools.product((0, 1), repeat=3):
            if ff and (hbc or pt):
                want = UNSUPPORTED                                  # the sine layer comes with neither
            elif (hbc, pt, ff) in have:
                want = 100 + hbc + 2 * pt + 4 * ff                  # the callback saw exactly Variant<hbc, pt, ff>
                legal += 1
            else:
                want = UNSUPPORTED                                  # outside the mask
            assert got[(mask, hbc, pt, ff)] == want, (mask, hbc, pt, ff)
        assert legal == len(have) <= 5
    # the pipelined launchers refuse every plan but the plain one: the one behaviour no plan reaches through the C ABI
    assert [k[1:] for k, v in got.items() if k[0] == "VARIANTS_PIPE" and v != UNSUPPORTED] == [TANH]


def test_a_width_dispatches_to_itself_and_any_other_to_the_fallback(lines):
    got = {(r[1], int(r[2])): (int(r[3]), int(r[4])) for r in lines if r[0] == "width"}
    assert len(got) == sum(len(probes(ws)) for ws in WIDTHS.values())
    for name, ws in WIDTHS.items():
        for hp in probes(ws):
            want = (hp, 4 * hp) if hp in ws else (UNSUPPORTED, OTHER_BYTES)
            assert got[(name, hp)] == want, (name, hp)
        assert got[(name, 0)] == (UNSUPPORTED, OTHER_BYTES)


def test_the_four_modes(lines):
    got = {(int(r[1]), int(r[2])): int(r[3]) for r in lines if r[0] == "mode"}
    # NS 4 is residual mode and anything else value mode; 3 terms is bf16x3 and anything else one product
    assert got == {(4, 3): 43, (4, 1): 41, (4, 2): 41, (1, 3): 13, (1, 1): 11, (1, 2): 11, (2, 3): 13, (2, 1): 11, (2, 2): 11}


def test_the_recorded_plans_still_resolve(golden_dir):
    """Through the C ABI, without a device: every plan of the census resolves or is refused as recorded, and none trips
    the resolver's own re-check of the variant table (-5).  tests/test_plan_census.py compares the full rows."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import plan_census
    from nsfnet_amd import build, _lib
    build.build()
    lib = _lib.load()
    with open(os.path.join(golden_dir, "plan_census.json")) as f:
        want = json.load(f)
    cases = plan_census.cases()
    assert len(want) == len(cases)
    for case, w in zip(cases, want):
        rc = plan_census.run_case(lib, case)[1]
        assert rc == w[1] and rc != -5, (w[0], rc)
