"""The S / Z-bar spill descriptor (nsfnet_amd/csrc/spill.h) on the CPU: a small stand-alone host program over the header
prints, for each of the four layouts, the descriptor and the offset of every (tile, layer) block; the checks are here.
The header has no HIP include, so the program is plain C++ and runs under the address and undefined-behaviour
sanitizers.  The expected offsets are written out independently of the header: ((tile * L) + l) * blk for the layouts
with a slot per layer, (tile * (L - 1) + (l - 1)) * sblk for the compact one."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nsfnet_amd", "csrc")
KINDS = ("SPILL_CLASSIC", "SPILL_SKIP0", "SPILL_P24_WIDE", "SPILL_P24_COMPACT")
DEPTHS = (1, 2, 6)
TILES = (1, 3, 70)
GEOMETRIES = ((64, 128), (256, 128), (400, 64))      # (HP, columns) of real plans

PROGRAM = r"""
#include <cstdio>
#include "spill.h"
int main() {
  const int kinds[] = {SPILL_CLASSIC, SPILL_SKIP0, SPILL_P24_WIDE, SPILL_P24_COMPACT};
  const int depths[] = {%(depths)s}, tiles[] = {%(tiles)s}, geo[][2] = {%(geo)s};
  for (int kind : kinds)
    for (auto& g : geo)
      for (int L : depths)
        for (int nt : tiles) {
          const size_t ablk = act_block(g[0], g[1]);
          const Spill s = spill_make(kind, ablk);
          // the descriptor must be its own kind and no other
          for (int k = 0; k < SPILL_KINDS; ++k)
            if (spill_is(s, ablk, 1u << k) != (k == kind)) return 1;
          printf("%%d %%d %%d %%d %%d %%d %%d %%d %%zu %%zu", kind, g[0], g[1], L, nt, s.quad, s.first, s.skip0, s.blk, spill_tile_floats(s, L));
          for (int t = 0; t < nt; ++t)
            for (int l = s.first; l < L; ++l) printf(" %%zu", spill_off(s, t, l, L));
          printf("\n");
        }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("spill_layout")
    src, exe = os.path.join(d, "spill_layout.cc"), os.path.join(d, "spill_layout")
    with open(src, "w") as f:
        f.write(PROGRAM % dict(depths=", ".join(map(str, DEPTHS)), tiles=", ".join(map(str, TILES)),
                               geo=", ".join("{%d, %d}" % g for g in GEOMETRIES)))
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:      # a host compiler without the sanitizer runtimes still checks the arithmetic
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert len(out) == len(KINDS) * len(GEOMETRIES) * len(DEPTHS) * len(TILES)
    return out


def test_the_four_layouts_are_the_four_descriptor_values(rows):
    want = {0: (0, 0, 0, 4), 1: (0, 0, 1, 4), 2: (1, 0, 0, 4), 3: (1, 1, 1, 3)}      # quad, first, skip0, quarters of ablk
    for kind, HP, cols, L, nt, quad, first, skip0, blk, tile_floats, *offs in rows:
        q, f, s0, quarters = want[kind]
        assert (quad, first, skip0) == (q, f, s0), KINDS[kind]
        assert blk == HP * cols // 4 * quarters
        assert tile_floats == (L - first) * blk
        assert len(offs) == nt * (L - first)


def test_blocks_lie_inside_the_buffer_and_do_not_overlap(rows):
    for kind, HP, cols, L, nt, quad, first, skip0, blk, tile_floats, *offs in rows:
        for o in offs:
            assert 0 <= o and o + blk <= nt * tile_floats, (KINDS[kind], HP, L, nt, o)
        srt = sorted(offs)
        assert all(b - a >= blk for a, b in zip(srt, srt[1:])), (KINDS[kind], HP, L, nt)


def test_offsets_equal_the_formulas_written_out_here(rows):
    for kind, HP, cols, L, nt, quad, first, skip0, blk, tile_floats, *offs in rows:
        if KINDS[kind] == "SPILL_P24_COMPACT":
            sblk = HP * cols * 3 // 4
            want = [(tile * (L - 1) + (l - 1)) * sblk for tile in range(nt) for l in range(1, L)]
        else:
            want = [((tile * L) + l) * (HP * cols) for tile in range(nt) for l in range(L)]
        assert offs == want, (KINDS[kind], HP, cols, L, nt)
