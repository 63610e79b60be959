// The S / Z-bar spill: how a plan's forward sweep, reverse sweep and dW kernel exchange the saved activations S and
// the z-adjoints Z-bar through HBM.  One descriptor (Spill) states the format; resolve_plan picks it, every argument
// block carries a copy, and every block address goes through spill_off.  Host and device; no HIP include.
//
// A (tile, layer) block holds the register quads of HP features x one tile's columns as 16-byte planes
// [plane][feature / 4][column in plane][feature % 4] (layout.h): FOUR fp32 planes - (t, z_x, z_y, z_D) of S, the four
// z-adjoints of Z-bar; value mode: four 32-point groups - or the THREE planes of the 24-bit format (spill_io.h pack24).
// Both S and Z-bar of a plan have the same descriptor.  The four layouts, `ablk` = HP x the tile's columns:
//
//   kind               quad  blk       first  skip0  written by                      read by
//   SPILL_CLASSIC      f32   ablk      0      0      fwd, fwd_wide, fwd_bf16,        bwd, bwd_wide, bwd_bf16, bwd_bf16_wide,
//                                                    fwd_bf16_wide, fwd_bf16_pipe    bwd_bf16_pipe; dw, dw_wide, dw_bf16,
//                                                    (S); their reverse sweeps (Z)   dw_bf16_wide.  Every value-mode plan.
//   SPILL_SKIP0        f32   ablk      0      1      fwd, fwd_wide; bwd, bwd_wide    bwd, bwd_wide, dw, dw_wide: all four
//                                                    (layer 0's slot stays unused)   recompute layer 0 (layer0_saved)
//   SPILL_P24_WIDE     p24   ablk      0      0      fwd_bf16_wide, fwd_bf16_wsplit; bwd_bf16_wide, bwd_bf16_wsplit (which
//                                                    bwd_bf16_wide, bwd_bf16_wsplit  recomputes layer 0 all the same),
//                                                    (3 of the block's 4 planes)     dw_bf16_wide
//                                                    FF: fwd_bf16_wsplit alone       FF: dw_bf16_wide alone reads layer 0
//   SPILL_P24_COMPACT  p24   3/4 ablk  1      1      fwd_bf16_split, bwd_bf16_split, bwd_bf16_split, fwdbwd_bf16_split,
//                                                    fwdbwd_bf16_split               dw_bf16: all recompute layer 0
//                                                    (FF: the same three)            FF: dw_bf16 alone recomputes layer 0
//
// A plan over a net with the frozen sine first layer (kernels.h FwdArgs::ff; FF above) is by default SPILL_CLASSIC in every
// precision, on the 8-wave kernels, and what its layer-0 block of S holds is that layer's a-streams (a, a_x, a_y, a_D)
// themselves: dW's layer-1 workgroups take their A operand straight from it, and nothing recomputes a sine layer.
// With $PINN_FF_SPLIT=1 a plan whose two sweeps are both role-split takes the layout of its families as any plan does:
// SPILL_P24_COMPACT at hidden 256, where layer 0 has no slot and dW's layer-1 workgroups recompute the a-streams from
// the point (spill_io.h layer0_sine of layer0_z, as the forward's first epilogue does), or SPILL_P24_WIDE at hidden
// 288..448, where layer 0's slot holds the a-streams in the 24-bit format - the 8-wave convention carried over.  The
// layer is frozen, so the reverse sweep of such a plan ends at layer 1 and reads nothing of layer 0 in either layout.
// Z-bar of layer 0 is never stored in any layout (dW_0 is accumulated by the reverse sweep itself); with first == 0 its
// slot exists and stays unused.
#pragma once
#include "layout.h"

enum SpillQuad { SPILL_QUAD_F32 = 0, SPILL_QUAD_P24 = 1 };
enum SpillKind { SPILL_CLASSIC = 0, SPILL_SKIP0, SPILL_P24_WIDE, SPILL_P24_COMPACT, SPILL_KINDS };
// sets of kinds, as spill_is takes them
enum : unsigned { IN_CLASSIC = 1u << SPILL_CLASSIC, IN_SKIP0 = 1u << SPILL_SKIP0, IN_P24_WIDE = 1u << SPILL_P24_WIDE, IN_P24_COMPACT = 1u << SPILL_P24_COMPACT };

struct Spill {
  int quad;      // SpillQuad: four fp32 planes per register quad, or three 24-bit planes
  int first;     // the layer in a tile's first block: 0, or 1 where layer 0 has no slot
  int skip0;     // 1: layer 0 of S is not stored; its readers recompute it from the point
  size_t blk;    // floats per (tile, layer) block
};

PINN_HD Spill spill_make(int kind, size_t ablk) {
  switch (kind) {
    case SPILL_SKIP0: return Spill{SPILL_QUAD_F32, 0, 1, ablk};
    case SPILL_P24_WIDE: return Spill{SPILL_QUAD_P24, 0, 0, ablk};
    case SPILL_P24_COMPACT: return Spill{SPILL_QUAD_P24, 1, 1, ablk / 4 * 3};
    default: return Spill{SPILL_QUAD_F32, 0, 0, ablk};
  }
}
// is `s` one of the layouts in the set `kinds` (IN_* bits) at HP x columns = ablk?  What a launcher asks
// before it launches, and resolve_plan of every role it has resolved.
PINN_HD bool spill_is(const Spill& s, size_t ablk, unsigned kinds) {
  for (int k = 0; k < SPILL_KINDS; ++k) {
    const Spill m = spill_make(k, ablk);
    if ((kinds >> k & 1u) && s.quad == m.quad && s.first == m.first && s.skip0 == m.skip0 && s.blk == m.blk) return true;
  }
  return false;
}

// floats of S (and of Z-bar) per tile
PINN_HD size_t spill_tile_floats(const Spill& s, int L) { return (size_t)(L - s.first) * s.blk; }
// float offset of the block of (tile, layer l).  A layer below `first` has no block: its offset is the tile's first
// block, so that a pointer formed for it and never used still lies inside the buffer.  A kernel may pass what its
// launcher has checked as constants and keep its address arithmetic free of loads: BLK, the floats per block of the
// layouts with a slot per layer (always its HP x columns), and FIRST where it admits one value only.
template <size_t BLK = 0, int FIRST = -1>
PINN_HD size_t spill_off(const Spill& s, int tile, int l, int L) {
  const int first = FIRST >= 0 ? FIRST : s.first;
  return first ? ((size_t)tile * (L - first) + (l > first ? l - first : 0)) * s.blk
               : ((size_t)tile * L + l) * (BLK ? BLK : s.blk);
}
