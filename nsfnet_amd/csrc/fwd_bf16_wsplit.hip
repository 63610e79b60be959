// Role-split bf16x3 forward sweep for WIDE nets (256 < hidden <= 448, e.g. BASELINE config 5's 8x400), residual mode:
// the schedule of fwd_bf16_split.hip (two wave groups per workgroup in opposite phases, SIMD partners overlap one
// group's MFMAs with the other's VALU / LDS / memory instructions) at the tile geometry of fwd_bf16_wide.hip (64 columns =
// 16 points x 4 streams, S in the 24-bit three-plane format, layer 0 spilled: dw_bf16_wide.hip and bwd_bf16_wsplit.hip
// read exactly what fwd_bf16_wide.hip would have written).  Reference lines replaced: NSFnet/net.py:52-54,
// NSFnet/pinn_solver.py:132-163,197-226, ev-NSFnet/pinn_solver.py:290-342,372-428 (see fwd.hip).
//
// Geometry.  NB = HP / 32 feature blocks.  A group is four waves; wave w owns the blocks 4 q + w (q = 0 .. MQ - 1, those
// that exist), so the accumulators are acc[MQ][2 column blocks] - 128 registers at MQ = 4, as in the hidden-256 kernel.
// The ONE shared image (bf16 hi/lo, [stream][point][k], 512-element rows) is split along K into MQ regions of four
// blocks (128 features): a phase is MQ quarters with a workgroup barrier after each; the M group reads region q in
// quarter q while the E group computes its block q (one per wave), parks the result in 32 registers and writes it into
// region q in quarter q + 1, when the M group has finished with that region.
// The LAST region needs no parking: the image rows have 512 - HP spare elements behind the features, enough for a
// second copy of that (short) region, and each group keeps its own copy - a group's E phase writes its last block
// straight into its copy while the other group's M phase reads the other one.  (The hidden-256 kernel parks it through
// the first quarter of the following M phase; here those 32 registers are the second half of the weight ring: four
// feature blocks per wave need 64 registers of weight fragments for two k-steps.)  Being private, that copy can be
// written at ANY time of the E phase: the last block's two quads are computed in quarters 0 and 1 (three quads per
// quarter there), and the last quarter - in which the M group has only the short last region to multiply - carries
// nothing but the dump of block MQ - 2.  (Measured neutral at 8x400: the wide sweeps wait on their weight stream.)
//
// A 64-column accumulator block holds two streams (lanes 0-15 / 16-31): v_permlane16_swap brings the four streams
// of a point into one lane (fwd_bf16_wide.hip), so lane (pp, hi, h) of a wave ends up with the eight features
// 32 b + 8 (gq + 2 hi) + 4 h + e (gq = 0, 1; e = 0..3) of point pp: two register quads per quarter, as in the hidden-256
// kernel.
#include "kernels.h"
#include "point_stage.h"
#include "wsplit_phases.h"

// FF: the frozen sine first layer (wsplit_phases.h): E0 forms the a-streams by layer0_sine and stores them in layer 0's
// slot; nothing else differs
template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
__global__ __launch_bounds__(512, 1) void fwd_wsplit_kernel(FwdArgs a) {
  resolve_viscosity(a);     // viscosity identification: *nu_dev in place of the launch constant (kernels.h)
  using SW = WSplitWave<HP, TERMS, FF>;
  constexpr int GT = 256, MQ = SW::MQ, PPL = SW::PPL, COLS = SW::COLS;
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  float* const part = reinterpret_cast<float*>(ldsb + SW::XI::BYTES);
  float* const outv = part + SW::PART_F;
  float* const woutL = outv + SW::OUTV_F;                 // [3][HP]
  float* const w0L = woutL + 3 * HP;                      // [w0x | w0y | b0][HP]
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, w = wave & 3;
  const int gtid = tid - grp * GT;
  const float* __restrict__ P = a.prep;
  const int L = a.L;
  const int npad = a.ntiles * PPL;
  float* const partG = part + (size_t)grp * 4 * 12 * 16;
  float* const outvG = outv + (size_t)grp * 3 * 64;
  float lsum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < 3 * HP; i += 2 * GT) { woutL[i] = P[prep_wout(HP, L) + i]; w0L[i] = P[prep_w0x(HP) + i]; }
  __syncthreads();
  SW sw(ldsb, P, woutL, w0L, grp, w, lane0);

  // the point stage of the group's previous tile rides in quarters 0 / 1 of E_0: output-layer bias + cross-wave sum,
  // then residuals / loss
  auto pstage = [&](int q, int ptile) {
    if (ptile >= 0 && q == 0) {
      for (int idx = gtid; idx < 3 * COLS; idx += GT) {
        const int c3 = idx / COLS, cc = idx % COLS;
        float s = cc < PPL ? P[prep_bout(HP, L) + c3] : 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) s += partG[(ww * 12 + c3 * 4 + cc / PPL) * 16 + (cc % PPL)];
        outvG[c3 * COLS + cc] = s;
      }
    }
    if (ptile >= 0 && ptile < a.ntiles && q == 1) residual_point_stage<PPL, COLS, HBC, PT>(a, outvG, ptile, gtid, npad, lsum);
  };
  auto S_of = [&](int tile, int l) { return a.S + spill_off<act_block(HP, COLS), 0>(a.spill, tile, l, L); };
  auto none = [](auto&&...) {};      // no kernel work in this hook

  // Program of a group: per tile E0 M1 E1 ... M_{L-1} E_{L-1}; group 1 runs it one phase behind group 0
  // (fwd_bf16_split.hip).  Tile of pair i: 2 i + grp.
  const int npairs = (a.ntiles + 1) / 2;
  if (grp == 1) SW::idle();
  int prev_tile = -1;
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int tile = 2 * pair + grp;
    sw.template fphase<0>(0, tile, S_of(tile, 0), a.x, a.y, a.n, partG, [&](int q) { pstage(q, prev_tile); });
    for (int l = 1; l < L - 1; ++l) {
      sw.template mphase<false, false>(l, nullptr);
      sw.template fphase<1>(l, tile, S_of(tile, l), a.x, a.y, a.n, partG, none);
    }
    sw.template mphase<false, false>(L - 1, nullptr);
    sw.template fphase<2>(L - 1, tile, S_of(tile, L - 1), a.x, a.y, a.n, partG, none);
    prev_tile = tile;
  }
  for (int q = 0; q < MQ; ++q) {                      // drain: point stage of the last tile
    pstage(q, prev_tile);
    __syncthreads();
  }
  if (grp == 0) SW::idle();
  float* red = reinterpret_cast<float*>(ldsb);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k * 2 * GT + tid] = lsum[k];
  __syncthreads();
  if (tid < 4) {
    float s = 0.f;
    for (int t = 0; t < 2 * GT; ++t) s += red[tid * 2 * GT + t];
    a.partials[blockIdx.x * PINN_NLOSS + tid] = s;
  } else if (tid < PINN_NLOSS) {
    a.partials[blockIdx.x * PINN_NLOSS + tid] = 0.f;
  }
}

size_t fwd_wsplit_lds_bytes(int HP) {
  return dispatch_width<WSPLIT_WIDTHS>(HP, (size_t)1 << 30, [](auto hp) { return WSplitWave<decltype(hp)::value, 3>::fwd_bytes(); });
}

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
static int launch_one(const FwdArgs& a, int grid, hipStream_t s) {
  const size_t lds = WSplitWave<HP, TERMS>::fwd_bytes();
  if (a.S && !spill_is(a.spill, act_block(HP, 64), IN_P24_WIDE)) return -1000;
  return launch_or_configure(&fwd_wsplit_kernel<HP, TERMS, HBC, PT, FF>, dim3(grid), dim3(512), lds, s, a.configure, a);
}

// residual mode, saved activations in the 24-bit format, L >= 2 hidden layers (the caller checks)
int launch_fwd_wsplit(int HP, int terms, const FwdArgs& a, int grid, hipStream_t s) {
  return dispatch_width<WSPLIT_WIDTHS>(HP, DISPATCH_UNSUPPORTED, [&](auto hp) {
    return dispatch_ns_terms(4, terms, [&](auto, auto t) {
      return dispatch_variant<VARIANTS_SPLIT>(a.hbc.kind, a.ptime, a.ff, [&](auto v) {
        using V = decltype(v);
        return launch_one<decltype(hp)::value, decltype(t)::value, V::hbc, V::pt, V::ff>(a, grid, s);
      });
    });
  });
}
