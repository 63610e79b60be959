// Role-split bf16x3 reverse sweep for WIDE nets (256 < hidden <= 448), residual mode: the schedule of bwd_bf16_split.hip
// at the tile geometry of bwd_bf16_wide.hip (64 columns = 16 points x 4 streams, S and Z-bar in the 24-bit three-plane
// format, classic [tile][L] blocks) - see fwd_bf16_wsplit.hip for the geometry (blocks 4 q + w per wave, MQ K regions,
// the last region's per-group copy) and bwd.hip for the algorithm and the reference lines it replaces
// (loss.backward(), NSFnet/pinn_solver.py:252, ev-NSFnet/pinn_solver.py:469).  Results layout (Z-bar, per-workgroup
// skinny-gradient accumulators, ebar) is that of bwd_bf16_wide.hip: dw_bf16_wide.hip / reduce do not care which reverse
// sweep ran.  Layer 0's saved activations are recomputed from the point (they are one FMA pair and one tanh), not read.
//
//     group 0:  E_{L-1}(A)  G_{L-1}(A)  E_{L-2}(A)  ...  G_1(A)  E_0(A) | E_{L-1}(A') ...
//     group 1:              E_{L-1}(B)  G_{L-1}(B)  ...          G_1(B)   E_0(B) | ...
//
// FF (the frozen sine first layer): the program ends at E_1, run with park = false, exactly as in
// bwd_bf16_split.hip - see there for why the two groups stay in opposite roles and why that phase must touch no image
// (here that includes the group's own copy of the last region: nothing reads it after E_1).  S of layer 0, which holds
// the a-streams in an FF plan, is not read by this kernel.
#include "kernels.h"
#include "point_stage.h"
#include "wsplit_phases.h"

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
__global__ __launch_bounds__(512, 1) void bwd_wsplit_kernel(BwdArgs a) {
  using SW = WSplitWave<HP, TERMS, FF>;
  constexpr int GT = 256, MQ = SW::MQ, PPL = SW::PPL, COLS = SW::COLS;
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  float* const oadjL = reinterpret_cast<float*>(ldsb + SW::XI::BYTES);       // [2][4][64]
  float* const dummy = oadjL + SW::OADJ_F;
  float* const sgacc = dummy + SW::DUMMY_F;                                  // [sg_total]
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, w = wave & 3;
  const int gtid = tid - grp * GT;
  const float* __restrict__ P = a.prep;
  const int L = a.L;
  const int npad = a.ntiles * PPL;
  const int SG = sg_total(HP, L);
  float* const oadjG = oadjL + (size_t)grp * 4 * 64;
  for (int i = tid; i < SG; i += 2 * GT) sgacc[i] = 0.f;
  for (int i = tid; i < (int)SW::DUMMY_F; i += 2 * GT) dummy[i] = 0.f;
  float dbo[3] = {0.f, 0.f, 0.f};
  // W_out and layer-0 rows from global memory: the LDS holds the image and the accumulators
  SW sw(ldsb, P, P + prep_wout(HP, L), P + prep_w0x(HP), grp, w, lane0);

  // the dummy partner of an odd tile count reads tile 0's (finite) S
  auto S_of = [&](int tile, int l) { return a.S + spill_off<act_block(HP, COLS), 0>(a.spill, tile < a.ntiles ? tile : 0, l, L); };
  auto Z_of = [&](int tile, int l) { return a.Zb + spill_off<act_block(HP, COLS), 0>(a.spill, tile, l, L); };
  // ---- output adjoints of a tile (point_stage.h) into the group's LDS block; zero for the dummy partner tile ----
  auto seeds = [&](int tile, float& px, float& py) {
    const int col = lane0 & 31;
    if (tile < a.ntiles) {
      float pxa[1], pya[1];
      output_adjoint_stage<PPL, COLS, 4, GT, 1, HBC, PT>(a, tile, gtid, col, col & 15, npad, oadjG, dbo, pxa, pya);
      px = pxa[0]; py = pya[0];
    } else {
      for (int i = gtid; i < 3 * COLS; i += GT) oadjG[i] = 0.f;
      px = py = 0.f;
    }
  };
  auto none = [](auto&&...) {};      // no kernel work in this hook

  // Straight-line program per group: per tile E_{L-1} G_{L-1} E_{L-2} ... G_1 E_0, group 1 one phase behind group 0.
  // Tile of pair i: 2 i + grp.  The next tile's output adjoints ride in the last quarter of E_0.
  resolve_viscosity(a);     // viscosity identification: *nu_dev in place of the launch constant (kernels.h)
  const int npairs = (a.ntiles + 1) / 2;
  float px = 0.f, py = 0.f, pxN = 0.f, pyN = 0.f;
  if ((int)blockIdx.x < npairs) seeds(2 * (int)blockIdx.x + grp, px, py);
  __syncthreads();
  if (grp == 1) SW::idle();
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int tile = 2 * pair + grp;
    const int next_tile = pair + (int)gridDim.x < npairs ? 2 * (pair + (int)gridDim.x) + grp : -1;
    auto hook = [&](int q) { if (q == MQ - 1 && next_tile >= 0) seeds(next_tile, pxN, pyN); };
    if constexpr (FF) {      // the program that ends at E_1 (see the head of the file)
      const bool more = L > 2;      // (L = 2: the first phase is the last)
      sw.template bphase<0>(L - 1, L, S_of(tile, L - 1), Z_of(tile, L - 1), px, py, oadjG, sgacc, dummy + wave * 64,
                            [&](int q) { if (!more) hook(q); }, more);
      if (more) {
        for (int l = L - 1; l >= 3; --l) {
          sw.template mphase<true, true>(l, S_of(tile, l - 1));
          sw.template bphase<1>(l - 1, L, S_of(tile, l - 1), Z_of(tile, l - 1), px, py, oadjG, sgacc, dummy + wave * 64, none);
        }
        sw.template mphase<true, true>(2, S_of(tile, 1));
        sw.template bphase<1>(1, L, S_of(tile, 1), Z_of(tile, 1), px, py, oadjG, sgacc, dummy + wave * 64, hook, false);
      }
    } else {
      sw.template bphase<0>(L - 1, L, S_of(tile, L - 1), Z_of(tile, L - 1), px, py, oadjG, sgacc, dummy + wave * 64, none);
      for (int l = L - 1; l >= 2; --l) {
        sw.template mphase<true, true>(l, S_of(tile, l - 1));
        sw.template bphase<1>(l - 1, L, S_of(tile, l - 1), Z_of(tile, l - 1), px, py, oadjG, sgacc, dummy + wave * 64, none);
      }
      sw.template mphase<true, false>(1, nullptr);
      sw.template bphase<2>(0, L, S_of(tile, 0), Z_of(tile, 0), px, py, oadjG, sgacc, dummy + wave * 64, hook);
    }
    px = pxN; py = pyN;
  }
  if (grp == 0) SW::idle();
  // ---------------- flush ----------------
  float* red = reinterpret_cast<float*>(ldsb);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) red[c * 2 * GT + tid] = dbo[c];
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int t = 0; t < 2 * GT; ++t) s += red[tid * 2 * GT + t];
    sgacc[sg_bout(HP, L) + tid] = s;
  }
  __syncthreads();
  float* out = a.sg + (size_t)blockIdx.x * SG;
  for (int i = tid; i < SG; i += 2 * GT) out[i] = sgacc[i];
}

size_t bwd_wsplit_lds_bytes(int HP, int L) {
  return dispatch_width<WSPLIT_WIDTHS>(HP, (size_t)1 << 30, [&](auto hp) { return WSplitWave<decltype(hp)::value, 3>::bwd_bytes(L); });
}

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
static int launch_one(const BwdArgs& a, int grid, hipStream_t s) {
  const size_t lds = WSplitWave<HP, TERMS>::bwd_bytes(a.L);
  if (!spill_is(a.spill, act_block(HP, 64), IN_P24_WIDE)) return -1000;
  return launch_or_configure(&bwd_wsplit_kernel<HP, TERMS, HBC, PT, FF>, dim3(grid), dim3(512), lds, s, a.configure, a);
}

// residual mode, 24-bit spill, L >= 2 hidden layers (the caller checks)
int launch_bwd_wsplit(int HP, int terms, const BwdArgs& a, int grid, hipStream_t s) {
  if (a.ff && a.L < 2) return DISPATCH_UNSUPPORTED;      // (the FF sweep ends at layer 1)
  return dispatch_width<WSPLIT_WIDTHS>(HP, DISPATCH_UNSUPPORTED, [&](auto hp) {
    return dispatch_ns_terms(4, terms, [&](auto, auto t) {
      return dispatch_variant<VARIANTS_SPLIT>(a.hbc.kind, a.ptime, a.ff, [&](auto v) {
        using V = decltype(v);
        return launch_one<decltype(hp)::value, decltype(t)::value, V::hbc, V::pt, V::ff>(a, grid, s);
      });
    });
  });
}
