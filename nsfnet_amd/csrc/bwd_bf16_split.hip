// Role-split bf16x3 reverse sweep for residual mode (4 streams): the schedule of fwd_bf16_split.hip (two wave groups
// per workgroup in opposite phases; SIMD partners overlap one group's MFMAs with the other's VALU / LDS / memory
// instructions) applied to bwd_bf16.hip - see there and bwd.hip for the algorithm and the reference lines it replaces
// (loss.backward(), NSFnet/pinn_solver.py:252, ev-NSFnet/pinn_solver.py:469).  Results layout (Z-bar spill,
// per-workgroup skinny-gradient accumulators, ebar) is unchanged: the dW / reduce kernels do not care which reverse
// sweep ran.
//
//     group 0:  E_{L-1}(A)  G_{L-1}(A)  E_{L-2}(A)  ...  G_1(A)  E_0(A) | E_{L-1}(A') ...
//     group 1:              E_{L-1}(B)  G_{L-1}(B)  ...          G_1(B)   E_0(B) | ...
//
// E_l = tanh adjoint of layer l: reads the saved (t, z_x, z_y, z_D) quads (requested SQ quads ahead: they stream from
// HBM; layer 0's are recomputed from the point instead - the role-split forward does not spill them), turns the a-stream adjoints (accumulators of G_{l+1}; for l = L-1 the rank-3 update W_out^T o-bar) into z-bar,
// column-sums the skinny gradients into the LDS accumulator, splits z-bar into bf16 hi/lo, spills it.
// G_l = W_l^T z-bar_l (MFMA only).  One shared z-bar image, four K regions, 32 parked registers: fwd_bf16_split.hip.
//
// FF (the frozen sine first layer): layer 0 is not trained, so nothing of it is needed - not
// G_1 = W_1^T z-bar_1, not E_0 (its adjoint, dW_0, db_0).  The per-tile program ends at E_1:
//
//     group 0:  E_{L-1}(A)  G_{L-1}(A)  ...  G_2(A)  E_1(A) | E_{L-1}(A') ...
//     group 1:              E_{L-1}(B)  ...          G_2(B)   E_1(B) | ...
//
// Two phases fewer per tile, so the groups stay in opposite roles across the tile boundary.  What made the boundary
// safe before is that E_0 touches no image: it may meet the other group's image-writing E_{L-1} of the next tile.  The
// last E_1 takes exactly that place, so it must touch no image either: it runs with park = false (split_phases.h) -
// z-bar_1 goes to its spill block, which dW reads, and nowhere else.  It also carries E_0's hook, the next tile's
// output adjoints in quarter 3.  For L = 2 the one phase per tile is the seed phase E_1 itself, unparked.  The layer-0
// entries of the skinny-gradient accumulator (db_0, dW_0) stay at the zeros they are initialised with.
#include "kernels.h"
#include "point_stage.h"
#include "split_phases.h"

template <int HP>
struct SplitBwdLds {
  using XI = XImg<HP, 32>;
  static constexpr size_t X_BYTES = XI::BYTES;                          // THE z-bar image (shared by the two groups)
  static constexpr size_t OADJ_F = (size_t)2 * 4 * 128;                 // [group][4][128] (3 outputs used)
  static constexpr size_t DUMMY_F = 64 * 8;                             // sink of the lanes that own no accumulator slot
  static size_t bytes(int L) { return X_BYTES + (OADJ_F + DUMMY_F + 6 * HP + (size_t)sg_total(HP, L)) * sizeof(float); }
};

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
__global__ __launch_bounds__(2 * HP, 1) void bwd_split_kernel(BwdArgs a) {
  resolve_viscosity(a);     // viscosity identification: *nu_dev in place of the launch constant (kernels.h)
  using G = SplitBwdLds<HP>;
  using SW = SplitWave<HP, TERMS, FF>;
  constexpr int GT = HP, PPL = SW::PPL, COLS = SW::COLS;
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  float* const oadjL = reinterpret_cast<float*>(ldsb + G::X_BYTES);         // [2][4][128]
  float* const dummy = oadjL + G::OADJ_F;
  float* const woutL = dummy + G::DUMMY_F;                                   // [3][HP]
  float* const w0L = woutL + 3 * HP;                                         // [w0x | w0y | b0][HP]
  float* const sgacc = w0L + 3 * HP;                                         // [sg_total]
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, w = wave & 3;
  const int gtid = tid - grp * GT;
  const float* __restrict__ P = a.prep;
  const int L = a.L;
  const int npad = a.ntiles * PPL;
  const int SG = sg_total(HP, L);
  float* const oadjG = oadjL + (size_t)grp * 4 * 128;
  for (int i = tid; i < SG; i += 2 * GT) sgacc[i] = 0.f;
  for (int i = tid; i < 3 * HP; i += 2 * GT) { woutL[i] = P[prep_wout(HP, L) + i]; w0L[i] = P[prep_w0x(HP) + i]; }
  for (int i = tid; i < (int)G::DUMMY_F; i += 2 * GT) dummy[i] = 0.f;
  float dbo[3] = {0.f, 0.f, 0.f};
  SW sw(ldsb, P, woutL, w0L, w, lane0);

  // the dummy partner of an odd tile count reads tile 0's (finite) S
  auto S_of = [&](int tile, int l) { return a.S + spill_off<act_block(HP, COLS)>(a.spill, tile < a.ntiles ? tile : 0, l, L); };
  auto Z_of = [&](int tile, int l) { return a.Zb + spill_off<act_block(HP, COLS)>(a.spill, tile, l, L); };
  // ---- output adjoints of a tile (point_stage.h) into the group's LDS block; zero for the dummy partner tile ----
  auto seeds = [&](int tile, float& px, float& py) {
    const int col = lane0 & 31;
    if (tile < a.ntiles) {
      float pxa[1], pya[1];
      output_adjoint_stage<PPL, COLS, 4, GT, 1, HBC, PT>(a, tile, gtid, col, col, npad, oadjG, dbo, pxa, pya);
      px = pxa[0]; py = pya[0];
    } else {
      for (int i = gtid; i < 3 * COLS; i += GT) oadjG[i] = 0.f;
      px = py = 0.f;
    }
  };
  auto oadj = [&](int col, int, float (&oc)[3][4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) oc[c][s] = oadjG[c * COLS + s * PPL + col];
  };
  auto none = [](auto&&...) {};      // no kernel work in this hook

  // Straight-line program per group (fwd_bf16_split.hip): per tile E_{L-1} G_{L-1} E_{L-2} ... G_1 E_0, group 1 one
  // phase behind group 0.  Tile of pair i: 2 i + grp.  The next tile's output adjoints ride in quarter 3 of E_0.
  const int npairs = (a.ntiles + 1) / 2;
  float px = 0.f, py = 0.f, pxN = 0.f, pyN = 0.f;
  if ((int)blockIdx.x < npairs) seeds(2 * (int)blockIdx.x + grp, px, py);
  __syncthreads();
  if (grp == 1) SW::idle();
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int tile = 2 * pair + grp;
    const int next_tile = pair + (int)gridDim.x < npairs ? 2 * (pair + (int)gridDim.x) + grp : -1;
    if constexpr (FF) {      // the program that ends at E_1 (see the head of the file); L = 2: the seed phase is the last
      const bool more = L > 2;
      sw.template bphase<0, false>(L - 1, L, S_of(tile, L - 1), Z_of(tile, L - 1), px, py, sgacc, dummy + wave * 64, oadj,
                                   [&](int q) { if (!more && q == 3 && next_tile >= 0) seeds(next_tile, pxN, pyN); }, more);
      if (more) {
        for (int l = L - 1; l >= 3; --l) {
          sw.template mphase<true, true>(l, S_of(tile, l - 1));
          sw.template bphase<1, false>(l - 1, L, S_of(tile, l - 1), Z_of(tile, l - 1), px, py, sgacc, dummy + wave * 64, oadj, none);
        }
        sw.template mphase<true, true>(2, S_of(tile, 1));
        sw.template bphase<1, false>(1, L, S_of(tile, 1), Z_of(tile, 1), px, py, sgacc, dummy + wave * 64, oadj,
                                     [&](int q) { if (q == 3 && next_tile >= 0) seeds(next_tile, pxN, pyN); }, false);
      }
    } else {
      sw.template bphase<0, false>(L - 1, L, S_of(tile, L - 1), Z_of(tile, L - 1), px, py, sgacc, dummy + wave * 64, oadj, none);
      for (int l = L - 1; l >= 2; --l) {
        sw.template mphase<true, true>(l, S_of(tile, l - 1));
        sw.template bphase<1, false>(l - 1, L, S_of(tile, l - 1), Z_of(tile, l - 1), px, py, sgacc, dummy + wave * 64, oadj, none);
      }
      sw.template mphase<true, false>(1, nullptr);
      sw.template bphase<2, false>(0, L, S_of(tile, 0), Z_of(tile, 0), px, py, sgacc, dummy + wave * 64, oadj,
                                   [&](int q) { if (q == 3 && next_tile >= 0) seeds(next_tile, pxN, pyN); });
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

size_t bwd_split_lds_bytes(int HP, int L) { (void)HP; return SplitBwdLds<256>::bytes(L); }

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
static int launch_one(const BwdArgs& a, int grid, hipStream_t s) {
  const size_t lds = SplitBwdLds<HP>::bytes(a.L);
  if (!spill_is(a.spill, act_block(HP), IN_P24_COMPACT)) return -1000;
  return launch_or_configure(&bwd_split_kernel<HP, TERMS, HBC, PT, FF>, dim3(grid), dim3(2 * HP), lds, s, a.configure, a);
}

// residual mode, L >= 2 hidden layers, HP = 256 (the caller checks)
int launch_bwd_split(int HP, int terms, const BwdArgs& a, int grid, hipStream_t s) {
  if (a.ff && a.L < 2) return DISPATCH_UNSUPPORTED;      // (the FF sweep ends at layer 1)
  return dispatch_width<256>(HP, DISPATCH_UNSUPPORTED, [&](auto hp) {
    return dispatch_ns_terms(4, terms, [&](auto, auto t) {
      return dispatch_variant<VARIANTS_SPLIT>(a.hbc.kind, a.ptime, a.ff, [&](auto v) {
        using V = decltype(v);
        return launch_one<decltype(hp)::value, decltype(t)::value, V::hbc, V::pt, V::ff>(a, grid, s);
      });
    });
  });
}
