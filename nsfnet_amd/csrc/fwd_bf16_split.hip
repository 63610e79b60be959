// Role-split bf16x3 forward sweep for residual mode (4 streams): two wave groups per workgroup in opposite phases.
//
// Same algorithm and results layout (S, field planes, loss partials) as fwd_bf16.hip - see there and fwd.hip for the
// reference lines replaced (NSFnet/net.py:52-54, NSFnet/pinn_solver.py:132-163,197-226,
// ev-NSFnet/pinn_solver.py:290-342,372-428).
//
// What the schedule rests on (tests/micro/mfma_valu_partner_pad.hip, MI355X round 2): on one SIMD, a wave issuing
// v_mfma_f32_32x32x16_bf16 back to back keeps its 32 cycles per MFMA while its PARTNER wave's VALU stream runs at
// 4.7 instructions per MFMA slot (78 % of its solo rate), and the partner's LDS / vector-memory instructions issue on
// ports the MFMA wave does not use.  One wave alone cannot do that for itself (every instruction of a wave issues in
// order: fwd_bf16_pipe.hip, one wave per SIMD, is issue-bound at ~45 cycles per MFMA).  What the schedule does NOT
// escape: the CU's one in-order vector-memory path - the M group's weight-fragment loads queue behind
// the E group's S stores, which drain at the HBM rate, so the M quarters run 1.2-1.4x their solo time.
//
// So: 512 threads = two groups of four waves; waves w and w + 4 are SIMD partners.  Group 0 owns tile A, group 1 tile
// B (32 points x 4 streams each); within a group wave w owns 64 features.  The groups run the SAME program one phase
// apart:          group 0:  E0(A)  M1(A)  E1(A)  M2(A) ...  M_{L-1}(A)  E_{L-1}(A) | E0(A') ...
//                 group 1:         E0(B)  M1(B)  E1(B) ...              M_{L-1}(B)  E_{L-1}(B) | ...
// M_l = hidden GEMM l (MFMA only: W fragments from L2 through a register ring, B fragments from the LDS image),
// E_l = tanh chain rule of layer l, bf16 hi/lo split, S spill (VALU / LDS / VMEM only).  In every phase but one per
// tile pair a SIMD has one wave in M and its partner in E.  A wave keeps ONE tile's accumulators (128 registers): no
// per-wave tile duplication, no hand interleave of two instruction streams - the hardware overlaps the partners.
//
// LDS: one tile's hi/lo image is 128 KB at HP = 256, two do not fit.  The groups SHARE one image, split along K into
// four 64-feature regions R0..R3; a phase is four quarters with a workgroup barrier after each.  The M group reads
// region q in quarter q.  A wave owns 16 features of every region (rows 0-15 / 16-31 of its two 32-row MFMA blocks map
// to regions 2fb / 2fb+1), so the E group computes its region-q quads in quarter q, parks them in 32 registers, and
// writes them into the image in quarter q + 1, when the M group has finished with that region (region 3: in quarter 0
// of the wave's own following M phase).  The output layer is folded into the last epilogue.
#include "kernels.h"
#include "point_stage.h"
#include "split_phases.h"

template <int HP>
struct SplitLds {
  using XI = XImg<HP, 32>;
  static constexpr size_t X_BYTES = XI::BYTES;                         // THE tile image (shared by the two groups)
  static constexpr size_t PART_F = (size_t)2 * 4 * 12 * 32;            // [group][wave][3 outputs x 4 streams][32 points]
  static constexpr size_t OUTV_F = (size_t)2 * 3 * 128;                // [group][3][128]
  static size_t bytes(int L) { return X_BYTES + (PART_F + OUTV_F + (size_t)L * HP + 6 * HP) * sizeof(float); }
};

// FF: the frozen sine first layer (split_phases.h): E0 forms the a-streams by layer0_sine; nothing else differs
template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
__global__ __launch_bounds__(2 * HP, 1) void fwd_split_kernel(FwdArgs a) {
  resolve_viscosity(a);     // viscosity identification: *nu_dev in place of the launch constant (kernels.h)
  using G = SplitLds<HP>;
  using SW = SplitWave<HP, TERMS, FF>;
  constexpr int GT = HP, PPL = SW::PPL, COLS = SW::COLS;      // GT: threads per group
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  float* const part = reinterpret_cast<float*>(ldsb + G::X_BYTES);
  float* const outv = part + G::PART_F;
  float* const biasL = outv + G::OUTV_F;                  // [L][HP], row 0 = zeros
  float* const woutL = biasL + (size_t)a.L * HP;          // [3][HP]
  float* const w0L = woutL + 3 * HP;                      // [w0x | w0y | b0][HP]
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, w = wave & 3;
  const int gtid = tid - grp * GT;                        // thread index inside the group
  const float* __restrict__ P = a.prep;
  const int L = a.L;
  const int npad = a.ntiles * PPL;
  float* const partG = part + (size_t)grp * 4 * 12 * 32;
  float* const outvG = outv + (size_t)grp * 3 * 128;
  float lsum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < L * HP; i += 2 * GT) biasL[i] = i < HP ? 0.f : P[prep_b(HP, i / HP) + (i % HP)];
  for (int i = tid; i < 3 * HP; i += 2 * GT) { woutL[i] = P[prep_wout(HP, L) + i]; w0L[i] = P[prep_w0x(HP) + i]; }
  __syncthreads();
  SW sw(ldsb, P, woutL, w0L, w, lane0);

  // the point stage of the group's previous tile rides in quarters 0 / 1 of E_0: output-layer bias + cross-wave sum,
  // then residuals / loss
  auto pstage = [&](int q, int ptile) {
    if (ptile >= 0 && q == 0) {
      for (int idx = gtid; idx < 3 * COLS; idx += GT) {
        const int c3 = idx / COLS, cc = idx % COLS;
        float s = cc < PPL ? P[prep_bout(HP, L) + c3] : 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) s += partG[(ww * 12 + c3 * 4 + cc / PPL) * 32 + (cc % PPL)];
        outvG[c3 * COLS + cc] = s;
      }
    }
    if (ptile >= 0 && ptile < a.ntiles && q == 1) residual_point_stage<PPL, COLS, HBC, PT>(a, outvG, ptile, gtid, npad, lsum);
  };
  auto bias = [&](int l) {      // bias rows from LDS
    return [=](int, int, int o, int) { return *reinterpret_cast<const f32x4*>(biasL + (size_t)l * HP + o); };
  };
  auto S_of = [&](int tile, int l) { return a.S + spill_off<act_block(HP, COLS)>(a.spill, tile, l, L); };
  auto none = [](auto&&...) {};      // no kernel work in this hook

  // Program of a group, one op per phase: per tile E0 M1 E1 ... M_{L-1} E_{L-1} (2L - 1 phases, four barriers each);
  // group 1 runs it one phase behind group 0 (an idle phase in front, group 0 idles one phase at the end), then one
  // drain phase for the last tile's point stage.  Tile of pair i: 2 i + grp.
  const int npairs = (a.ntiles + 1) / 2;
  if (grp == 1) SW::idle();
  int prev_tile = -1;
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int tile = 2 * pair + grp;
    sw.template fphase<0, false>(0, tile, nullptr, a.x, a.y, a.n, partG, bias(0), [&](int q) { pstage(q, prev_tile); });
    for (int l = 1; l < L - 1; ++l) {
      sw.template mphase<false, false>(l, nullptr);
      sw.template fphase<1, false>(l, tile, S_of(tile, l), a.x, a.y, a.n, partG, bias(l), none);
    }
    sw.template mphase<false, false>(L - 1, nullptr);
    sw.template fphase<2, false>(L - 1, tile, S_of(tile, L - 1), a.x, a.y, a.n, partG, bias(L - 1), none);
    prev_tile = tile;
  }
  for (int q = 0; q < 4; ++q) {                       // drain: point stage of the last tile
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

size_t fwd_split_lds_bytes(int HP, int L) { (void)HP; return SplitLds<256>::bytes(L); }

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
static int launch_one(const FwdArgs& a, int grid, hipStream_t s) {
  const size_t lds = SplitLds<HP>::bytes(a.L);
  if (a.S && !spill_is(a.spill, act_block(HP), IN_P24_COMPACT)) return -1000;
  return launch_or_configure(&fwd_split_kernel<HP, TERMS, HBC, PT, FF>, dim3(grid), dim3(2 * HP), lds, s, a.configure, a);
}

// residual mode, saved activations, L >= 2 hidden layers, HP = 256 (the caller checks)
int launch_fwd_split(int HP, int terms, const FwdArgs& a, int grid, hipStream_t s) {
  return dispatch_width<256>(HP, DISPATCH_UNSUPPORTED, [&](auto hp) {
    return dispatch_ns_terms(4, terms, [&](auto, auto t) {
      return dispatch_variant<VARIANTS_SPLIT>(a.hbc.kind, a.ptime, a.ff, [&](auto v) {
        using V = decltype(v);
        return launch_one<decltype(hp)::value, decltype(t)::value, V::hbc, V::pt, V::ff>(a, grid, s);
      });
    });
  });
}
