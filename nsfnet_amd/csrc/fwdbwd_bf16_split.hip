// Role-split forward and reverse sweep of one tile in ONE kernel (residual mode, MSE seeds, hidden 256): the phases of
// split_phases.h, which fwd_bf16_split.hip and bwd_bf16_split.hip run as two launches (fwd_bf16_split.hip describes the
// schedule and the shared K-region image; the two kernels name the reference lines replaced), run back to back per
// tile, so the last hidden layer's saved activations S_{L-1} never leave the registers (KEEP in split_phases.h).
// S_{L-1} has one reader, the reverse sweep's first epilogue (dW_l needs a_{l-1}; the output-layer gradient
// is summed inside the reverse sweep), and the MSE seed 2 alpha_e c_k / N is known before the forward runs, so nothing
// global separates a tile's forward from its reverse sweep.
//
//     per tile and group:  E0 M1 E1 ... M_{L-1}  XA XB  G_{L-1} E'_{L-2} ... G_1 E'_0
//     XA = E_{L-1}: tanh chain rule, output layer into the per-wave partials, S_{L-1} kept as 24-bit quads (pack24)
//     XB = point stage (residuals, loss, field planes) + output adjoints + E'_{L-1} on the kept quads (unpack24)
// 4L - 2 phases per tile, as the two launches have together; group 1 runs one phase behind group 0, so XA of one
// group meets the other's M_{L-1} / XB, and XB (the only image writer of the two) meets the other's XA, which touches
// no image.  Every value, and every order of summation (loss partials, skinny gradients, dbo), is the one of
// fwd_split + bwd_split on the same plan: tile of pair i = 2 i + grp, the point stage's owner thread (lanes 0-31 of
// the group's wave 0) is the one both kernels use, and S_{L-1} passes through pack24 / unpack24 exactly as if it had
// been spilled and read back.
//
// LDS (hidden 256, L = 6: 161 808 of 163 840 bytes): the image, the output-layer partials, w_out / w0 rows (one copy
// for both sweeps) and the skinny-gradient accumulator.  What the split pair keeps besides does not fit and is not
// needed: the bias rows are read from the prepared buffer with scalar loads; the point stage of XB is computed by
// every lane of the group for its own column straight from the partials, so neither the forward's output block nor
// the reverse sweep's output-adjoint block exists; the commit sink of the lanes that own no accumulator slot is the
// unused fourth output row of the dW_out accumulator.
//
// Hard wall conditions (HBC): XB's point stage runs the output map and its transpose of point_stage.h
// on the lane's column, exactly where residual_point_stage / output_adjoint_stage run them in the two launches; the
// descriptor rides in the kernel arguments, so the LDS budget is the unconstrained one.
//
// Pseudo-time stepping (PT): every lane reads the three anchor values of its column from global memory
// (no LDS is left for them).  As the two launches do, XB builds the residuals q_k twice: for the loss sums from the
// registers of the forward, and for the seeds from opaque copies of the values the reverse sweep would read back from
// the planes.  The planes keep the steady residuals.
//
// FF (the frozen sine first layer): E0 forms the a-streams by layer0_sine, and the reverse half ends at
// E'_1 as in bwd_bf16_split.hip (see there): no G_1, no E'_0.
//
//     per tile and group:  E0 M1 E1 ... M_{L-1}  XA XB  G_{L-1} E'_{L-2} ... G_2 E'_1        (L = 2:  E0 M1 XA XB)
//
// 4L - 4 phases per tile, two fewer, so the groups keep their opposite roles.  The last phase meets the other group's
// image-reading G_2 (or, for L = 2, its XA, which touches no image) and is followed by the group's own E0 of the next
// tile while the partner runs ITS last phase: E'_0's place, which is safe because E'_0 touches no image.  So the last
// phase runs with park = false (split_phases.h): z-bar_1 goes to its spill block for dW and nowhere else.  Same bodies
// and orders of summation as the FF two launches: bit for bit their results.
#include "kernels.h"
#include "point_stage.h"
#include "split_phases.h"

template <int HP>
struct FusedLds {
  using XI = XImg<HP, 32>;
  static constexpr size_t X_BYTES = XI::BYTES;
  static constexpr size_t PART_F = (size_t)2 * 4 * 12 * 32;            // [group][wave][3 outputs x 4 streams][32 points]
  static size_t bytes(int L) { return X_BYTES + (PART_F + 6 * HP + (size_t)sg_total(HP, L)) * sizeof(float); }
};

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
__global__ __launch_bounds__(2 * HP, 1) void fwdbwd_split_kernel(FwdArgs fa, BwdArgs a) {
  resolve_viscosity(fa); resolve_viscosity(a);     // viscosity identification: *nu_dev in place of the launch constant (kernels.h)
  using G = FusedLds<HP>;
  using SW = SplitWave<HP, TERMS, FF>;
  constexpr int GT = HP, PPL = SW::PPL, COLS = SW::COLS;
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  float* const part = reinterpret_cast<float*>(ldsb + G::X_BYTES);
  float* const woutL = part + G::PART_F;                  // [3][HP]
  float* const w0L = woutL + 3 * HP;                      // [w0x | w0y | b0][HP]
  float* const sgacc = w0L + 3 * HP;                      // [sg_total]
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, w = wave & 3;
  const float* __restrict__ P = a.prep;
  const int L = a.L;
  const int npad = a.ntiles * PPL;
  const int SG = sg_total(HP, L);
  float* const partG = part + (size_t)grp * 4 * 12 * 32;
  float* const sink = sgacc + sg_wout(HP, L) + 3 * HP;    // (n_out = 3: row 3 of dW_out is never reduced)
  for (int i = tid; i < SG; i += 2 * GT) sgacc[i] = 0.f;
  for (int i = tid; i < 3 * HP; i += 2 * GT) { woutL[i] = P[prep_wout(HP, L) + i]; w0L[i] = P[prep_w0x(HP) + i]; }
  __syncthreads();
  float lsum[4] = {0.f, 0.f, 0.f, 0.f};
  float dbo[3] = {0.f, 0.f, 0.f};

  SW sw(ldsb, P, woutL, w0L, w, lane0);

  // ---- bias quad of layer l from the prepared buffer (uniform address: scalar loads, no wait on the spill stores) ----
  auto bias = [&](int l) {
    return [&, l](int fb, int g, int, int h) {
      typedef __attribute__((address_space(4))) const f32x4 cf32x4;
      const cf32x4* bp = (const cf32x4*)(uintptr_t)(P + prep_b(HP, l) + sw.qbase(fb, g));
      const f32x4 b0 = bp[0], b1 = bp[1];
      return h ? b1 : b0;
    };
  };
  // The dummy partner of an odd tile count reads its OWN S (the +1 scratch block its forward just wrote), not tile 0's as
  // bwd_bf16_split.hip does: here tile 0 may still be in its forward on another workgroup.  Its output adjoints are zero,
  // so its z-bars are zeros either way.
  auto S_of = [&](int tile, int l) { return a.S + spill_off<act_block(HP, COLS)>(a.spill, tile, l, L); };
  auto Sw_of = [&](int tile, int l) { return fa.S + spill_off<act_block(HP, COLS)>(a.spill, tile, l, L); };
  auto Z_of = [&](int tile, int l) { return a.Zb + spill_off<act_block(HP, COLS)>(a.spill, tile, l, L); };
  auto none = [](auto&&...) {};      // no kernel work in this hook

  // ---------------- point stage + output adjoints of column col (start of XB) ----------------
  // Every lane of the group computes its column's point (the output adjoints are needed by all of them); lanes 0-31 of
  // the group's wave 0 - the owner thread of the point in both split kernels - also write the fields, vis_t, vis_t_minus,
  // ebar and accumulate the loss and dbo partials.  Same expressions as point_stage.h, in the same order.
  auto point_stage = [&](int tile, int col, bool owner, float vtm_old, float (&oc)[3][4]) {
    const int pt = tile * PPL + col;
    const bool m = pt < a.n;
    float ov[3][4];
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float v = s == 0 ? P[prep_bout(HP, L) + c3] : 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) v += partG[(ww * 12 + c3 * 4 + s) * 32 + col];
        ov[c3][s] = v;
      }
    const float sc = fa.scale, sc2 = fa.scale * fa.scale;
    float u = ov[0][0], ux = ov[0][1] * sc, uy = ov[0][2] * sc, ud = ov[0][3] * sc2;
    float v = ov[1][0], vx = ov[1][1] * sc, vy = ov[1][2] * sc, vd = ov[1][3] * sc2;
    float p = ov[2][0], pxx = ov[2][1] * sc, pyy = ov[2][2] * sc;
    float an0 = 0.f, an1 = 0.f, an2 = 0.f;  // the column's anchors u*, v*, p*
    if constexpr (PT) {
      if (m) { an0 = fa.anchor[pt]; an1 = fa.anchor[(size_t)npad + pt]; an2 = fa.anchor[2 * (size_t)npad + pt]; }
    }
    HardBcPoint hb = {};
    if constexpr (HBC) {                    // hard wall conditions (point_stage.h): a masked or dummy column has D = 0
      hb = hard_bc_point(fa.hbc, m ? a.x[pt] : 0.f, m ? a.y[pt] : 0.f);
      hard_bc_apply(hb, true, u, ux, uy, ud);
      hard_bc_apply(hb, false, v, vx, vy, vd);
    }
    float vt = 0.f;
    float ev = (fa.e && m) ? fa.e[pt] : 0.f;
    if (fa.vtm && m) {
      vt = fminf(fa.vis_t0, vtm_old);
      if (owner) fa.vtm[pt] = fa.alpha_evm * fabsf(ev);
    }
    if (owner && fa.vis_used && m) fa.vis_used[pt] = vt;
    float nu = fa.inv_re + vt;
    float eq1 = (u * ux + v * uy) + pxx - nu * ud;
    float eq2 = (u * vx + v * vy) + pyy - nu * vd;
    if (owner && fa.lap) { fa.lap[pt] = ud; fa.lap[(size_t)npad + pt] = vd; }      // viscosity identification (point_stage.h)
    float eq3 = ux + vy;
    float eq4 = fa.e ? (eq1 * (u - 0.5f) + eq2 * (v - 0.5f)) - ev : 0.f;
    if (owner) {
      float* f = fa.fld + pt;
      f[FLD_U * (size_t)npad] = u; f[FLD_V * (size_t)npad] = v;
      f[FLD_UX * (size_t)npad] = ux; f[FLD_UY * (size_t)npad] = uy;
      f[FLD_VX * (size_t)npad] = vx; f[FLD_VY * (size_t)npad] = vy;
      f[FLD_EQ1 * (size_t)npad] = eq1; f[FLD_EQ2 * (size_t)npad] = eq2;
      f[FLD_EQ3 * (size_t)npad] = eq3; f[FLD_EQ4 * (size_t)npad] = eq4;
      f[FLD_P * (size_t)npad] = p;
      if (m) {
        float ww = fa.w ? fa.w[pt] : 1.f;
        if constexpr (PT) {                 // (the planes above hold the steady residuals)
          const float q1 = eq1 + fa.sigma * (u - an0), q2 = eq2 + fa.sigma * (v - an1);
          const float q3 = eq3 + fa.sigma_p * (p - an2);
          lsum[0] += ww * q1 * q1; lsum[1] += ww * q2 * q2;
          lsum[2] += ww * q3 * q3; lsum[3] += ww * eq4 * eq4;
        } else {
          lsum[0] += ww * eq1 * eq1; lsum[1] += ww * eq2 * eq2;
          lsum[2] += ww * eq3 * eq3; lsum[3] += ww * eq4 * eq4;
        }
      }
    }
    // output adjoints (point_stage.h output_adjoint_stage, residual mode) from the values above instead of the field planes
    HardBcPoint hbt = {};
    if constexpr (HBC) {
      // The constrained reverse sweep reads the planes back and computes the point's factors for itself: there 1 - Y
      // contracts into fma(-inv_len, eta - y0, 1), while above, beside the lift, where Y has other readers, it is
      // 1 - round(Y).  The transpose takes the reverse sweep's factors, computed again from an opaque copy of the
      // point, and the planes are opaque too, so that nothing of the map is contracted into the adjoints.
      float xo = m ? a.x[pt] : 0.f, yo = m ? a.y[pt] : 0.f;
      asm volatile("" : "+v"(xo), "+v"(yo));
      asm volatile("" : "+v"(u), "+v"(v), "+v"(ux), "+v"(uy), "+v"(vx), "+v"(vy));
      asm volatile("" : "+v"(eq1), "+v"(eq2), "+v"(eq3), "+v"(eq4));
      hbt = hard_bc_point(a.hbc, xo, yo);
    }
    float ww = m ? (a.w ? a.w[pt] : 1.f) : 0.f;
    float q1 = eq1, q2 = eq2, q3 = eq3;
    if constexpr (PT) {
      // The reverse sweep rebuilds q_k from the planes and the anchors: opaque copies, so that nothing of the forward's
      // expressions above is shared with or contracted into the seeds.
      asm volatile("" : "+v"(u), "+v"(v), "+v"(ux), "+v"(uy), "+v"(vx), "+v"(vy));
      asm volatile("" : "+v"(eq1), "+v"(eq2), "+v"(eq3), "+v"(eq4), "+v"(p));
      asm volatile("" : "+v"(an0), "+v"(an1), "+v"(an2));
      q1 = eq1; q2 = eq2; q3 = eq3;
      if (m) {
        q1 += a.sigma * (u - an0);
        q2 += a.sigma * (v - an1);
        q3 += a.sigma_p * (p - an2);
      }
    }
    float g1 = a.coef_eq[0] * ww * q1, g2 = a.coef_eq[1] * ww * q2, g3 = a.coef_eq[2] * ww * q3;
    float g4 = a.e ? a.coef_eq[3] * ww * eq4 : 0.f;
    float r1 = g1 + g4 * (u - 0.5f), r2 = g2 + g4 * (v - 0.5f), r3 = g3;
    float nub = a.inv_re + ((a.vis_used && m) ? vt : 0.f);
    const float bsc = a.scale, bsc2 = a.scale * a.scale;
    float au = r1 * ux + r2 * vx + g4 * eq1;
    float av = r1 * uy + r2 * vy + g4 * eq2;
    float ap = 0.f;
    if constexpr (PT) {
      // r1 u_x + r2 v_x starts with two products, and which of them is rounded by itself is the compiler's choice:
      // bwd_split_kernel rounds r1 u_x, this kernel rounded r2 v_x (1-ulp gradients).  The reverse sweep's pairing
      // written out, with the pseudo-time term last as there.
      float pu = r1 * ux, pv = r1 * uy;
      asm volatile("" : "+v"(pu), "+v"(pv));
      au = fmaf(a.sigma, g1, fmaf(g4, eq1, fmaf(r2, vx, pu)));
      av = fmaf(a.sigma, g2, fmaf(g4, eq2, fmaf(r2, vy, pv)));
      ap = a.sigma_p * g3;
    }
    if constexpr (HBC) {                    // the adjoints of the constrained fields, pulled back to the net's streams
      float aux = r1 * u + r3, auy = r1 * v, aud = -nub * r1;
      float avx = r2 * u, avy = r2 * v + r3, avd = -nub * r2;
      // The transpose's first sum, D a + D_X a_X + ..., starts with two products, and which of them is rounded by itself
      // is the compiler's choice by use counts: bwd_split_kernel rounds D_X a_X, this kernel rounded D a.  The reverse
      // sweep's pairing written out; the other three outputs are hard_bc_transpose's own.
      float pu = hbt.Dx * aux, pv = hbt.Dx * avx;
      asm volatile("" : "+v"(pu), "+v"(pv));
      const float nu0 = fmaf(hbt.Dd, aud, fmaf(hbt.Dy, auy, fmaf(hbt.D, au, pu)));
      const float nv0 = fmaf(hbt.Dd, avd, fmaf(hbt.Dy, avy, fmaf(hbt.D, av, pv)));
      hard_bc_transpose(hbt, au, aux, auy, aud);
      hard_bc_transpose(hbt, av, avx, avy, avd);
      au = nu0; av = nv0;
      oc[0][0] = au; oc[0][1] = aux * bsc; oc[0][2] = auy * bsc; oc[0][3] = aud * bsc2;
      oc[1][0] = av; oc[1][1] = avx * bsc; oc[1][2] = avy * bsc; oc[1][3] = avd * bsc2;
    } else {
      oc[0][0] = au; oc[0][1] = (r1 * u + r3) * bsc; oc[0][2] = (r1 * v) * bsc; oc[0][3] = -nub * r1 * bsc2;
      oc[1][0] = av; oc[1][1] = (r2 * u) * bsc; oc[1][2] = (r2 * v + r3) * bsc; oc[1][3] = -nub * r2 * bsc2;
    }
    oc[2][0] = ap; oc[2][1] = r1 * bsc; oc[2][2] = r2 * bsc; oc[2][3] = 0.f;
    // opaque from here on, as the LDS values of bwd_bf16_split.hip are: the compiler then contracts the epilogue's dot
    // products of them as there (with the zeros and expressions visible it picked other fma pairings: 1-ulp gradients)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(oc[c][s]));
    if (owner) {
      if (a.ebar && m) a.ebar[pt] = -g4;
      dbo[0] += au; dbo[1] += av;
      if constexpr (PT) dbo[2] += ap;
    }
  };

  // the output adjoints of XB: the point stage of the tile, or zeros for the dummy partner
  auto seed = [&](int tile, float vtm_old) {
    return [&, tile, vtm_old](int col, int h, float (&oc)[3][4]) {
      if (tile < a.ntiles) {
        point_stage(tile, col, w == 0 && h == 0, vtm_old, oc);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int s = 0; s < 4; ++s) { oc[c][s] = 0.f; asm volatile("" : "+v"(oc[c][s])); }
      }
    };
  };

  const int npairs = (a.ntiles + 1) / 2;
  if (grp == 1) SW::idle();
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int tile = 2 * pair + grp;
    // the tile's point and its vis_t_minus entry (read before the owner thread rewrites it in XB)
    float px, py, vtm_old;
    {
      const int pt = tile * PPL + (lane0 & 31);
      px = pt < a.n ? a.x[pt] : 0.f; py = pt < a.n ? a.y[pt] : 0.f;
      vtm_old = (fa.vtm && pt < a.n) ? fa.vtm[pt] : 0.f;
    }
    sw.template fphase<0, true>(0, tile, nullptr, a.x, a.y, a.n, partG, bias(0), none);
    for (int l = 1; l < L - 1; ++l) {
      sw.template mphase<false, false>(l, nullptr);
      sw.template fphase<1, true>(l, tile, Sw_of(tile, l), a.x, a.y, a.n, partG, bias(l), none);
    }
    sw.template mphase<false, false>(L - 1, nullptr);
    sw.template fphase<2, true>(L - 1, tile, nullptr, a.x, a.y, a.n, partG, bias(L - 1), none);                 // XA
    if constexpr (FF) {      // the reverse half that ends at E'_1 (see the head of the file)
      const bool more = L > 2;      // (L = 2: XB is the last phase)
      sw.template bphase<0, true>(L - 1, L, nullptr, Z_of(tile, L - 1), px, py, sgacc, sink, seed(tile, vtm_old), none, more);  // XB
      if (more) {
        for (int l = L - 1; l >= 3; --l) {
          sw.template mphase<true, true>(l, S_of(tile, l - 1));
          sw.template bphase<1, true>(l - 1, L, S_of(tile, l - 1), Z_of(tile, l - 1), px, py, sgacc, sink, none, none);
        }
        sw.template mphase<true, true>(2, S_of(tile, 1));
        sw.template bphase<1, true>(1, L, S_of(tile, 1), Z_of(tile, 1), px, py, sgacc, sink, none, none, false);
      }
    } else {
      sw.template bphase<0, true>(L - 1, L, nullptr, Z_of(tile, L - 1), px, py, sgacc, sink, seed(tile, vtm_old), none);  // XB
      for (int l = L - 1; l >= 2; --l) {
        sw.template mphase<true, true>(l, S_of(tile, l - 1));
        sw.template bphase<1, true>(l - 1, L, S_of(tile, l - 1), Z_of(tile, l - 1), px, py, sgacc, sink, none, none);
      }
      sw.template mphase<true, false>(1, nullptr);
      sw.template bphase<2, true>(0, L, nullptr, Z_of(tile, 0), px, py, sgacc, sink, none, none);
    }
  }
  if (grp == 0) SW::idle();
  // ---------------- flush: loss partials (fwd_split order), then dbo and the skinny gradients (bwd_split order) ----------------
  float* red = reinterpret_cast<float*>(ldsb);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k * 2 * GT + tid] = lsum[k];
  __syncthreads();
  if (tid < 4) {
    float s = 0.f;
    for (int t = 0; t < 2 * GT; ++t) s += red[tid * 2 * GT + t];
    fa.partials[blockIdx.x * PINN_NLOSS + tid] = s;
  } else if (tid < PINN_NLOSS) {
    fa.partials[blockIdx.x * PINN_NLOSS + tid] = 0.f;
  }
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
  for (int i = tid; i < SG; i += 2 * GT) out[i] = i >= sg_wout(HP, L) + 3 * HP && i < sg_bout(HP, L) ? 0.f : sgacc[i];
}

size_t fwdbwd_split_lds_bytes(int HP, int L) { (void)HP; return FusedLds<256>::bytes(L); }

template <int HP, int TERMS, bool HBC = false, bool PT = false, bool FF = false>
static int launch_one(const FwdArgs& fa, const BwdArgs& a, int grid, hipStream_t s) {
  const size_t lds = FusedLds<HP>::bytes(a.L);
  if (!spill_is(a.spill, act_block(HP), IN_P24_COMPACT) || !spill_is(fa.spill, act_block(HP), IN_P24_COMPACT)) return -1000;
  return launch_or_configure(&fwdbwd_split_kernel<HP, TERMS, HBC, PT, FF>, dim3(grid), dim3(2 * HP), lds, s, a.configure, fa, a);
}

// residual mode, MSE seeds, role-split plan (HP = 256, SPILL_P24_COMPACT)
int launch_fwdbwd_split(int HP, int terms, const FwdArgs& fa, const BwdArgs& a, int grid, hipStream_t s) {
  if (!fa.ff != !a.ff || (a.ff && a.L < 2)) return DISPATCH_UNSUPPORTED;      // (one net on both sides; the FF sweep ends at layer 1)
  return dispatch_width<256>(HP, DISPATCH_UNSUPPORTED, [&](auto hp) {
    return dispatch_ns_terms(4, terms, [&](auto, auto t) {
      return dispatch_variant<VARIANTS_SPLIT>(fa.hbc.kind, fa.ptime, fa.ff, [&](auto v) {
        using V = decltype(v);
        return launch_one<decltype(hp)::value, decltype(t)::value, V::hbc, V::pt, V::ff>(fa, a, grid, s);
      });
    });
  });
}
