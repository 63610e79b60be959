// Role-split forward and reverse sweep of one tile in ONE kernel (residual mode, MSE seeds, hidden 256): the phases of
// fwd_bf16_split.hip and bwd_bf16_split.hip (see there for the schedule, the shared K-region image and the reference
// lines replaced), run back to back per tile, so the last hidden layer's saved activations S_{L-1} never leave the
// registers.  S_{L-1} has one reader, the reverse sweep's first epilogue (dW_l needs a_{l-1}; the output-layer gradient
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
#include "kernels.h"
#include "bf16_util.h"
#include "reduce_util.h"

template <int HP>
struct FusedLds {
  using XI = XImg<HP, 32>;
  static constexpr size_t X_BYTES = XI::BYTES;
  static constexpr size_t PART_F = (size_t)2 * 4 * 12 * 32;            // [group][wave][3 outputs x 4 streams][32 points]
  static size_t bytes(int L) { return X_BYTES + (PART_F + 6 * HP + (size_t)sg_total(HP, L)) * sizeof(float); }
};

template <int HP, int TERMS>
__global__ __launch_bounds__(2 * HP, 1) void fwdbwd_split_kernel(FwdArgs fa, BwdArgs a) {
  static_assert(HP == 256, "four waves x 64 features per group");
  using G = FusedLds<HP>;
  using XI = typename G::XI;
  constexpr int GT = HP, KS = HP / 16, PPL = 32, COLS = 128;
  constexpr int RING = 2, WPRE = RING - 1, SQ = 2;        // weight ring, S quads requested ahead (the split pair's defaults)
  constexpr size_t PLQ = (size_t)(HP / 4) * PPL;          // f32x4 per plane of S / Z-bar
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  unsigned char* const X = ldsb;
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

  auto qbase = [&](int fb, int g) { return 64 * (2 * fb + (g >> 1)) + 16 * w + 8 * (g & 1); };
#define PHASE_LANE_F()                                 \
  int lane = lane0;                                    \
  asm volatile("" : "+v"(lane));                       \
  const int col = lane & 31, h = lane >> 5;            \
  (void)col; (void)h
#define E_SB() __builtin_amdgcn_sched_barrier(0)

  f32x16 acc[2][4];                       // [feature block][stream]
  u32x2 st[2][4][2];                      // parked epilogue output of one region: [quad][stream][hi | lo]
  u32x4 skeep[8][3];                      // S_{L-1} of the tile, 24-bit quads in the spill's plane order (XA -> XB)
  u32x4 sq[SQ + 1][3];                    // saved-activation quads in flight (reverse sweep)
  bool have_parked = false;

  // ---- bias quad of layer l from the prepared buffer (uniform address: scalar loads, no wait on the spill stores) ----
  auto bias4 = [&](int l, int fb, int g, int h) {
    typedef __attribute__((address_space(4))) const f32x4 cf32x4;
    const cf32x4* bp = (const cf32x4*)(uintptr_t)(P + prep_b(HP, l) + qbase(fb, g));
    const f32x4 b0 = bp[0], b1 = bp[1];
    return h ? b1 : b0;
  };
  auto dump_kp = [&](int fb, int g0, int k, int p, int col, int h) {
    const int off = XI::chunk_off(col, qbase(fb, g0 + k) >> 3) + 8 * h;
    *reinterpret_cast<u32x2*>(X + p * XI::PLANE * 2 + off) = st[k][p][0];
    if (TERMS == 3) *reinterpret_cast<u32x2*>(X + XI::HALF * 2 + p * XI::PLANE * 2 + off) = st[k][p][1];
  };
  auto dump_k = [&](int fb, int g0, int k, int col, int h) {
#pragma unroll
    for (int p = 0; p < 4; ++p) dump_kp(fb, g0, k, p, col, h);
  };
  auto dump = [&](int fb, int g0, int col, int h) { dump_k(fb, g0, 0, col, h); dump_k(fb, g0, 1, col, h); };

  u32x4 wh[2][RING], wl[2][RING];
  typedef __attribute__((address_space(1))) u32x4 gu32x4;
  auto w_lane = [&](int col, int h) { return ((2 * (col >> 4) + (w >> 1)) * KS) * 64 + 16 * (w & 1) + (col & 15) + 32 * h; };
  auto wload = [&](size_t poff, int s, int wlane) {      // poff: prep_wf (forward) or prep_wtf (reverse) of the layer
    const gu32x4* const wf = reinterpret_cast<const gu32x4*>(pin_base(reinterpret_cast<const u32x4*>(P + poff)));
#pragma unroll
    for (int fb = 0; fb < 2; ++fb) {
      wh[fb][s % RING] = (wf + (size_t)fb * 4 * KS * 64 + s * 64)[wlane];
      if (TERMS == 3) wl[fb][s % RING] = (wf + (size_t)(HP * HP / 8) + (size_t)fb * 4 * KS * 64 + s * 64)[wlane];
    }
  };
  auto quad_o = [&](int qq, int h) { return qbase(qq >> 2, qq & 3) + 4 * h; };
  auto sload = [&](const float* Sl, int qq, int col, int h) {
    const int o = quad_o(qq, h);
    const unsigned so = (unsigned)(((o - 4 * h) >> 2) + h) * PPL + col;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      sq[qq % (SQ + 1)][k] = __builtin_bit_cast(u32x4, __builtin_nontemporal_load(pin_base(reinterpret_cast<const f32x4*>(Sl) + k * PLQ) + so));
  };
  auto unpack_plane = [&](const u32x4 (&pk)[3], int p) {
    return unpack24(u32x2{pk[p >> 1][2 * (p & 1)], pk[p >> 1][2 * (p & 1) + 1]}, pk[2][p]);
  };
  // The dummy partner of an odd tile count reads its OWN S (the +1 scratch block its forward just wrote), not tile 0's as
  // bwd_bf16_split.hip does: here tile 0 may still be in its forward on another workgroup.  Its output adjoints are zero,
  // so its z-bars are zeros either way.
  auto s_layer = [&](int tile, int l) { return a.S + spill_off(tile, l, L, a.sl0, a.sblk, (size_t)HP * COLS); };

  // ---------------- M / G phase: acc <- W x image, region q in quarter q (both sweeps; fwd_bf16_split.hip) ----------------
  // REV: reverse sweep (W_l^T; parked region 3 dumped only after an E' phase that parked; pre_s: the next E' phase's
  // first S quads requested in the last k-steps)
  auto mphase = [&](auto REV, int l, int tile, auto PRE_S) {
    constexpr bool rev = decltype(REV)::value, pre_s = decltype(PRE_S)::value;
    PHASE_LANE_F();
    const int wlane = w_lane(col, h);
    const size_t poff = rev ? prep_wtf(HP, l) : prep_wf(HP, l);
    u32x4 bh[2], bo[2];
    const float* const Snext = rev && pre_s ? s_layer(tile, l - 1) : nullptr;
    auto bload = [&](int u) {
      const int s = u >> 2, j = u & 3;
      const int off = XI::chunk_off(col, 2 * s + h);
      bh[u & 1] = *reinterpret_cast<const u32x4*>(X + j * XI::PLANE * 2 + off);
      if (TERMS == 3) bo[u & 1] = *reinterpret_cast<const u32x4*>(X + XI::HALF * 2 + j * XI::PLANE * 2 + off);
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (rev && q == 0 && have_parked) dump(1, 2, col, h);
      bload(16 * q);
#pragma unroll
      for (int u = 16 * q; u < 16 * q + 16; ++u) {
        const int s = u >> 2, j = u & 3;
        if (j == 0 && s + WPRE < KS) wload(poff, s + WPRE, wlane);
        if (rev && pre_s && u >= 4 * (KS - WPRE) && u < 4 * (KS - WPRE) + SQ) sload(Snext, u - 4 * (KS - WPRE), col, h);
        if ((u & 15) != 15) bload(u + 1);
        if (!rev && q == 0 && (u & 1)) dump_kp(1, 2, u >> 3, (u >> 1) & 3, col, h);
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) {
          if (s == 0) {
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[fb][j] = TERMS == 3 ? MFMA_Q(0, wh[fb][0], bo[u & 1], zero) : MFMA_Q(0, wh[fb][0], bh[u & 1], zero);
            if (TERMS == 3) {
              acc[fb][j] = MFMA_Q(1, wl[fb][0], bh[u & 1], acc[fb][j]);
              acc[fb][j] = MFMA_Q(0, wh[fb][0], bh[u & 1], acc[fb][j]);
            }
          } else {
            if (TERMS == 3) {
              acc[fb][j] = MFMA_Q(s, wh[fb][s % RING], bo[u & 1], acc[fb][j]);
              acc[fb][j] = MFMA_Q(s + 1, wl[fb][s % RING], bh[u & 1], acc[fb][j]);
            }
            acc[fb][j] = MFMA_Q(s, wh[fb][s % RING], bh[u & 1], acc[fb][j]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }
    have_parked = false;
  };

  // ---------------- forward E phase of layer lE (fwd_bf16_split.hip) ----------------
  // EK: 0 = layer 0, 1 = hidden layer 1..L-2 (S spilled), 2 = last hidden layer = XA (output layer, S kept in skeep)
  auto fphase = [&](auto EKIND, int lE, int tileE) {
    constexpr int EK = decltype(EKIND)::value;
    constexpr bool last = EK == 2, first = EK == 0;
    PHASE_LANE_F();
    float* const Sl = fa.S + spill_off(tileE, lE, L, a.sl0, a.sblk, (size_t)HP * COLS);
    float po[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) po[c][s] = 0.f;
    float px = 0.f, py = 0.f;
    if (first) {
      const int pt = tileE * PPL + col;
      px = pt < a.n ? a.x[pt] : 0.f; py = pt < a.n ? a.y[pt] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int fb = q >> 1;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int g = 2 * (q & 1) + k, o = qbase(fb, g) + 4 * h;
        if (!last && q == 3 && k == 1) {      // first weight k-steps of M_{lE+1}
#pragma unroll
          for (int s = 0; s < WPRE; ++s) wload(prep_wf(HP, lE + 1), s, w_lane(col, h));
        }
        f32x4 av[4], sv[4];
        f32x4 b4, wx4, wy4;
        if (first) {
          wx4 = *reinterpret_cast<const f32x4*>(w0L + o); wy4 = *reinterpret_cast<const f32x4*>(w0L + HP + o);
          b4 = *reinterpret_cast<const f32x4*>(w0L + 2 * HP + o);
        } else {
          b4 = bias4(lE, fb, g, h);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          float z, zx, zy, zd;
          if (first) {
            z = fmaf(wx4[e], px, fmaf(wy4[e], py, b4[e])); zx = wx4[e]; zy = wy4[e]; zd = 0.f;
          } else {
            z = acc[fb][0][r] + b4[e]; zx = acc[fb][1][r]; zy = acc[fb][2][r]; zd = acc[fb][3][r];
          }
          const float t = fast_tanh(z);
          const float d1 = 1.f - t * t;
          const float d2 = -2.f * t * d1;
          av[0][e] = t; av[1][e] = d1 * zx; av[2][e] = d1 * zy; av[3][e] = d2 * (zx * zx + zy * zy) + d1 * zd;
          sv[0][e] = t; sv[1][e] = zx; sv[2][e] = zy; sv[3][e] = zd;
          E_SB();
        }
        const unsigned so = (unsigned)(((o - 4 * h) >> 2) + h) * PPL + col;
        u32x4 pk[3];
        if (q > 0 && !last) dump_k((q - 1) >> 1, 2 * ((q - 1) & 1), k, col, h);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          if (!last) {
            split4(av[p][0], av[p][1], av[p][2], av[p][3], st[k][p][0], st[k][p][1]);
          } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const f32x4 wo = *reinterpret_cast<const f32x4*>(woutL + c * HP + o);
#pragma unroll
              for (int e = 0; e < 4; ++e) po[c][p] = fmaf(wo[e], av[p][e], po[c][p]);
            }
          }
          if (!first) {      // 24-bit format (bf16_util.h pack24): spilled, or kept for XB
            u32x2 hi24; unsigned lo24;
            pack24(sv[p], hi24, lo24);
            pk[p >> 1][2 * (p & 1)] = hi24[0]; pk[p >> 1][2 * (p & 1) + 1] = hi24[1]; pk[2][p] = lo24;
            if (!last) {
              if (p & 1) __builtin_nontemporal_store(__builtin_bit_cast(f32x4, pk[p >> 1]), pin_base(reinterpret_cast<const f32x4*>(Sl) + (p >> 1) * PLQ) + so);
              if (p == 3) __builtin_nontemporal_store(__builtin_bit_cast(f32x4, pk[2]), pin_base(reinterpret_cast<const f32x4*>(Sl) + 2 * PLQ) + so);
            }
          }
          if (last) asm volatile("" : "+v"(po[0][p]), "+v"(po[1][p]), "+v"(po[2][p]));
          E_SB();
        }
        if (last) {
#pragma unroll
          for (int kk = 0; kk < 3; ++kk) skeep[2 * q + k][kk] = pk[kk];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (last && q == 3) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            partG[(w * 12 + c * 4 + s) * 32 + col] = po[c][s] + __shfl_xor(po[c][s], 32, 64);
      }
      __syncthreads();
    }
  };

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
        lsum[0] += ww * eq1 * eq1; lsum[1] += ww * eq2 * eq2;
        lsum[2] += ww * eq3 * eq3; lsum[3] += ww * eq4 * eq4;
      }
    }
    // output adjoints (point_stage.h output_adjoint_stage, residual mode) from the values above instead of the field planes
    float ww = m ? (a.w ? a.w[pt] : 1.f) : 0.f;
    float g1 = a.coef_eq[0] * ww * eq1, g2 = a.coef_eq[1] * ww * eq2, g3 = a.coef_eq[2] * ww * eq3;
    float g4 = a.e ? a.coef_eq[3] * ww * eq4 : 0.f;
    float r1 = g1 + g4 * (u - 0.5f), r2 = g2 + g4 * (v - 0.5f), r3 = g3;
    float nub = a.inv_re + ((a.vis_used && m) ? vt : 0.f);
    const float bsc = a.scale, bsc2 = a.scale * a.scale;
    float au = r1 * ux + r2 * vx + g4 * eq1;
    float av = r1 * uy + r2 * vy + g4 * eq2;
    oc[0][0] = au; oc[0][1] = (r1 * u + r3) * bsc; oc[0][2] = (r1 * v) * bsc; oc[0][3] = -nub * r1 * bsc2;
    oc[1][0] = av; oc[1][1] = (r2 * u) * bsc; oc[1][2] = (r2 * v + r3) * bsc; oc[1][3] = -nub * r2 * bsc2;
    oc[2][0] = 0.f; oc[2][1] = r1 * bsc; oc[2][2] = r2 * bsc; oc[2][3] = 0.f;
    // opaque from here on, as the LDS values of bwd_bf16_split.hip are: the compiler then contracts the epilogue's dot
    // products of them exactly as there (with the zeros and expressions visible it picked other fma pairings: 1-ulp dW_out)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(oc[c][s]));
    if (owner) {
      if (a.ebar && m) a.ebar[pt] = -g4;
      dbo[0] += au; dbo[1] += av;
    }
  };

  // ---------------- reverse E phase of layer lE (bwd_bf16_split.hip) ----------------
  // EK: 0 = last hidden layer = XB (point stage first; S from skeep), 1 = layer L-2..1, 2 = layer 0 (recomputed S)
  auto bphase = [&](auto EKIND, int lE, int tileE, float pxE, float pyE, float vtm_old) {
    constexpr int EK = decltype(EKIND)::value;
    constexpr bool first = EK == 0, last = EK == 2;
    PHASE_LANE_F();
    const float* const Sl = s_layer(tileE, lE);
    float* const Zl = a.Zb + spill_off(tileE, lE, L, a.sl0, a.sblk, (size_t)HP * COLS);
    float oc[3][4];
    if (first) {
      if (tileE < a.ntiles) {
        point_stage(tileE, col, w == 0 && h == 0, vtm_old, oc);
      } else {      // the dummy partner tile: zero output adjoints
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int s = 0; s < 4; ++s) { oc[c][s] = 0.f; asm volatile("" : "+v"(oc[c][s])); }
      }
    }
    auto commit = [&](int base, int o4, float v) {        // lanes col < 4 of each half own feature o4 + col (reduce_util.h)
      float* p = col < 4 ? &sgacc[base + o4 + (col & 3)] : &sink[lane];
      lds_rmw_add(p, v);
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q > 0 && !last) dump((q - 1) >> 1, 2 * ((q - 1) & 1), col, h);
      const int fb = q >> 1;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int g = 2 * (q & 1) + k, qq = 2 * q + k, o = quad_o(qq, h);
        if (!first && !last && qq + SQ < 8) sload(Sl, qq + SQ, col, h);
        if (!last && qq == 7) {
#pragma unroll
          for (int s = 0; s < WPRE; ++s) wload(prep_wtf(HP, lE), s, w_lane(col, h));
        }
        f32x4 sc[4];
        if (last) {
          const f32x4 wx4 = *reinterpret_cast<const f32x4*>(w0L + o), wy4 = *reinterpret_cast<const f32x4*>(w0L + HP + o);
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(w0L + 2 * HP + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) sc[0][e] = fast_tanh(fmaf(wx4[e], pxE, fmaf(wy4[e], pyE, b4[e])));
          sc[1] = wx4; sc[2] = wy4; sc[3] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else if (first) {
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            sc[p] = unpack_plane(skeep[qq], p);
            asm volatile("" : "+v"(sc[p]));      // opaque, as the values bwd_bf16_split.hip reads back
          }
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p) sc[p] = unpack_plane(sq[qq % (SQ + 1)], p);
        }
        f32x4 zq[4], wov[3], dwv[2], wo4[3];
        if (first) {
#pragma unroll
          for (int c = 0; c < 3; ++c) wo4[c] = *reinterpret_cast<const f32x4*>(woutL + c * HP + o);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          float ga, gx, gy, gd;
          if (first) {
            ga = wo4[0][e] * oc[0][0] + wo4[1][e] * oc[1][0] + wo4[2][e] * oc[2][0];
            gx = wo4[0][e] * oc[0][1] + wo4[1][e] * oc[1][1] + wo4[2][e] * oc[2][1];
            gy = wo4[0][e] * oc[0][2] + wo4[1][e] * oc[1][2] + wo4[2][e] * oc[2][2];
            gd = wo4[0][e] * oc[0][3] + wo4[1][e] * oc[1][3] + wo4[2][e] * oc[2][3];
          } else {
            ga = acc[fb][0][r]; gx = acc[fb][1][r]; gy = acc[fb][2][r]; gd = acc[fb][3][r];
          }
          const float t = sc[0][e], zx = sc[1][e], zy = sc[2][e], zd = sc[3][e];
          const float d1 = 1.f - t * t;
          const float d2 = -2.f * t * d1;
          const float d3 = -2.f * d1 * (1.f - 3.f * t * t);
          const float zz = zx * zx + zy * zy;
          zq[1][e] = d1 * gx + 2.f * d2 * zx * gd;
          zq[2][e] = d1 * gy + 2.f * d2 * zy * gd;
          zq[3][e] = d1 * gd;
          zq[0][e] = d1 * ga + d2 * (zx * gx + zy * gy) + (d3 * zz + d2 * zd) * gd;
          if (first) {
            const float ax = d1 * zx, ay = d1 * zy, ad = d2 * zz + d1 * zd;
#pragma unroll
            for (int c = 0; c < 3; ++c) wov[c][e] = oc[c][0] * t + oc[c][1] * ax + oc[c][2] * ay + oc[c][3] * ad;
          }
          if (last) { dwv[0][e] = zq[0][e] * pxE + zq[1][e]; dwv[1][e] = zq[0][e] * pyE + zq[2][e]; }
          E_SB();
        }
        const int o4 = o;
        commit(sg_db(HP, lE), o4, sum_cols4<32>(zq[0][0], zq[0][1], zq[0][2], zq[0][3], lane));
        if (first) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            commit(sg_wout(HP, L) + c * HP, o4, sum_cols4<32>(wov[c][0], wov[c][1], wov[c][2], wov[c][3], lane));
        }
        if (last) {
          commit(sg_w0x(HP, L), o4, sum_cols4<32>(dwv[0][0], dwv[0][1], dwv[0][2], dwv[0][3], lane));
          commit(sg_w0y(HP, L), o4, sum_cols4<32>(dwv[1][0], dwv[1][1], dwv[1][2], dwv[1][3], lane));
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!last) {
          const unsigned so = (unsigned)(((o - 4 * h) >> 2) + h) * PPL + col;
          u32x4 pk[3];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            split4(zq[p][0], zq[p][1], zq[p][2], zq[p][3], st[k][p][0], st[k][p][1]);
            u32x2 hi24; unsigned lo24;
            pack24(zq[p], hi24, lo24);
            pk[p >> 1][2 * (p & 1)] = hi24[0]; pk[p >> 1][2 * (p & 1) + 1] = hi24[1]; pk[2][p] = lo24;
            if (p & 1) __builtin_nontemporal_store(__builtin_bit_cast(f32x4, pk[p >> 1]), pin_base(reinterpret_cast<const f32x4*>(Zl) + (p >> 1) * PLQ) + so);
            if (p == 3) __builtin_nontemporal_store(__builtin_bit_cast(f32x4, pk[2]), pin_base(reinterpret_cast<const f32x4*>(Zl) + 2 * PLQ) + so);
            E_SB();
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }
    have_parked = !last;
  };
  auto idle = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) __syncthreads();
  };

  using K0 = std::integral_constant<int, 0>;
  using K1 = std::integral_constant<int, 1>;
  using K2 = std::integral_constant<int, 2>;
  using FWD = std::false_type;
  using REV = std::true_type;
  const int npairs = (a.ntiles + 1) / 2;
  if (grp == 1) idle();
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int tile = 2 * pair + grp;
    // the tile's point and its vis_t_minus entry (read before the owner thread rewrites it in XB)
    float px, py, vtm_old;
    {
      const int pt = tile * PPL + (lane0 & 31);
      px = pt < a.n ? a.x[pt] : 0.f; py = pt < a.n ? a.y[pt] : 0.f;
      vtm_old = (fa.vtm && pt < a.n) ? fa.vtm[pt] : 0.f;
    }
    fphase(K0{}, 0, tile);
    for (int l = 1; l < L - 1; ++l) {
      mphase(FWD{}, l, tile, std::false_type{});
      fphase(K1{}, l, tile);
    }
    mphase(FWD{}, L - 1, tile, std::false_type{});
    fphase(K2{}, L - 1, tile);                                  // XA
    bphase(K0{}, L - 1, tile, px, py, vtm_old);                 // XB
    for (int l = L - 1; l >= 2; --l) {
      mphase(REV{}, l, tile, std::true_type{});
      bphase(K1{}, l - 1, tile, px, py, 0.f);
    }
    mphase(REV{}, 1, tile, std::false_type{});
    bphase(K2{}, 0, tile, px, py, 0.f);
  }
  if (grp == 0) idle();
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

template <int HP, int TERMS>
static int launch_one(const FwdArgs& fa, const BwdArgs& a, int grid, hipStream_t s) {
  const size_t lds = FusedLds<HP>::bytes(a.L);
  if (a.configure) {   // pinn_plan_create: raise the kernel's dynamic-LDS limit on the current device
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fwdbwd_split_kernel<HP, TERMS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, PINN_LDS_MAX);
    return e == hipSuccess ? 0 : -(int)e;
  }
  hipLaunchKernelGGL((fwdbwd_split_kernel<HP, TERMS>), dim3(grid), dim3(2 * HP), lds, s, fa, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// residual mode, MSE seeds, role-split plan (HP = 256, s0_skip, compact 24-bit spill; the caller checks)
int launch_fwdbwd_split(int HP, int terms, const FwdArgs& fa, const BwdArgs& a, int grid, hipStream_t s) {
  if (HP != 256) return -1000;
  return terms == 3 ? launch_one<256, 3>(fa, a, grid, s) : launch_one<256, 1>(fa, a, grid, s);
}
