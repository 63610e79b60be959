// Phase bodies of the role-split hidden-256 sweeps, written once for fwd_bf16_split.hip, bwd_bf16_split.hip and
// fwdbwd_bf16_split.hip (the schedule: fwd_bf16_split.hip; KEEP: the fused kernel's S_{L-1}, handed from the forward's
// last epilogue to the reverse sweep's first in registers instead of through the spill).  A SplitWave is one
// wave's register state - accumulators, parked region, weight ring, saved-activation quads in flight - with the K-region
// geometry and the phases that use it.  A kernel keeps its LDS layout, bias source, point stage, the S source of a dummy
// partner tile and its program; it hands the phases what differs as arguments (spill blocks, LDS rows) and as callables
// (bias, output adjoints, per-quarter work).
//
// Every phase is force-inlined into a straight-line per-group program: no per-phase dispatch (with one, the register
// allocator spilled the whole accumulator set around the phase loop).
//
// FF: the net's first layer is the frozen sine layer (spill_io.h layer0_sine).  The forward's E phase of
// layer 0 forms the four a-streams by that one function instead of the tanh chain rule; nothing else of the forward
// changes (layer 0 has no slot in the compact layout either way).  The layer is not trained, so the reverse sweep of an
// FF kernel ends at E_1 - no G_1, no E_0 - and that last phase runs with park = false (bphase).
#pragma once
#include "kernels.h"
#include "bf16_util.h"
#include "reduce_util.h"

template <int HP, int TERMS, bool FF = false>
struct SplitWave {
  static_assert(HP == 256, "four waves x 64 features per group");
  using XI = XImg<HP, 32>;
  typedef __attribute__((address_space(1))) u32x4 gu32x4;
  static constexpr int KS = HP / 16, PPL = 32, COLS = 128;
  static constexpr int RING = 2, WPRE = RING - 1;         // weight k-steps in the register ring / requested ahead
  static constexpr int SQ = 2;                            // saved-activation quads requested ahead (reverse sweep)
  static constexpr size_t PLQ = (size_t)(HP / 4) * PPL;   // f32x4 per plane of S / Z-bar

  unsigned char* const X;                 // the shared K-region image
  const float* const P;                   // prepared parameters
  const float* const woutL;               // [3][HP] LDS rows
  const float* const w0L;                 // [w0x | w0y | b0][HP] LDS rows
  const int w, lane0;                     // wave in the group, lane
  f32x16 acc[2][4];                       // accumulators: [feature block][stream]
  u32x2 st[2][4][2];                      // parked epilogue output of one region: [quad][stream][hi | lo]
  // weight-fragment ring [feature block][k-step % RING].  It lives across phases: the first WPRE k-steps of an M / G
  // phase are requested during the last quad of the E phase before it, so no M / G phase opens with an L2 round trip.
  u32x4 wh[2][RING], wl[2][RING];
  u32x4 sq[SQ + 1][3];                    // saved-activation quads in flight, 24-bit format (spill_io.h pack24)
  u32x4 skeep[8][3];                      // S_{L-1} kept in registers from the forward to the reverse epilogue (KEEP)
  bool have_parked = false;               // the last E phase parked region 3 (reverse sweep: G dumps it in quarter 0)

  __device__ __forceinline__ SplitWave(unsigned char* X_, const float* P_, const float* woutL_, const float* w0L_, int w_, int lane0_)
      : X(X_), P(P_), woutL(woutL_), w0L(w0L_), w(w_), lane0(lane0_) {}

  // Lane geometry is re-derived inside every phase from an opaque copy of the lane id: address arithmetic then lives
  // in the phase that uses it instead of being hoisted in front of the phase loop (it was: 139 spilled registers).
  __device__ __forceinline__ int phase_lane() const {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    return lane;
  }
  // feature geometry: row i of the wave's 32-row block fb is feature 64 (2 fb + (i >> 4)) + 16 w + (i & 15), i.e. the
  // register quad (fb, g) (rows 8g + 4h + e) holds features qbase(fb, g) + 4h + e of region 2 fb + (g >> 1)
  __device__ __forceinline__ int qbase(int fb, int g) const { return 64 * (2 * fb + (g >> 1)) + 16 * w + 8 * (g & 1); }
  __device__ __forceinline__ int quad_o(int qq, int h) const { return qbase(qq >> 2, qq & 3) + 4 * h; }      // qq = 4 fb + g
  // this wave's rows in the prepared weight image (32-row blocks b, lane slot r + 32 h): per-lane offset in u32x4
  // units, plus fb * 4 * KS * 64 + s * 64 (uniform)
  __device__ __forceinline__ int w_lane(int col, int h) const {
    return ((2 * (col >> 4) + (w >> 1)) * KS) * 64 + 16 * (w & 1) + (col & 15) + 32 * h;
  }
  // k-step s of the weight image at P + poff (prep_wf: W_l, forward; prep_wtf: W_l^T, reverse) into the ring
  __device__ __forceinline__ void wload(size_t poff, int s, int wlane) {
    const gu32x4* const wf = reinterpret_cast<const gu32x4*>(pin_base(reinterpret_cast<const u32x4*>(P + poff)));
#pragma unroll
    for (int fb = 0; fb < 2; ++fb) {
      wh[fb][s % RING] = (wf + (size_t)fb * 4 * KS * 64 + s * 64)[wlane];
      if (TERMS == 3) wl[fb][s % RING] = (wf + (size_t)(HP * HP / 8) + (size_t)fb * 4 * KS * 64 + s * 64)[wlane];
    }
  }
  // parked quad (fb, g0 + k), stream p -> image
  __device__ __forceinline__ void dump_kp(int fb, int g0, int k, int p, int col, int h) {
    const int off = XI::chunk_off(col, qbase(fb, g0 + k) >> 3) + 8 * h;
    *reinterpret_cast<u32x2*>(X + p * XI::PLANE * 2 + off) = st[k][p][0];
    if (TERMS == 3) *reinterpret_cast<u32x2*>(X + XI::HALF * 2 + p * XI::PLANE * 2 + off) = st[k][p][1];
  }
  __device__ __forceinline__ void dump_k(int fb, int g0, int k, int col, int h) {
#pragma unroll
    for (int p = 0; p < 4; ++p) dump_kp(fb, g0, k, p, col, h);
  }
  __device__ __forceinline__ void dump(int fb, int g0, int col, int h) { dump_k(fb, g0, 0, col, h); dump_k(fb, g0, 1, col, h); }
  // saved-activation quad qq of the spill block Sl into the in-flight slot qq % (SQ + 1)
  __device__ __forceinline__ void sload(const float* Sl, int qq, int col, int h) {
    const int o = quad_o(qq, h);
    const unsigned so = (unsigned)(((o - 4 * h) >> 2) + h) * PPL + col;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      sq[qq % (SQ + 1)][k] = __builtin_bit_cast(u32x4, __builtin_nontemporal_load(pin_base(reinterpret_cast<const f32x4*>(Sl) + k * PLQ) + so));
  }
  __device__ __forceinline__ static void idle() {
#pragma unroll
    for (int q = 0; q < 4; ++q) __syncthreads();
  }

  // ---------------- M / G phase: acc <- W_l x image (forward) or W_l^T x image (REV), region q in quarter q ----------------
  // The forward writes the parked region 3 of the E phase before during quarter 0, one stream of a quad every other
  // step (a burst of 64 writes per CU behind the barrier sits in the LDS queue in front of the partner group's first
  // B-fragment reads); the reverse sweep dumps it at the top of quarter 0, if the E phase before parked.  PRE_S: the
  // next E phase's first SQ saved-activation quads, from Snext, are requested in the last k-steps, younger than every
  // weight request of this phase.
  template <bool REV, bool PRE_S>
  __device__ __forceinline__ void mphase(int l, const float* Snext) {
    const int lane = phase_lane(), col = lane & 31, h = lane >> 5;
    const int wlane = w_lane(col, h);
    const size_t poff = REV ? prep_wtf(HP, l) : prep_wf(HP, l);
    u32x4 bh[2], bo[2];
    auto bload = [&](int u) {
      const int s = u >> 2, j = u & 3;
      const int off = XI::chunk_off(col, 2 * s + h);
      bh[u & 1] = *reinterpret_cast<const u32x4*>(X + j * XI::PLANE * 2 + off);
      if (TERMS == 3) bo[u & 1] = *reinterpret_cast<const u32x4*>(X + XI::HALF * 2 + j * XI::PLANE * 2 + off);
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (REV && q == 0 && have_parked) dump(1, 2, col, h);
      bload(16 * q);
#pragma unroll
      for (int u = 16 * q; u < 16 * q + 16; ++u) {
        const int s = u >> 2, j = u & 3;
        if (j == 0 && s + WPRE < KS) wload(poff, s + WPRE, wlane);
        if (PRE_S && u >= 4 * (KS - WPRE) && u < 4 * (KS - WPRE) + SQ) sload(Snext, u - 4 * (KS - WPRE), col, h);
        if ((u & 15) != 15) bload(u + 1);
        if (!REV && q == 0 && (u & 1)) dump_kp(1, 2, u >> 3, (u >> 1) & 3, col, h);
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) {
          if (s == 0) {
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[fb][j] = TERMS == 3 ? mfma_bf16(wh[fb][0], bo[u & 1], zero) : mfma_bf16(wh[fb][0], bh[u & 1], zero);
            if (TERMS == 3) {
              acc[fb][j] = mfma_bf16(wl[fb][0], bh[u & 1], acc[fb][j]);
              acc[fb][j] = mfma_bf16(wh[fb][0], bh[u & 1], acc[fb][j]);
            }
          } else {
            if (TERMS == 3) {
              acc[fb][j] = mfma_bf16(wh[fb][s % RING], bo[u & 1], acc[fb][j]);
              acc[fb][j] = mfma_bf16(wl[fb][s % RING], bh[u & 1], acc[fb][j]);
            }
            acc[fb][j] = mfma_bf16(wh[fb][s % RING], bh[u & 1], acc[fb][j]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);      // requests stay where they are written (one k-step / one step ahead)
      }
      __syncthreads();
    }
    have_parked = false;
  }

  // ---------------- forward E phase: tanh chain rule of layer lE ----------------
  // EK: 0 = layer 0 (pre-activations from the point (x, y) on the VALU; nothing spilled; FF: layer0_sine), 1 = hidden layer 1..L-2,
  // 2 = last hidden layer (output layer folded into the per-wave partials partG, nothing parked).  S goes to the
  // block Sl, or, for EK 2 with KEEP, to skeep.  bias(fb, g, o, h): the bias quad of features o..o+3;
  // quarter(q): the kernel's work at the top of quarter q.
  template <int EK, bool KEEP, class Bias, class Quarter>
  __device__ __forceinline__ void fphase(int lE, int tileE, float* Sl, const float* x, const float* y, int n, float* partG,
                                         Bias bias, Quarter quarter) {
    constexpr bool last = EK == 2, first = EK == 0;
    const int lane = phase_lane(), col = lane & 31, h = lane >> 5;
    float po[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) po[c][s] = 0.f;
    float px = 0.f, py = 0.f;
    if (first) {
      const int pt = tileE * PPL + col;
      px = pt < n ? x[pt] : 0.f; py = pt < n ? y[pt] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      quarter(q);
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
          b4 = bias(fb, g, o, h);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          float z, zx, zy, zd;
          if (first) {
            z = layer0_z(wx4[e], wy4[e], b4[e], px, py); zx = wx4[e]; zy = wy4[e]; zd = 0.f;
          } else {
            z = acc[fb][0][r] + b4[e]; zx = acc[fb][1][r]; zy = acc[fb][2][r]; zd = acc[fb][3][r];
          }
          if constexpr (FF && first) {      // the frozen sine layer: the a-streams by its one statement, nothing saved
            float f0, f1, f2, f3;
            layer0_sine(z, zx, zy, SinCosFast(), f0, f1, f2, f3);
            av[0][e] = f0; av[1][e] = f1; av[2][e] = f2; av[3][e] = f3;
          } else {
            const float t = fast_tanh(z);
            const float d1 = 1.f - t * t;
            const float d2 = -2.f * t * d1;
            av[0][e] = t; av[1][e] = d1 * zx; av[2][e] = d1 * zy; av[3][e] = d2 * (zx * zx + zy * zy) + d1 * zd;
            sv[0][e] = t; sv[1][e] = zx; sv[2][e] = zy; sv[3][e] = zd;
          }
          __builtin_amdgcn_sched_barrier(0);      // the epilogue's elements / planes are scheduled one at a time
        }
        const unsigned so = (unsigned)(((o - 4 * h) >> 2) + h) * PPL + col;
        u32x4 pk[3];      // the quad's 24-bit spill: hi16 of streams 0-1, hi16 of streams 2-3, lo8 of all four
        // region q - 1, parked in the previous quarter, is free now: quad k leaves its registers just before they are refilled
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
          // (layer 0 is not spilled: t = tanh(w0x x + w0y y + b0), z_x = w0x, z_y = w0y, z_D = 0 cost the reverse sweep
          // and the dW kernel one FMA pair and one tanh to recompute - a sixth of the spill at 6 layers)
          if (!first) {
            pack24_plane(sv[p], p, pk);
            if (!(KEEP && last)) store24_planes(Sl, PLQ, so, p, pk);
          }
          if (last) asm volatile("" : "+v"(po[0][p]), "+v"(po[1][p]), "+v"(po[2][p]));   // (no sinking behind the loop)
          __builtin_amdgcn_sched_barrier(0);
        }
        if (KEEP && last) {
#pragma unroll
          for (int kk = 0; kk < 3; ++kk) skeep[2 * q + k][kk] = pk[kk];
        }
        __builtin_amdgcn_sched_barrier(0);        // 128 arch VGPRs: do not interleave the two quads' live ranges
      }
      if (last && q == 3) {
        // the lane pair (l, l + 32) holds the same column: add the halves (both publish the same value)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            partG[(w * 12 + c * 4 + s) * 32 + col] = po[c][s] + __shfl_xor(po[c][s], 32, 64);
      }
      __syncthreads();
    }
  }

  // ---------------- reverse E phase: tanh adjoint of layer lE ----------------
  // EK: 0 = last hidden layer L-1 (a-stream adjoints from the output adjoints on the VALU, dW_out), 1 = layer L-2..1,
  // 2 = layer 0 (dW_0; its saved activations recomputed from the point (pxE, pyE); nothing parked, no spill).
  // Saved activations come from the block Sl (requested SQ quads ahead; all but EK 0's by the G phase before), or, for
  // EK 0 with KEEP, from skeep.  Z-bar goes to the block Zl.  The column sums of the skinny gradients go into sgacc;
  // the lanes that own no slot add into sink[lane].  seed(col, h, oc): EK 0's output adjoints [output][stream];
  // quarter(q): the kernel's work at the end of quarter q.
  // park = false (orthogonal to EK; the last phase of an FF reverse sweep, E_1 or for L = 2 the seed phase itself): no G
  // phase follows, so z-bar is spilled to Zl as ever (dW reads it) but neither split into st nor dumped into the image,
  // no weight k-step of a G phase is requested, and have_parked stays false.  The phase then touches no image, as EK 2
  // does, and keeps its four barriers.  An argument, not a template parameter: uniform, a constant wherever the phase
  // is inlined but in the seed phase of an FF kernel (L = 2 or not), which a second instantiation would duplicate.
  template <int EK, bool KEEP, class Seed, class Quarter>
  __device__ __forceinline__ void bphase(int lE, int L, const float* Sl, float* Zl, float pxE, float pyE, float* sgacc,
                                         float* sink, Seed seed, Quarter quarter, bool park = true) {
    constexpr bool first = EK == 0, last = EK == 2;
    const int lane = phase_lane(), col = lane & 31, h = lane >> 5;
    float oc[3][4];
    if (first) seed(col, h, oc);
    auto commit = [&](int base, int o4, float v) {        // lanes col < 4 of each half own feature o4 + col (reduce_util.h)
      float* p = col < 4 ? &sgacc[base + o4 + (col & 3)] : &sink[lane];
      lds_rmw_add(p, v);      // (unconditional, the other lanes hit a sink: a plain read-modify-write costs the same for 8 lanes as for 64)
    };
    if (first && !KEEP) {
#pragma unroll
      for (int qq = 0; qq < SQ; ++qq) sload(Sl, qq, col, h);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q > 0 && !last && park) dump((q - 1) >> 1, 2 * ((q - 1) & 1), col, h);
      const int fb = q >> 1;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int g = 2 * (q & 1) + k, qq = 2 * q + k, o = quad_o(qq, h);
        if (!last && !(first && KEEP) && qq + SQ < 8) sload(Sl, qq + SQ, col, h);
        if (!last && park && qq == 7) {      // first weight k-steps of G_lE
#pragma unroll
          for (int s = 0; s < WPRE; ++s) wload(prep_wtf(HP, lE), s, w_lane(col, h));
        }
        f32x4 sc[4];
        if (last) {
          // layer 0 is not stored: recomputed as the forward computed it
          layer0_saved(*reinterpret_cast<const f32x4*>(w0L + o), *reinterpret_cast<const f32x4*>(w0L + HP + o),
                       *reinterpret_cast<const f32x4*>(w0L + 2 * HP + o), pxE, pyE, TanhFast(), sc[0], sc[1], sc[2], sc[3]);
        } else if (first && KEEP) {
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            sc[p] = unpack24_plane(skeep[qq], p);
            asm volatile("" : "+v"(sc[p]));      // opaque, as the values read back from a spill
          }
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p) sc[p] = unpack24_plane(sq[qq % (SQ + 1)], p);
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
          if (first) {      // adjoint of the last hidden layer's a-streams: rank-3 update from the output adjoints
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
          if (first) {      // dWout[c][o] += sum_s oadj[c][s] * a_s[o]
            // (fma pairings written out: left to the compiler, they came out differently in the two kernels that
            // include this body, and the fused sweep must match the two launches bit for bit)
            const float ax = d1 * zx, ay = d1 * zy, ad = fmaf(d1, zd, d2 * zz);
#pragma unroll
            for (int c = 0; c < 3; ++c) wov[c][e] = fmaf(oc[c][3], ad, fmaf(oc[c][2], ay, fmaf(oc[c][0], t, oc[c][1] * ax)));
          }
          if (last) { dwv[0][e] = zq[0][e] * pxE + zq[1][e]; dwv[1][e] = zq[0][e] * pyE + zq[2][e]; }
          __builtin_amdgcn_sched_barrier(0);
        }
        // column sums of the four features at once (reduce_util.h); lane col == e of each half commits feature e
        commit(sg_db(HP, lE), o, sum_cols4<32>(zq[0][0], zq[0][1], zq[0][2], zq[0][3], lane));
        if (first) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            commit(sg_wout(HP, L) + c * HP, o, sum_cols4<32>(wov[c][0], wov[c][1], wov[c][2], wov[c][3], lane));
        }
        if (last) {
          commit(sg_w0x(HP, L), o, sum_cols4<32>(dwv[0][0], dwv[0][1], dwv[0][2], dwv[0][3], lane));
          commit(sg_w0y(HP, L), o, sum_cols4<32>(dwv[1][0], dwv[1][1], dwv[1][2], dwv[1][3], lane));
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!last) {
          const unsigned so = (unsigned)(((o - 4 * h) >> 2) + h) * PPL + col;
          u32x4 pk[3];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            if (park) split4(zq[p][0], zq[p][1], zq[p][2], zq[p][3], st[k][p][0], st[k][p][1]);
            pack24_plane(zq[p], p, pk);
            store24_planes(Zl, PLQ, so, p, pk);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      quarter(q);
      __syncthreads();
    }
    have_parked = !last && park;
  }
};
