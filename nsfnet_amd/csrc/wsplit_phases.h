// Phase bodies of the wide role-split sweeps (256 < hidden <= 448), written once for fwd_bf16_wsplit.hip and
// bwd_bf16_wsplit.hip (the schedule and the geometry: fwd_bf16_wsplit.hip).  A WSplitWave is one wave's register state -
// accumulators, parked block, weight ring, saved-activation quads in flight - with the K-region geometry and the phases
// that use it.  A kernel keeps its LDS layout, point stage or output-adjoint seeds, the S source of a dummy partner tile
// and its program; it hands the phases what differs as arguments (spill blocks, LDS rows) and as per-quarter callables.
//
// Every phase is force-inlined into a straight-line per-group program (split_phases.h).
//
// FF: the frozen sine first layer, as in split_phases.h.  The forward's E phase of layer 0 forms the a-streams by
// layer0_sine and stores THEM in layer 0's slot of S, in the 24-bit format (the 8-wave FF convention: dw_bf16_wide.hip
// takes the layer-1 A operand from that quad); the reverse sweep ends at E_1, run with park = false (bphase).
#pragma once
#include <type_traits>
#include "kernels.h"
#include "bf16_util.h"
#include "reduce_util.h"

template <int HP, int TERMS, bool FF = false>
struct WSplitWave {
  using XI = XImg<HP, 16>;
  typedef __attribute__((address_space(1))) u32x4 gu32x4;
  static constexpr int NB = HP / 32, MQ = (NB + 3) / 4, KS = HP / 16;
  static constexpr int LASTK = 128 * (MQ - 1);          // first feature of the last region
  static constexpr int LASTN = HP - LASTK;              // its width (32 .. 128)
  static constexpr bool FITS = XI::RSE - HP >= LASTN;   // room for the second copy of the last region
  static_assert(HP > 256 && HP <= 512 && FITS, "hidden widths whose last K region fits twice in the image rows");
  static constexpr int PPL = 16, COLS = 64, RING = 2;
  static constexpr int SQ = 2, NQD = 2 * MQ;            // saved-activation quads requested ahead / register quads per phase
  static constexpr size_t PLQ = (size_t)(HP / 4) * PPL; // f32x4 per plane of S / Z-bar
  // LDS behind the image (independent of TERMS).  Forward: per-wave output partials [group][wave][3 outputs x 4
  // streams][16 points], outputs [group][3][64], W_out and layer-0 rows [6][HP].  Reverse: output adjoints
  // [group][4][64] (3 used), the sink of the lanes that own no accumulator slot, the gradient accumulators.
  static constexpr size_t PART_F = (size_t)2 * 4 * 12 * 16, OUTV_F = (size_t)2 * 3 * 64;
  static constexpr size_t OADJ_F = (size_t)2 * 4 * 64, DUMMY_F = 64 * 8;
  static size_t fwd_bytes() { return XI::BYTES + (PART_F + OUTV_F + 6 * HP) * sizeof(float); }
  static size_t bwd_bytes(int L) { return XI::BYTES + (OADJ_F + DUMMY_F + (size_t)sg_total(HP, L)) * sizeof(float); }

  unsigned char* const X;                 // the shared K-region image
  const float* const P;                   // prepared parameters
  const float* const wout;                // [3][HP] rows of W_out
  const float* const w0;                  // [w0x | w0y | b0][HP] rows
  const int grp, w, lane0;                // group, wave in the group, lane
  const int mc = (NB - w + 3) / 4;        // feature blocks of this wave: 4 q + w, q < mc
  f32x16 acc[MQ][2];                      // [feature block of this wave][column block: streams 2 j, 2 j + 1]
  u32x2 st[2][4][2];                      // parked epilogue output of one block: [quad][stream][hi | lo]
  // weight-fragment ring [block][k-step % RING]; lives across phases (the first k-step of an M / G phase is requested
  // during the last quad of the E phase before it)
  u32x4 wh[MQ][RING], wl[MQ][RING];
  u32x4 sq[SQ + 1][3];                    // saved-activation quads in flight, 24-bit format (reverse sweep)

  __device__ __forceinline__ WSplitWave(unsigned char* X_, const float* P_, const float* wout_, const float* w0_, int grp_, int w_, int lane0_)
      : X(X_), P(P_), wout(wout_), w0(w0_), grp(grp_), w(w_), lane0(lane0_) {}

  // lane geometry, re-derived inside every phase from an opaque copy of the lane id (split_phases.h)
  __device__ __forceinline__ int phase_lane() const {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    return lane;
  }
  // lane (pp, hi, h) of quad k of block bq holds features quad_o .. quad_o + 3 of point pp
  __device__ __forceinline__ int quad_o(int bq, int k, int hi, int h) const { return 32 * (4 * bq + w) + 8 * (k + 2 * hi) + 4 * h; }
  // image chunk (8 k) of feature o: this group's copy of the last region sits behind the features
  __device__ __forceinline__ int img_chunk(int o) const { return (o >> 3) + ((o >= LASTK && grp) ? LASTN / 8 : 0); }
  // items of a reverse phase in processing order (the last block's two quads ride in quarters 0 and 1):
  //   quarter 0: (block 0, quad 0) (0, 1) (MQ-1, 0) | quarter 1: (1, 0) (1, 1) (MQ-1, 1) | quarter q >= 2: (q, 0) (q, 1) | last: none
  __device__ __forceinline__ static int item_bq(int i) { return i < 6 ? ((i % 3) == 2 ? MQ - 1 : i / 3) : 2 + (i - 6) / 2; }
  __device__ __forceinline__ static int item_k(int i) { return i < 6 ? ((i % 3) == 2 ? i / 3 : i % 3) : (i - 6) % 2; }

  // k-step s of the weight image at P + poff (prep_wf: W_l, forward; prep_wtf: W_l^T, reverse) into the ring
  __device__ __forceinline__ void wload(size_t poff, int s, int lane) {
    const gu32x4* const wf = reinterpret_cast<const gu32x4*>(pin_base(reinterpret_cast<const u32x4*>(P + poff)));
#pragma unroll
    for (int m = 0; m < MQ; ++m) {
      if (m == MQ - 1 && m >= mc) continue;            // (only the last block can be missing: mc >= MQ - 1)
      wh[m][s % RING] = (wf + (size_t)(4 * m + w) * KS * 64 + s * 64)[lane];
      if (TERMS == 3) wl[m][s % RING] = (wf + (size_t)(HP * HP / 8) + (size_t)(4 * m + w) * KS * 64 + s * 64)[lane];
    }
  }
  // hi / lo of stream p of quad k of block bq into the image
  __device__ __forceinline__ void img_put(int bq, int k, int p, int pp, int hi, int h, const u32x2& th, const u32x2& tl) {
    const int off = XI::chunk_off(pp, img_chunk(quad_o(bq, k, hi, 0))) + 8 * h;
    *reinterpret_cast<u32x2*>(X + p * XI::PLANE * 2 + off) = th;
    if (TERMS == 3) *reinterpret_cast<u32x2*>(X + XI::HALF * 2 + p * XI::PLANE * 2 + off) = tl;
  }
  // the parked quad k of block bq -> image
  __device__ __forceinline__ void dump_k(int bq, int k, int pp, int hi, int h) {
#pragma unroll
    for (int p = 0; p < 4; ++p) img_put(bq, k, p, pp, hi, h, st[k][p][0], st[k][p][1]);
  }
  // saved-activation quad of item i of the spill block Sl into the in-flight slot i % (SQ + 1)
  __device__ __forceinline__ void sload(const float* Sl, int i, int pp, int hi, int h) {
    if (item_bq(i) >= mc) return;                       // (uniform: this wave owns no block in the last region)
    const unsigned so = (unsigned)(quad_o(item_bq(i), item_k(i), hi, h) >> 2) * PPL + pp;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      sq[i % (SQ + 1)][k] = __builtin_bit_cast(u32x4, __builtin_nontemporal_load(pin_base(reinterpret_cast<const f32x4*>(Sl) + k * PLQ) + so));
  }
  // the four streams of a point into one lane: a 64-column block holds two streams in its lane halves
  __device__ __forceinline__ void swaps(int bq) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      auto s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[bq][0][r]), __float_as_uint(acc[bq][0][r + 8]), false, false);
      auto s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[bq][1][r]), __float_as_uint(acc[bq][1][r + 8]), false, false);
      acc[bq][0][r] = __uint_as_float(s01[0]); acc[bq][0][r + 8] = __uint_as_float(s01[1]);
      acc[bq][1][r] = __uint_as_float(s23[0]); acc[bq][1][r + 8] = __uint_as_float(s23[1]);
    }
  }
  __device__ __forceinline__ static void idle() {
#pragma unroll
    for (int q = 0; q < MQ; ++q) __syncthreads();
  }

  // ---------------- M / G phase: acc <- W_l x image (forward) or W_l^T x image (REV), region q in quarter q ----------------
  // PRE_S: the next E phase's first SQ saved-activation quads, from Snext, are requested in the last k-step, younger
  // than every weight request of this phase.
  template <bool REV, bool PRE_S>
  __device__ __forceinline__ void mphase(int l, const float* Snext) {
    const int lane = phase_lane(), col = lane & 31, h = lane >> 5, hi = col >> 4, pp = col & 15;
    const size_t poff = REV ? prep_wtf(HP, l) : prep_wf(HP, l);
    u32x4 bh[2], bo[2];
    auto bload = [&](int u) {                          // u = 2 s + j
      const int s = u >> 1, j = u & 1;
      const int off = XI::chunk_off(pp, img_chunk(16 * s) + h) + (2 * j + hi) * XI::PLANE * 2;
      bh[u & 1] = *reinterpret_cast<const u32x4*>(X + off);
      if (TERMS == 3) bo[u & 1] = *reinterpret_cast<const u32x4*>(X + XI::HALF * 2 + off);
    };
#pragma unroll
    for (int q = 0; q < MQ; ++q) {
      const int s0 = 8 * q, s1 = (8 * q + 8 < KS) ? 8 * q + 8 : KS;
      bload(2 * s0);
#pragma unroll
      for (int u = 2 * s0; u < 2 * s1; ++u) {
        const int s = u >> 1, j = u & 1;
        if (j == 0 && s + 1 < KS) wload(poff, s + 1, lane);
        if (PRE_S && s == KS - 1) sload(Snext, j, pp, hi, h);
        if (u + 1 < 2 * s1) bload(u + 1);
#pragma unroll
        for (int m = 0; m < MQ; ++m) {
          if (m == MQ - 1 && m >= mc) continue;
          if (s == 0) {
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[m][j] = TERMS == 3 ? mfma_bf16(wh[m][0], bo[u & 1], zero) : mfma_bf16(wh[m][0], bh[u & 1], zero);
            if (TERMS == 3) {
              acc[m][j] = mfma_bf16(wl[m][0], bh[u & 1], acc[m][j]);
              acc[m][j] = mfma_bf16(wh[m][0], bh[u & 1], acc[m][j]);
            }
          } else {
            if (TERMS == 3) {
              acc[m][j] = mfma_bf16(wh[m][s % RING], bo[u & 1], acc[m][j]);
              acc[m][j] = mfma_bf16(wl[m][s % RING], bh[u & 1], acc[m][j]);
            }
            acc[m][j] = mfma_bf16(wh[m][s % RING], bh[u & 1], acc[m][j]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);      // requests stay where they are written (one k-step / one step ahead)
      }
      __syncthreads();
    }
  }

  // ---------------- forward E phase: chain rule of layer lE ----------------
  // EK: 0 = layer 0 (pre-activations from the point (x, y) on the VALU), 1 = hidden layer 1..L-2, 2 = last hidden layer
  // (output layer folded into the per-wave partials partG, nothing written to the image).  S goes to the block Sl.
  // quarter(q): the kernel's work at the top of quarter q.
  template <int EK, class Quarter>
  __device__ __forceinline__ void fphase(int lE, int tileE, float* Sl, const float* x, const float* y, int n, float* partG, Quarter quarter) {
    constexpr bool last = EK == 2, first = EK == 0;
    const int lane = phase_lane(), col = lane & 31, h = lane >> 5, hi = col >> 4, pp = col & 15;
    const float* const bE = P + (first ? prep_b0(HP) : prep_b(HP, lE));      // (global: 160 KiB of LDS do not hold L x HP biases too)
    float po[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) po[c][s] = 0.f;
    float px = 0.f, py = 0.f;
    if (first) {
      const int pt = tileE * PPL + pp;
      px = pt < n ? x[pt] : 0.f; py = pt < n ? y[pt] : 0.f;
    }
    // chain rule of quad k of block bq: a-streams av, saved values sv
    auto compute = [&](int bq, int k, f32x4 (&av)[4], f32x4 (&sv)[4]) {
      const int o = quad_o(bq, k, hi, h);
      f32x4 b4, wx4, wy4;
      if (first) {
        wx4 = *reinterpret_cast<const f32x4*>(w0 + o); wy4 = *reinterpret_cast<const f32x4*>(w0 + HP + o);
        b4 = *reinterpret_cast<const f32x4*>(w0 + 2 * HP + o);
      } else {
        b4 = *reinterpret_cast<const f32x4*>(bE + o);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * k + e;
        float z, zx, zy, zd;
        if (first) {
          z = layer0_z(wx4[e], wy4[e], b4[e], px, py); zx = wx4[e]; zy = wy4[e]; zd = 0.f;
        } else {
          z = acc[bq][0][r] + b4[e]; zx = acc[bq][0][r + 8]; zy = acc[bq][1][r]; zd = acc[bq][1][r + 8];
        }
        if constexpr (FF && first) {      // the frozen sine layer: the a-streams by its one statement, saved as they are
          float f0, f1, f2, f3;
          layer0_sine(z, zx, zy, SinCosFast(), f0, f1, f2, f3);
          av[0][e] = f0; av[1][e] = f1; av[2][e] = f2; av[3][e] = f3;
          sv[0][e] = f0; sv[1][e] = f1; sv[2][e] = f2; sv[3][e] = f3;
        } else {
          const float t = fast_tanh(z);
          const float d1 = 1.f - t * t;
          const float d2 = -2.f * t * d1;
          // (zx zx + zy zy as one fmaf, in the pairing contraction chose before these bodies were shared: left to it, the
          // last block's quads now pair the other way - see bphase)
          av[0][e] = t; av[1][e] = d1 * zx; av[2][e] = d1 * zy; av[3][e] = d2 * fmaf(zx, zx, zy * zy) + d1 * zd;
          sv[0][e] = t; sv[1][e] = zx; sv[2][e] = zy; sv[3][e] = zd;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // hi/lo split of the a-streams (parked in st[k], or straight into the image: `direct`), output layer (last), S spill
    auto finish = [&](int bq, int k, f32x4 (&av)[4], f32x4 (&sv)[4], bool direct) {
      const int o = quad_o(bq, k, hi, h);
      const unsigned so = (unsigned)(o >> 2) * PPL + pp;
      u32x4 pk[3];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (!last) {
          if (direct) {
            u32x2 th, tl;
            split4(av[p][0], av[p][1], av[p][2], av[p][3], th, tl);
            img_put(bq, k, p, pp, hi, h, th, tl);
          } else {
            split4(av[p][0], av[p][1], av[p][2], av[p][3], st[k][p][0], st[k][p][1]);
          }
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const f32x4 wo = *reinterpret_cast<const f32x4*>(wout + c * HP + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) po[c][p] = fmaf(wo[e], av[p][e], po[c][p]);
          }
        }
        pack24_plane(sv[p], p, pk);
        store24_planes(Sl, PLQ, so, p, pk);
        if (last) asm volatile("" : "+v"(po[0][p]), "+v"(po[1][p]), "+v"(po[2][p]));
        __builtin_amdgcn_sched_barrier(0);
      }
    };
#pragma unroll
    for (int q = 0; q < MQ; ++q) {
      quarter(q);
      // Blocks 0 .. MQ - 2 (every wave owns them) ride in their own quarter.  The LAST block's two quads ride in quarters
      // 0 and 1 instead of a quarter of their own: its region has a per-group copy that nobody else touches during this
      // phase, so it can be written at any time - and the last quarter, where the M group has only the short last
      // region to multiply (2 k-steps at hidden 416), is left with the dump of block MQ - 2 alone.
      const bool mainb = q < MQ - 1;
      const bool prev = q > 0 && !last;                  // block q - 1 is parked and its region is free now
      const bool extra = q < 2 && mc == MQ;              // (uniform: this wave owns a block in the last region)
      if (mainb && !first) swaps(q);
      if (q == 0 && mc == MQ && !first) swaps(MQ - 1);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (!last && q == MQ - 1 && k == 1) wload(prep_wf(HP, lE + 1), 0, lane);      // first weight k-step of M_{lE+1}
        f32x4 av[4], sv[4];
        if (mainb) compute(q, k, av, sv);
        // block q - 1, parked in the previous quarter: quad k leaves its registers just before they are refilled
        if (prev) dump_k(q - 1, k, pp, hi, h);
        if (mainb) finish(q, k, av, sv, false);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (extra) {
        f32x4 av[4], sv[4];
        compute(MQ - 1, q, av, sv);
        finish(MQ - 1, q, av, sv, true);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (last && q == MQ - 1) {
        // the lanes (pp, hi, h) of a point hold different features: add the four of them (all publish the same value)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            float v = po[c][s];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            partG[(w * 12 + c * 4 + s) * 16 + pp] = v;
          }
      }
      __syncthreads();
    }
  }

  // ---------------- reverse E phase: tanh adjoint of layer lE ----------------
  // EK: 0 = last hidden layer L-1 (a-stream adjoints from the output adjoints oadj [output][64] on the VALU, dW_out),
  // 1 = layer L-2..1, 2 = layer 0 (dW_0; its saved activations recomputed from the point (pxE, pyE); nothing parked, no
  // spill).  Saved activations come from the block Sl (requested SQ quads ahead; all but EK 0's by the G phase before),
  // z-bar goes to the block Zl.  The column sums of the skinny gradients go into sgacc; the lanes that own no slot add
  // into sink[lane].  quarter(q): the kernel's work at the end of quarter q.
  // park = false (orthogonal to EK; the last phase of an FF reverse sweep, E_1 or for L = 2 the first phase itself): no
  // G phase follows, so z-bar is spilled to Zl as ever (dW reads it) but is neither split nor written to the image -
  // not parked, not dumped, not put into the group's copy of the last region - and no weight k-step is requested.  The
  // phase then touches no image, as EK 2 does, and keeps its MQ barriers.  An argument, not a template parameter
  // (split_phases.h).
  template <int EK, class Quarter>
  __device__ __forceinline__ void bphase(int lE, int L, const float* Sl, float* Zl, float pxE, float pyE, const float* oadj,
                                         float* sgacc, float* sink, Quarter quarter, bool park = true) {
    constexpr bool first = EK == 0, last = EK == 2;
    const int lane = phase_lane(), col = lane & 31, h = lane >> 5, hi = col >> 4, pp = col & 15;
    float oc[3][4];
    if (first) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) oc[c][s] = oadj[c * COLS + s * PPL + pp];
    }
    auto commit = [&](int base, int o4, float v) {        // lanes pp < 4 of each 16-lane row own feature o4 + pp (reduce_util.h)
      float* p = pp < 4 ? &sgacc[base + o4 + pp] : &sink[lane];
      lds_rmw_add(p, v);
    };
    if (!last && first) {      // (every other E phase follows a G phase, which has requested them)
#pragma unroll
      for (int qq = 0; qq < SQ; ++qq) sload(Sl, qq, pp, hi, h);
    }
    // item i = quad k of block bq: z-bar of its four features x four streams, skinny-gradient column sums
    auto compute = [&](int i, f32x4 (&zq)[4]) {
      const int bq = item_bq(i), k = item_k(i), o = quad_o(bq, k, hi, h);
      f32x4 sc[4];
      if (last) {
        // layer 0: recomputed as the forward computed it (stored too in this layout, but not read back here)
        layer0_saved(*reinterpret_cast<const f32x4*>(w0 + o), *reinterpret_cast<const f32x4*>(w0 + HP + o),
                     *reinterpret_cast<const f32x4*>(w0 + 2 * HP + o), pxE, pyE, TanhFast(), sc[0], sc[1], sc[2], sc[3]);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) sc[p] = unpack24_plane(sq[i % (SQ + 1)], p);
      }
      f32x4 wov[3], dwv[2], wo4[3];
      if (first) {
#pragma unroll
        for (int c = 0; c < 3; ++c) wo4[c] = *reinterpret_cast<const f32x4*>(wout + c * HP + o);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * k + e;
        float ga, gx, gy, gd;
        if (first) {      // adjoint of the last hidden layer's a-streams: rank-3 update from the output adjoints
          ga = wo4[0][e] * oc[0][0] + wo4[1][e] * oc[1][0] + wo4[2][e] * oc[2][0];
          gx = wo4[0][e] * oc[0][1] + wo4[1][e] * oc[1][1] + wo4[2][e] * oc[2][1];
          gy = wo4[0][e] * oc[0][2] + wo4[1][e] * oc[1][2] + wo4[2][e] * oc[2][2];
          gd = wo4[0][e] * oc[0][3] + wo4[1][e] * oc[1][3] + wo4[2][e] * oc[2][3];
        } else {
          ga = acc[bq][0][r]; gx = acc[bq][0][r + 8]; gy = acc[bq][1][r]; gd = acc[bq][1][r + 8];
        }
        const float t = sc[0][e], zx = sc[1][e], zy = sc[2][e], zd = sc[3][e];
        const float d1 = 1.f - t * t;
        const float d2 = -2.f * t * d1;
        const float d3 = -2.f * d1 * (1.f - 3.f * t * t);
        // zx zx + zy zy and zx gx + zy gy as explicit fmaf, in the pairings contraction chose before these bodies were
        // shared, so that the results stay bit for bit: the y product fused for the last block's quads at widths where
        // some waves own none of it (NB % 4 != 0) - both sums in layers L-2..1, zx zx + zy zy in layer L-1 - and the x
        // product fused everywhere else
        const bool yx = i < 6 && i % 3 == 2 && NB % 4 != 0 && !last;
        const float zz = yx ? fmaf(zy, zy, zx * zx) : fmaf(zx, zx, zy * zy);
        const float zg = yx && !first ? fmaf(zy, gy, zx * gx) : fmaf(zx, gx, zy * gy);
        zq[1][e] = d1 * gx + 2.f * d2 * zx * gd;
        zq[2][e] = d1 * gy + 2.f * d2 * zy * gd;
        zq[3][e] = d1 * gd;
        zq[0][e] = d1 * ga + d2 * zg + (d3 * zz + d2 * zd) * gd;
        if (first) {      // dWout[c][o] += sum_s oadj[c][s] * a_s[o]
          const float ax = d1 * zx, ay = d1 * zy, ad = d2 * zz + d1 * zd;
#pragma unroll
          for (int c = 0; c < 3; ++c) wov[c][e] = oc[c][0] * t + oc[c][1] * ax + oc[c][2] * ay + oc[c][3] * ad;
        }
        if (last) { dwv[0][e] = zq[0][e] * pxE + zq[1][e]; dwv[1][e] = zq[0][e] * pyE + zq[2][e]; }
        __builtin_amdgcn_sched_barrier(0);
      }
      // column sums over the 16 points of a lane row, four features at once (reduce_util.h)
      commit(sg_db(HP, lE), o, sum_cols4<16>(zq[0][0], zq[0][1], zq[0][2], zq[0][3], lane));
      if (first) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          commit(sg_wout(HP, L) + c * HP, o, sum_cols4<16>(wov[c][0], wov[c][1], wov[c][2], wov[c][3], lane));
      }
      if (last) {
        commit(sg_w0x(HP, L), o, sum_cols4<16>(dwv[0][0], dwv[0][1], dwv[0][2], dwv[0][3], lane));
        commit(sg_w0y(HP, L), o, sum_cols4<16>(dwv[1][0], dwv[1][1], dwv[1][2], dwv[1][3], lane));
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    // hi/lo split of z-bar (parked in st[k], or straight into this group's copy of the last region) and its 24-bit spill
    auto finish = [&](int i, f32x4 (&zq)[4], bool direct) {
      const int bq = item_bq(i), k = item_k(i), o = quad_o(bq, k, hi, h);
      const unsigned so = (unsigned)(o >> 2) * PPL + pp;
      u32x4 pk[3];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (park && direct) {
          u32x2 th, tl;
          split4(zq[p][0], zq[p][1], zq[p][2], zq[p][3], th, tl);
          img_put(bq, k, p, pp, hi, h, th, tl);
        } else if (park) {
          split4(zq[p][0], zq[p][1], zq[p][2], zq[p][3], st[k][p][0], st[k][p][1]);
        }
        pack24_plane(zq[p], p, pk);
        store24_planes(Zl, PLQ, so, p, pk);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
#pragma unroll
    for (int q = 0; q < MQ; ++q) {
      const bool mainb = q < MQ - 1;                     // blocks 0 .. MQ - 2 ride in their own quarter (every wave owns them)
      const bool prev = q > 0 && !last && park;          // block q - 1 is parked and its region is free now
      const bool extra = q < 2 && mc == MQ;              // the last block's quads ride in quarters 0 and 1 (uniform)
      const int i0 = q < 2 ? 3 * q : 6 + 2 * (q - 2);    // first item of this quarter
      if (mainb && !first) swaps(q);
      if (q == 0 && mc == MQ && !first) swaps(MQ - 1);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int i = i0 + k;
        if (mainb && !last && i + SQ < NQD) sload(Sl, i + SQ, pp, hi, h);
        // first weight k-step of the G phase that follows (its first MFMA would otherwise wait out an L2 round trip)
        if (!last && park && q == MQ - 1 && k == 1) wload(prep_wtf(HP, lE), 0, lane);
        f32x4 zq[4];
        if (mainb) compute(i, zq);
        // block q - 1, parked in the previous quarter: its region is free now; quad k leaves its registers before the refill
        if (prev) dump_k(q - 1, k, pp, hi, h);
        if (mainb && !last) finish(i, zq, false);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (q < 2) {
        const int i = i0 + 2;
        if (!last && i + SQ < NQD) sload(Sl, i + SQ, pp, hi, h);
        if (extra) {
          f32x4 zq[4];
          compute(i, zq);
          if (!last) finish(i, zq, true);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      quarter(q);
      __syncthreads();
    }
  }
};

// The supported widths (those whose last K region fits twice in the image rows), as dispatch_width's list; 480 and
// 512 keep the 8-wave kernels.
#define WSPLIT_WIDTHS 288, 320, 352, 384, 416, 448
