// Per-point stages shared by every forward kernel (fwd / fwd_wide / fwd_bf16 / fwd_bf16_wide).
// `outv` is the tile's output-layer result in LDS, [3 outputs][COLS] with column = stream * PPL + point in
// residual mode (PPL points x 4 streams) and column = point in value mode (COLS points).
#pragma once
#include "kernels.h"

// Hard wall conditions of the lid-driven unit cavity (include/nsfnet_pinn.h, "Hard boundary conditions"): the stages
// below, instantiated with HBC = true, run u = g + D N_u, v = D N_v on the net's streams N and pull the adjoints back
// through the transpose.  X, Y: the point in the unit cavity; D = 16 X(1-X) Y(1-Y) vanishes on the four walls; the lift
// g = l(X) Y^m carries the regularised lid l = 1 - cosh(r (X - 1/2)) / cosh(r / 2).  (x, dx, dy, dd) = value, d/dX, d/dY
// and Laplacian of D and of g.  Y^m by repeated multiplication (m = 1..8).
struct HardBcPoint { float D, Dx, Dy, Dd, g, gx, gy, gd; };
__device__ __forceinline__ HardBcPoint hard_bc_point(const HardBc& b, float xi, float eta) {
  const float X = (xi - b.x0) * b.inv_len, Y = (eta - b.y0) * b.inv_len;
  const float ax = X * (1.f - X), ay = Y * (1.f - Y);
  HardBcPoint h;
  h.D = 16.f * ax * ay;
  h.Dx = 16.f * (1.f - 2.f * X) * ay;
  h.Dy = 16.f * ax * (1.f - 2.f * Y);
  h.Dd = -32.f * (ax + ay);
  const float t = b.r * (X - 0.5f);
  const float ep = expf(t), em = expf(-t);           // cosh and sinh from one pair: even / odd in t to the bit, so l(0) = l(1)
  const float ch = 0.5f * (ep + em) * b.c, sh = 0.5f * (ep - em) * b.c;
  const float l = 1.f - ch, l1 = -b.r * sh, l2 = -b.r * b.r * ch;
  float pm2 = 1.f;                                   // Y^(m-2) (m = 1: its coefficient m (m-1) is zero)
  for (int i = 2; i < b.m; ++i) pm2 *= Y;
  const float pm1 = b.m >= 2 ? pm2 * Y : 1.f, pm = pm1 * Y;
  const float fm = (float)b.m;
  h.g = l * pm;
  h.gx = l1 * pm;
  h.gy = l * fm * pm1;
  h.gd = l2 * pm + l * (fm * (fm - 1.f)) * pm2;
  return h;
}
// c = lift + D N on the four streams (n, nx, ny, nd; physical derivatives) in place; lift: u carries g, v does not
__device__ __forceinline__ void hard_bc_apply(const HardBcPoint& h, bool lift, float& n, float& nx, float& ny, float& nd) {
  const float c = h.D * n, cx = h.Dx * n + h.D * nx, cy = h.Dy * n + h.D * ny;
  const float cd = h.Dd * n + 2.f * (h.Dx * nx + h.Dy * ny) + h.D * nd;
  n = lift ? h.g + c : c; nx = lift ? h.gx + cx : cx; ny = lift ? h.gy + cy : cy; nd = lift ? h.gd + cd : cd;
}
// the transpose: adjoints of (c, c_X, c_Y, Lap c) in, adjoints of the net's four streams out, in place
__device__ __forceinline__ void hard_bc_transpose(const HardBcPoint& h, float& a, float& ax, float& ay, float& ad) {
  const float n = h.D * a + h.Dx * ax + h.Dy * ay + h.Dd * ad;
  const float nx = h.D * ax + 2.f * h.Dx * ad, ny = h.D * ay + 2.f * h.Dy * ad;
  a = n; ax = nx; ay = ny; ad = h.D * ad;
}

// Residual mode: NS-residual assembly, lagged artificial viscosity, field planes, loss partial sums.
// Replaces NSFnet/pinn_solver.py:132-163,212-222 and ev-NSFnet/pinn_solver.py:290-342,372-428.
// PT = true (pseudo-time stepping, include/nsfnet_pinn.h "Pseudo-time stepping"): the loss sums 0..2 take the residuals
// q1 = eq1 + sigma (u - u*), q2 = eq2 + sigma (v - v*), q3 = eq3 + sigma_p (p - p*) against the anchor planes
// a.anchor = [3][npad]; the field planes keep the steady eq1..eq4, and eq4 is built on the steady eq1, eq2.
template <int PPL, int COLS, bool HBC = false, bool PT = false>
__device__ __forceinline__ void residual_point_stage(const FwdArgs& a, const float* outv, int tile, int tid, int npad,
                                                     float (&lsum)[4]) {
  if (tid >= PPL) return;
  const int pt = tile * PPL + tid;
  const bool m = pt < a.n;
  const float sc = a.scale, sc2 = a.scale * a.scale;
  float u = outv[tid], ux = outv[PPL + tid] * sc, uy = outv[2 * PPL + tid] * sc, ud = outv[3 * PPL + tid] * sc2;
  float v = outv[COLS + tid], vx = outv[COLS + PPL + tid] * sc, vy = outv[COLS + 2 * PPL + tid] * sc,
        vd = outv[COLS + 3 * PPL + tid] * sc2;
  float p = outv[2 * COLS + tid], pxx = outv[2 * COLS + PPL + tid] * sc, pyy = outv[2 * COLS + 2 * PPL + tid] * sc;
  if constexpr (HBC) {                    // from here on u and v are the constrained fields
    const HardBcPoint hb = hard_bc_point(a.hbc, m ? a.x[pt] : 0.f, m ? a.y[pt] : 0.f);
    hard_bc_apply(hb, true, u, ux, uy, ud);
    hard_bc_apply(hb, false, v, vx, vy, vd);
  }
  float vt = 0.f;
  float ev = (a.e && m) ? a.e[pt] : 0.f;
  if (a.vtm && m) {                       // ev-NSFnet/pinn_solver.py:327-334, kept on the device
    vt = fminf(a.vis_t0, a.vtm[pt]);
    a.vtm[pt] = a.alpha_evm * fabsf(ev);
  }
  if (a.vis_used && m) a.vis_used[pt] = vt;
  float nu = a.inv_re + vt;               // (viscosity identification: the kernel put *nu_dev there, resolve_viscosity)
  float eq1 = (u * ux + v * uy) + pxx - nu * ud;
  float eq2 = (u * vx + v * vy) + pyy - nu * vd;
  if (a.lap) {                            // viscosity identification (visc.hip): d eq1 / d nu = -Lap u, d eq2 / d nu = -Lap v,
    a.lap[pt] = ud; a.lap[(size_t)npad + pt] = vd;      // the physical Laplacians, padded like fld
  }
  float eq3 = ux + vy;
  float eq4 = a.e ? (eq1 * (u - 0.5f) + eq2 * (v - 0.5f)) - ev : 0.f;
  float* f = a.fld + pt;
  f[FLD_U * (size_t)npad] = u; f[FLD_V * (size_t)npad] = v;
  f[FLD_UX * (size_t)npad] = ux; f[FLD_UY * (size_t)npad] = uy;
  f[FLD_VX * (size_t)npad] = vx; f[FLD_VY * (size_t)npad] = vy;
  f[FLD_EQ1 * (size_t)npad] = eq1; f[FLD_EQ2 * (size_t)npad] = eq2;
  f[FLD_EQ3 * (size_t)npad] = eq3; f[FLD_EQ4 * (size_t)npad] = eq4;
  f[FLD_P * (size_t)npad] = p;
  if (m) {
    float ww = a.w ? a.w[pt] : 1.f;
    if constexpr (PT) {                   // (the planes above hold the steady residuals)
      const float* an = a.anchor + pt;
      eq1 += a.sigma * (u - an[0]);
      eq2 += a.sigma * (v - an[(size_t)npad]);
      eq3 += a.sigma_p * (p - an[2 * (size_t)npad]);
    }
    lsum[0] += ww * eq1 * eq1; lsum[1] += ww * eq2 * eq2;
    lsum[2] += ww * eq3 * eq3; lsum[3] += ww * eq4 * eq4;
  }
}

// Value mode: predictions, squared errors against (possibly masked) targets, output adjoints.
// Replaces the BC / supervised MSE terms (NSFnet/pinn_solver.py:199-207, ev-NSFnet/pinn_solver.py:399-411).
template <int COLS, int NT, bool HBC = false>
__device__ __forceinline__ void value_point_stage(const FwdArgs& a, const float* outv, int tile, int tid, int npad,
                                                  float (&lsum)[4]) {
  for (int idx = tid; idx < COLS; idx += NT) {
    const int pt = tile * COLS + idx;
    const bool m = pt < a.n;
    float hD = 1.f, hg = 0.f;
    if constexpr (HBC) {
      const HardBcPoint hb = hard_bc_point(a.hbc, m ? a.x[pt] : 0.f, m ? a.y[pt] : 0.f);
      hD = hb.D; hg = hb.g;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= a.n_out) break;
      float pv = outv[c * COLS + idx];
      if constexpr (HBC) {
        if (c < 2) pv = c == 0 ? hg + hD * pv : hD * pv;
      }
      if (a.pred[c] && m) a.pred[c][pt] = pv;
      float adj = 0.f;
      if (a.tgt[c] && m) {
        float t = a.tgt[c][pt];
        if (t == t && fabsf(t) <= 3.0e38f) {   // finite target (NaN pressure = masked, ev:405-410)
          float d = pv - t;
          lsum[c] += d * d;
          lsum[3] += (c == 2) ? 1.f : 0.f;     // count of valid pressure targets
          adj = a.coef[c] * d;
          if constexpr (HBC) {
            if (c < 2) adj *= hD;           // the net's output adjoint: the reverse sweep's value branch stays as it is
          }
        }
      }
      if (a.oadj) a.oadj[(size_t)c * npad + pt] = adj;
    }
  }
}

// Reverse sweep, start of a tile: adjoints of the three network outputs per MFMA column into LDS `oadjL`
// ([3 outputs][COLS], same column order as `outv` above), this lane's coordinates (px, py: the layer-0 weight
// gradient needs them), the output-bias gradient partials `dbo`, and d loss / d e (ebar).  The residual-mode
// seeds are the hand-derived derivatives of alpha_e * sum_k c_k w eq_k^2 with respect to (u, u_x, u_y, u_D, v, ...,
// p_x, p_y) - what loss.backward() (NSFnet/pinn_solver.py:252, ev-NSFnet/pinn_solver.py:469) propagates into the
// output layer; value mode copies the adjoints the value forward wrote.  px[j] / py[j]: point of column
// 32 j + col (value mode) or of column pp (residual mode, j = 0).
// PT = true (residual mode only): the seeds of the pseudo-time residuals q_k, rebuilt from the planes and the anchors;
// the field values take sigma g1, sigma g2 and - the one non-zero value adjoint of the pressure - sigma_p g3.
template <int PPL, int COLS, int NS, int NT, int NJ, bool HBC = false, bool PT = false>
__device__ __forceinline__ void output_adjoint_stage(const BwdArgs& a, int tile, int tid, int col, int pp, int npad,
                                                     float* oadjL, float (&dbo)[3], float (&px)[NJ], float (&py)[NJ]) {
  if (NS == 4) {
    const int ptc = tile * PPL + pp;
    px[0] = ptc < a.n ? a.x[ptc] : 0.f;
    py[0] = ptc < a.n ? a.y[ptc] : 0.f;
    if (tid < PPL) {
      const int pt = tile * PPL + tid;
      const bool m = pt < a.n;
      const float* f = a.fld + pt;
      float u = f[FLD_U * (size_t)npad], v = f[FLD_V * (size_t)npad];
      float ux = f[FLD_UX * (size_t)npad], uy = f[FLD_UY * (size_t)npad];
      float vx = f[FLD_VX * (size_t)npad], vy = f[FLD_VY * (size_t)npad];
      float eq1 = f[FLD_EQ1 * (size_t)npad], eq2 = f[FLD_EQ2 * (size_t)npad];
      float eq3 = f[FLD_EQ3 * (size_t)npad], eq4 = f[FLD_EQ4 * (size_t)npad];
      float ww = m ? (a.w ? a.w[pt] : 1.f) : 0.f;
      float q1 = eq1, q2 = eq2, q3 = eq3;
      if constexpr (PT) {
        if (m) {
          const float* an = a.anchor + pt;
          q1 += a.sigma * (u - an[0]);
          q2 += a.sigma * (v - an[(size_t)npad]);
          q3 += a.sigma_p * (f[FLD_P * (size_t)npad] - an[2 * (size_t)npad]);
        }
      }
      float g1 = a.coef_eq[0] * ww * q1, g2 = a.coef_eq[1] * ww * q2, g3 = a.coef_eq[2] * ww * q3;
      float g4 = a.e ? a.coef_eq[3] * ww * eq4 : 0.f;
      float r1 = g1 + g4 * (u - 0.5f), r2 = g2 + g4 * (v - 0.5f), r3 = g3;
      float nu = a.inv_re + ((a.vis_used && m) ? a.vis_used[pt] : 0.f);
      const float sc = a.scale, sc2 = a.scale * a.scale;
      float au = r1 * ux + r2 * vx + g4 * eq1;
      float av = r1 * uy + r2 * vy + g4 * eq2;
      float ap = 0.f;
      if constexpr (PT) { au += a.sigma * g1; av += a.sigma * g2; ap = a.sigma_p * g3; }
      if constexpr (HBC) {                  // the planes hold the constrained fields: their adjoints, pulled back to the net's
        const HardBcPoint hb = hard_bc_point(a.hbc, m ? a.x[pt] : 0.f, m ? a.y[pt] : 0.f);
        float aux = r1 * u + r3, auy = r1 * v, aud = -nu * r1;
        float avx = r2 * u, avy = r2 * v + r3, avd = -nu * r2;
        hard_bc_transpose(hb, au, aux, auy, aud);
        hard_bc_transpose(hb, av, avx, avy, avd);
        oadjL[0 * COLS + 0 * PPL + tid] = au;
        oadjL[0 * COLS + 1 * PPL + tid] = aux * sc;
        oadjL[0 * COLS + 2 * PPL + tid] = auy * sc;
        oadjL[0 * COLS + 3 * PPL + tid] = aud * sc2;
        oadjL[1 * COLS + 0 * PPL + tid] = av;
        oadjL[1 * COLS + 1 * PPL + tid] = avx * sc;
        oadjL[1 * COLS + 2 * PPL + tid] = avy * sc;
        oadjL[1 * COLS + 3 * PPL + tid] = avd * sc2;
      } else {
        oadjL[0 * COLS + 0 * PPL + tid] = au;
        oadjL[0 * COLS + 1 * PPL + tid] = (r1 * u + r3) * sc;
        oadjL[0 * COLS + 2 * PPL + tid] = (r1 * v) * sc;
        oadjL[0 * COLS + 3 * PPL + tid] = -nu * r1 * sc2;
        oadjL[1 * COLS + 0 * PPL + tid] = av;
        oadjL[1 * COLS + 1 * PPL + tid] = (r2 * u) * sc;
        oadjL[1 * COLS + 2 * PPL + tid] = (r2 * v + r3) * sc;
        oadjL[1 * COLS + 3 * PPL + tid] = -nu * r2 * sc2;
      }
      oadjL[2 * COLS + 0 * PPL + tid] = ap;
      oadjL[2 * COLS + 1 * PPL + tid] = r1 * sc;
      oadjL[2 * COLS + 2 * PPL + tid] = r2 * sc;
      oadjL[2 * COLS + 3 * PPL + tid] = 0.f;
      if (a.ebar && m) a.ebar[pt] = -g4;
      dbo[0] += au; dbo[1] += av;
      if constexpr (PT) dbo[2] += ap;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int pt = tile * COLS + 32 * j + col;
      px[j] = pt < a.n ? a.x[pt] : 0.f;
      py[j] = pt < a.n ? a.y[pt] : 0.f;
    }
    for (int idx = tid; idx < 3 * COLS; idx += NT) {
      int c3 = idx / COLS, cc = idx % COLS;
      int pt = tile * COLS + cc;
      float v = (c3 < a.n_out && pt < a.n) ? a.oadj[(size_t)c3 * npad + pt] : 0.f;
      oadjL[idx] = v;
      if (c3 == 0) dbo[0] += v; else if (c3 == 1) dbo[1] += v; else dbo[2] += v;
    }
  }
}
