// Internal kernel argument blocks and launchers (gfx950).  Not part of the C ABI;
// the exported surface is include/nsfnet_pinn.h.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "fixed_fold.h"
#include "launch_dispatch.h"
#include "layout.h"
#include "spill.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifdef __HIPCC__
typedef __attribute__((address_space(1))) f32x4 gf32x4;
// A uniform (tile, layer, plane) base pinned to scalar registers: lane addresses then cost ONE VALU (base +
// 32-bit offset) instead of a 64-bit add pair per plane - the epilogues pay full issue time for every VALU.
__device__ __forceinline__ gf32x4* pin_base(const void* q) {
  const unsigned long long b = (unsigned long long)q;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  return (gf32x4*)(((unsigned long long)hi << 32) | lo);
}
// Viscosity identification (visc.hip): once per residual kernel, before anything reads a.inv_re - that is before the
// tile loop AND before a prologue that already runs a point stage (the role-split reverse sweeps build their first
// tile's output adjoints ahead of the loop).  It is the kernel's first statement, except in the four wide kernels whose
// register allocation that place disturbed: fwd_wide, fwd_bf16_wide and bwd_bf16_wide call it right
// before their tile loop, bwd_bf16_wsplit right before its prologue's seeds.  Where the plan carries a trainable
// viscosity (FwdArgs / BwdArgs::nu_dev), the kernel's own copy of the argument block gets *nu_dev as its inv_re, so the
// per-point stages (point_stage.h, fwdbwd_bf16_split.hip) form nu = a.inv_re + vis_t as they always did and the tile
// loops carry no new state.  Only another launch ever writes *nu_dev, so it is read through the constant address
// space: one scalar load per workgroup, no vector register.
template <class Args>
__device__ __forceinline__ void resolve_viscosity(Args& a) {
  typedef const __attribute__((address_space(4))) float cfloat;
  if (a.nu_dev) a.inv_re = *(cfloat*)(unsigned long long)a.nu_dev;
}
// The host tail of every sweep and dW launcher.  configure != 0 (pinn_plan_create's configure pass): launch nothing,
// raise the kernel's dynamic-LDS limit on the current device.  Otherwise launch.  Returns 0 or -(the HIP error).
template <typename... Params, typename... Args>
static int launch_or_configure(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t s, int configure,
                               const Args&... args) {
  if (configure)
    return -(int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, PINN_LDS_MAX);
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  return -(int)hipGetLastError();
}
#endif

// Field planes written by the residual forward and read by the backward
// (plane stride = padded point count).
enum { FLD_U = 0, FLD_V, FLD_UX, FLD_UY, FLD_VX, FLD_VY, FLD_EQ1, FLD_EQ2, FLD_EQ3, FLD_EQ4, FLD_P, FLD_COUNT };

// Hard wall conditions of the lid-driven unit cavity (include/nsfnet_pinn.h pinn_hard_bc_t; point_stage.h): kind 0 = none,
// m = lift_power, r = lid_sharpness, c = 1 / cosh(r / 2) computed on the host in double.
struct HardBc { int kind, m; float x0, y0, inv_len, r, c; };

struct FwdArgs {
  const float* x; const float* y;
  int n;            // real points
  int ntiles;       // tiles of 32 (residual) / 128 (value) points
  int L;            // hidden layers
  int n_out;        // 3 (u,v,p) or 1 (e)
  const float* prep;
  float* S;         // saved (t, z_x, z_y, z_D) per (tile, layer) block (spill.h) or null
  // residual mode (4 streams)
  float* fld;       // [FLD_COUNT][npad]
  const float* e;   // entropy-net output per point or null
  const float* w;   // per-point weights or null
  float* vtm;       // vis_t_minus state (in/out) or null
  float* vis_used;  // artificial viscosity used this step (out) or null
  float inv_re, vis_t0, alpha_evm, scale;
  union {
    struct {               // value mode (1 stream)
      float* pred[3];        // optional prediction planes
      const float* tgt[3];   // optional targets (NaN target = masked)
      float* oadj;           // [4][npad] output adjoints (written when non-null)
      float coef[3];         // oadj_c = coef[c] * (pred_c - tgt_c)
    };
    // Pseudo-time stepping (residual mode; 8-wave, role-split and fused families; point_stage.h), in the bytes residual mode leaves unused:
    // the block keeps its size and every other member its offset, so the kernels that do not read these are
    // compiled as before.  The launchers read ptime in residual mode only (NS == 4).
    struct {
      const float* anchor;   // [3][npad] anchors u*, v*, p*
      float sigma, sigma_p;  // 1 / dtau of the momentum equations, of the continuity equation
      int ptime;             // != 0: launch the pseudo-time variant
      // Viscosity identification (residual mode, every family; point_stage.h, visc.hip), behind ptime in the same bytes:
      const float* nu_dev;   // one fp32 in device memory read in place of inv_re (the trainable 1 / Re), or null
      float* lap;            // [2][npad] planes Lap u, Lap v (physical, of the constrained fields on a constrained plan), or null
      const float* cap_dev;  // Reynolds-number continuation: one fp32 read in place of vis_t0 (only beside nu_dev), or null
    };
  };
  float* partials;       // [grid][PINN_NLOSS]
  int stagger;           // start offset unit (x 4096 cycles x (block*5 mod 8)); 0 = off
  int configure;         // 1: do not launch, only raise the kernel's dynamic-LDS limit (pinn_plan_create)
  Spill spill;           // the plan's S / Z-bar format (spill.h)
  HardBc hbc;            // kind != 0: the 8-wave, role-split and fused families launch their constrained instantiation
  int ff;                // != 0: the net's first layer is the frozen sine layer (spill_io.h layer0_sine); the 8-wave families
                         // launch their FF instantiation, which saves layer 0's a-streams.  Never with hbc.kind or ptime.
};

#ifdef __HIPCC__
// Reynolds-number continuation (visc_sched.hip): resolve_viscosity of a forward argument block also takes the cap of
// the entropy viscosity, vis_t0, from device memory where the plan carries one (cap_dev, only ever beside nu_dev).
// Being an overload it runs at the place the call already has in every forward kernel and in the fused one: one more
// scalar load per workgroup.  The reverse sweeps read the stored vis_used plane and need nothing.
__device__ __forceinline__ void resolve_viscosity(FwdArgs& a) {
  typedef const __attribute__((address_space(4))) float cfloat;
  if (a.nu_dev) {
    a.inv_re = *(cfloat*)(unsigned long long)a.nu_dev;
    if (a.cap_dev) a.vis_t0 = *(cfloat*)(unsigned long long)a.cap_dev;
  }
}
#endif

struct BwdArgs {
  const float* x; const float* y;
  int n, ntiles, L, n_out;
  const float* prep;
  const float* S;
  float* Zb;             // z-adjoints per (tile, layer) block (layers 1..L-1 used)
  // residual mode
  const float* fld; const float* e; const float* w; const float* vis_used;
  float coef_eq[4];      // 2*alpha_e*c_k/N_total
  float inv_re, scale;
  float* ebar;           // d loss / d e per point (out) or null
  // value mode
  const float* oadj;     // [4][npad]
  float* sg;             // [grid][sg_total]
  int configure;         // see FwdArgs
  Spill spill;           // see FwdArgs
  HardBc hbc;            // see FwdArgs (residual mode; value mode takes adjoints that carry D already)
  // pseudo-time stepping (residual mode; 8-wave, role-split and fused families; point_stage.h): ptime != 0 launches the variant
  int ptime;
  const float* anchor;   // [3][npad] anchors u*, v*, p*
  float sigma, sigma_p;  // 1 / dtau of the momentum equations, of the continuity equation
  int ff;                // != 0 (residual mode): the net's first layer is the frozen sine layer.  The role-split and fused
                         // families launch their FF instantiation, whose sweep ends at layer 1; the 8-wave families do not read it.
  const float* nu_dev;   // see FwdArgs (residual mode; last, so that no other member moves)
};

struct DwArgs {
  const float* S; const float* Zb;
  int ntiles, L, groups;
  float* slabs;          // [(L-1)][groups][HP*HP]
  int configure;         // see FwdArgs
  // where the plan does not store layer 0 (Spill::skip0), the layer-1 workgroups recompute its activations: the
  // points, the prepared parameters (w0x | w0y | b0 lead them) and n
  const float* x; const float* y; const float* prep; int n;
  Spill spill;           // see FwdArgs
  int ff;                // != 0 (residual mode): layer 0's stored quad holds its a-streams; the layer-1 workgroups run the
                         // instantiation that takes the A operand straight from it (see FwdArgs)
};

struct ReduceSrc { const float* slabs; int groups; const float* sg; int nwg; };
struct ReduceArgs {
  ReduceSrc src[4]; int nsrc;
  int H, HP, L, n_out;
  float* grads; int accumulate;
  int frozen;            // the first `frozen` flat parameters are not trained (a frozen sine first layer: 3 H): their entries
                         // are written as +0.0 whatever the sources hold and whether or not the call accumulates
};

// Where flat parameter p (state_dict order) finds its partials: a row of the dW slabs of layer `layer` (>= 1) at
// slab_off, or entry sgi of the per-workgroup skinny accumulators (layer < 0).
struct ReduceLoc { int sgi; int layer; size_t slab_off; };
__device__ __forceinline__ ReduceLoc reduce_locate(size_t p, int H, int HP, int L, int n_out) {
  ReduceLoc r{-1, -1, 0};
  if (p < (size_t)2 * H) {
    int o = (int)(p / 2), j = (int)(p % 2);
    r.sgi = (j == 0 ? sg_w0x(HP, L) : sg_w0y(HP, L)) + o;
  } else if (p < (size_t)3 * H) {
    r.sgi = sg_db(HP, 0) + (int)(p - 2 * H);
  } else if (p < flat_w(H, L)) {
    size_t rel = p - (size_t)3 * H;
    size_t per = (size_t)H * H + H;
    int l = 1 + (int)(rel / per);
    size_t q = rel % per;
    if (q < (size_t)H * H) { r.layer = l; r.slab_off = (q / H) * HP + (q % H); }
    else r.sgi = sg_db(HP, l) + (int)(q - (size_t)H * H);
  } else {
    size_t q = p - flat_w(H, L);
    if (q < (size_t)n_out * H) r.sgi = sg_wout(HP, L) + (int)(q / H) * HP + (int)(q % H);
    else r.sgi = sg_bout(HP, L) + (int)(q - (size_t)n_out * H);
  }
  return r;
}
// s + the partials of one source that wave w of 8 sums (its groups / workgroups w, w+8, ..., 4 loads in flight),
// added one by one in that order: the fixed per-wave order of the gradient assembly.
__device__ __forceinline__ double reduce_source_add(double s, const ReduceSrc& src, const ReduceLoc& loc, int HP,
                                                    size_t SG, int w) {
  const float* base; size_t stride; int n;
  if (loc.layer >= 0) { base = src.slabs + (size_t)(loc.layer - 1) * src.groups * HP * HP + loc.slab_off; stride = (size_t)HP * HP; n = src.groups; }
  else { base = src.sg + loc.sgi; stride = SG; n = src.nwg; }
  int g = w;
  for (; g + 24 < n; g += 32) {
    float v0 = base[(size_t)g * stride], v1 = base[(size_t)(g + 8) * stride];
    float v2 = base[(size_t)(g + 16) * stride], v3 = base[(size_t)(g + 24) * stride];
    s += (double)v0; s += (double)v1; s += (double)v2; s += (double)v3;
  }
  for (; g < n; g += 8) s += (double)base[(size_t)g * stride];
  return s;
}

// Term-split assembly (balance.hip): the sources in three consecutive groups (collocation | boundary | supervised),
// each group summed like ReduceArgs into its own vector.  out[t] == nullptr: group t is not written (nsrc[t] must be
// 0); nsrc[t] == 0 with out[t] given writes zeros (or leaves out[t] as it is where accumulating).  acc_mask bit t: add
// to out[t].  partials != nullptr: per workgroup b, partials[6 b + 2 t] = max|out[t]| (NaN-propagating) and
// [6 b + 2 t + 1] = sum|out[t]| in fp64 over its 64 parameters, of the values written (0 for an unwritten group).
// gram != nullptr (confgrad.hip): per workgroup b, gram[6 b + c] = the fp64 dot products rr, bb, ss, rb, rs, bs over
// its 64 parameters of the values written (r, b, s = out[0..2]; 0 for an unwritten group).
struct TermReduceArgs {
  ReduceSrc src[4]; int nsrc[3];
  int H, HP, L, n_out;
  float* out[3]; int acc_mask;
  double* partials;
  double* gram;
  int frozen;            // see ReduceArgs; partials and gram see the zeros
};

// The six dot products of the 64 (r, b, s) a full wave holds, one triple per lane: exact fp64 products of the fp32
// values, each summed by wave_fold (fixed_fold.h); lane 0 writes out[0..5] = rr bb ss rb rs bs.
__device__ __forceinline__ void wave_gram(float r, float b, float s, int lane, double* __restrict__ out) {
  const double dr = r, db = b, ds = s;
  double q[6] = {__dmul_rn(dr, dr), __dmul_rn(db, db), __dmul_rn(ds, ds),
                 __dmul_rn(dr, db), __dmul_rn(dr, ds), __dmul_rn(db, ds)};
#pragma unroll
  for (int c = 0; c < 6; ++c) q[c] = wave_fold<FoldSum>(q[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) out[c] = q[c];
  }
}

int launch_fwd(int HP, int NS, const FwdArgs& a, int grid, hipStream_t s);
int launch_bwd(int HP, int NS, const BwdArgs& a, int grid, hipStream_t s);
int launch_dw(int HP, int NS, const DwArgs& a, hipStream_t s);
size_t fwd_lds_bytes(int HP);
size_t bwd_lds_bytes(int HP, int L);
size_t dw_lds_bytes(int HP);
int dw_threads(int HP);

int launch_prep(const float* params, float* prep, int H, int HP, int L, int n_out, int prec_fwd, int prec_bwd,
                hipStream_t s);
// wide nets (256 < HP <= 512): 64-column tiles, fp32 MFMA only
int launch_fwd_wide(int HP, int NS, const FwdArgs& a, int grid, hipStream_t s);
int launch_bwd_wide(int HP, int NS, const BwdArgs& a, int grid, hipStream_t s);
int launch_dw_wide(int HP, int NS, const DwArgs& a, hipStream_t s);
size_t fwd_wide_lds_bytes(int HP);
size_t bwd_wide_lds_bytes(int HP, int L);
size_t dw_wide_lds_bytes();
// bf16 MFMA variants (terms = 3: bf16x3 split, terms = 1: plain bf16)
// cols = 128 (32-point tiles) or 64 (16-point tiles, HP 128/256 only)
int launch_fwd_bf16(int HP, int NS, int terms, int cols, const FwdArgs& a, int grid, hipStream_t s);
int launch_bwd_bf16(int HP, int NS, int terms, int cols, const BwdArgs& a, int grid, hipStream_t s);
int launch_dw_bf16(int HP, int NS, int terms, int cols, const DwArgs& a, hipStream_t s);
size_t fwd_bf16_lds_bytes(int HP, int L, int cols);
size_t bwd_bf16_lds_bytes(int HP, int L, int cols);
size_t dw_bf16_lds_bytes(int HP);
// hidden > 256: 64-column tiles, two 32-feature blocks per wave (fwd_bf16_wide.hip / bwd_bf16_wide.hip)
int launch_fwd_bf16_wide(int HP, int NS, int terms, const FwdArgs& a, int grid, hipStream_t s);
int launch_bwd_bf16_wide(int HP, int NS, int terms, const BwdArgs& a, int grid, hipStream_t s);
int launch_dw_bf16_wide(int HP, int NS, int terms, const DwArgs& a, hipStream_t s);
size_t dw_bf16_wide_lds_bytes();
size_t fwd_bf16_wide_lds_bytes(int HP, int L);
size_t bwd_bf16_wide_lds_bytes(int HP, int L);
// one wave per SIMD, two tiles in flight, chain rule in the MFMA shadow (fwd_bf16_pipe.hip): HP = 256, residual mode
int launch_fwd_pipe(int HP, int terms, const FwdArgs& a, int grid, hipStream_t s);
size_t fwd_pipe_lds_bytes(int HP, int L);
// two wave groups in opposite phases (fwd_bf16_split.hip): HP = 256, residual mode
int launch_fwd_split(int HP, int terms, const FwdArgs& a, int grid, hipStream_t s);
size_t fwd_split_lds_bytes(int HP, int L);
int launch_bwd_split(int HP, int terms, const BwdArgs& a, int grid, hipStream_t s);
size_t bwd_split_lds_bytes(int HP, int L);
// the two role-split sweeps of each tile in one kernel (fwdbwd_bf16_split.hip): residual mode, MSE seeds
int launch_fwdbwd_split(int HP, int terms, const FwdArgs& fa, const BwdArgs& a, int grid, hipStream_t s);
size_t fwdbwd_split_lds_bytes(int HP, int L);
int launch_bwd_pipe(int HP, int terms, const BwdArgs& a, int grid, hipStream_t s);
size_t bwd_pipe_lds_bytes(int HP, int L);
// wide nets (256 < HP <= 448), residual mode, 24-bit spill: the role-split schedule at 64-column tiles (fwd_bf16_wsplit.hip)
int launch_fwd_wsplit(int HP, int terms, const FwdArgs& a, int grid, hipStream_t s);
size_t fwd_wsplit_lds_bytes(int HP);
int launch_bwd_wsplit(int HP, int terms, const BwdArgs& a, int grid, hipStream_t s);
size_t bwd_wsplit_lds_bytes(int HP, int L);
int launch_reduce(const ReduceArgs& a, hipStream_t s);
int launch_loss_sums(const float* partials, int nparts, float* out, hipStream_t s);
int launch_adam_dev(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2,
                    float eps, long long* step_counter, hipStream_t s);
int launch_adam(float* p, const float* g, float* m, float* v, long n, float step_size, float b1, float b2,
                float eps, float bc2_sqrt, hipStream_t s);
// residual-based resampling of the collocation points (resample.hip)
size_t resample_scratch_bytes(long n_pool);
int launch_resample_select(long n, const float* fields, long npad, double w4, double k, double c, double u, long m,
                           void* scratch, long long* out, hipStream_t s);
int launch_resample_gather(const long long* idx, long lo, long hi, long n_pool, const float* sx, const float* sy,
                           const float* sw, const float* sv, float* dx, float* dy, float* dw, float* dv, void* scratch,
                           double* w_sum, hipStream_t s);
// L-BFGS direction by the compact representation (lbfgs.hip)
size_t lbfgs_workspace_bytes(long n, long m);
int launch_lbfgs_reset(void* ws, long n, long m, hipStream_t s);
int launch_lbfgs_direction(void* ws, long n, long m, const float* g, float t_prev, float* d, double* result,
                           hipStream_t s);
int launch_lbfgs_probe(void* ws, long n, long m, const float* g, const float* d, double* result, hipStream_t s);
// adaptive loss-weight balancing (balance.hip)
long balance_blocks(long n);
int launch_reduce_terms(const TermReduceArgs& a, hipStream_t s);
int launch_balance_stats(const float* v0, const float* v1, const float* v2, long n, double* partials, hipStream_t s);
int launch_balance_update(const double* partials, long n, int terms, double beta, float* lam, double* record,
                          hipStream_t s);
int launch_balance_combine(float* g, const float* gr, const float* gb, const float* gs, const float* lam, long n,
                           hipStream_t s);
// conflict-free combination of the per-term gradients (confgrad.hip); partials: balance_blocks(n) * 6 doubles
int launch_confgrad_gram(const float* v0, const float* v1, const float* v2, long n, double* partials, hipStream_t s);
int launch_confgrad_coef(const double* partials, long n, int nterms, float* coef, double* record, hipStream_t s);
int launch_confgrad_combine(float* g, const float* gr, const float* gb, const float* gs, const float* coef, long n,
                            hipStream_t s);
// stochastic mini-batching of the collocation term (batch.hip)
struct BatchDrawArgs {
  long n, b;                               // store points, batch points (1 <= b <= n)
  unsigned seed, rank;                     // Philox key
  long long* counter;                      // [draw counter t, ticket of the workgroups done]
  const float *sx, *sy, *sw, *sv;          // store x, y, w, vis_t_minus (sw / sv NULL: absent)
  float *dx, *dy, *dw, *dv;                // batch buffers
  long long* idx;                          // [b] drawn store indices
};
int launch_batch_draw(const BatchDrawArgs& a, hipStream_t s);
int launch_batch_scatter(const long long* idx, long b, long n, const float* src, float* dst, hipStream_t s);
// residual-based attention weights on the collocation points (rba.hip)
struct RbaApplyArgs {
  long n, npad, n_store;                   // points of the evaluation, its plane stride, points of the store
  const float* fld;                        // [FLD_COUNT][npad] field planes of the evaluation
  double w4, gamma, eta;
  const long long* idx;                    // [n] store index of evaluation point j (NULL: identity)
  const float* s;                          // [n_store] static weights (NULL: 1)
  float *lam, *w;                          // [n_store] attention multipliers, effective weights
  double *scratch, *record;
};
long rba_blocks(long n);
size_t rba_scratch_bytes(long n);
int launch_rba_stats(long n, const float* fld, long npad, double w4, double* scratch, hipStream_t s);
int launch_rba_apply(const RbaApplyArgs& a, hipStream_t s);
int launch_rba_fill(long n, double init, const float* sw, float* lam, float* w, hipStream_t s);
// validation error on the device and the best-weights snapshot (validate.hip)
constexpr int VAL_RECORD = 8, VAL_STATE = 8;
struct ValStatsArgs {
  const float* pred[3];                    // prediction planes u^, v^, p^ ([2] NULL: no pressure), rows of ceil4(n) floats
  const float* tgt[3];                     // target planes, same layout (a NaN target masks the point for that channel)
  long n, capacity;                        // points; rows of the history ring
  int metric;                              // 0 uv, 1 u, 2 v, 3 p, 4 p0
  double t, every;                         // t < 0: t = (cadence records + 1) * every, from the state
  double *scratch, *state, *ring;
};
struct ValKeepArgs {
  const float* src[2];
  float* dst[2];
  long n[2];
  const double* state;
};
// pseudo-time stepping: the per-update record and anchor refresh (ptime.hip)
constexpr int PTIME_RECORD = 8;
struct PtimeArgs {
  long n, npad;                            // points; plane stride of fld and of anchor
  const float* fld;                        // [FLD_COUNT][npad] field planes of the last evaluation
  const float* w;                          // [n] weights (NULL: 1)
  float* anchor;                           // [3][npad] u*, v*, p*
  double every; int force;                 // refresh when record[6] + 1 >= every, or when force != 0
  double *scratch, *record;
};
size_t ptime_scratch_bytes(long n);
int launch_ptime_advance(const PtimeArgs& a, hipStream_t s);
// convergence monitor: the vis_t statistics of an evaluation and the per-update observation (monitor.hip)
constexpr int MON_RECORD = 12, MON_STATE = 16, MON_INFO = 4;
constexpr int MON_STOP_PLATEAU = 1, MON_STOP_RE_EFF = 2, MON_STOP_NONFINITE = 4;
struct MonVisArgs {
  long n;                                  // local entries of the plane
  const float* vis_t;                      // [n], 16-byte aligned
  float vis_t0;                            // the cap: entries >= vis_t0 are counted
  float* sum_out;                          // one fp32 slot of the loss-sum block
  double *info, *scratch;                  // [MON_INFO] per-rank words; scratch
};
struct MonObserveArgs {
  const float *eq, *bc, *sup;              // the exchanged loss-sum blocks (PINN_NLOSS floats each) of the evaluation that
                                           // produced the update: eq[0..3] sum w eq_k^2, eq[4] sum vis_t; bc[0..1]; sup[0..2] (NULL: none)
  const float* lam;                        // [2] balancing weights (lambda_b, lambda_s) on the device, or NULL: alpha_b, alpha_s
  double alpha_b, alpha_s, alpha_e, w4;
  double n_eq, n_b, n_s, n_p, Re;          // the normalisers (n_s / n_p 0: that part is absent)
  long every, window, patience, min_updates, capacity;
  int quantity, ev, plateau_on, re_on;     // quantity: 0 loss, 1 loss_e, 2 loss_b; ev: eq4 and vis_t take part
  double min_rel, re_tol;
  double *state, *ring;                    // [MON_STATE]; [capacity][MON_RECORD]
};
size_t monitor_scratch_bytes();
int launch_monitor_vis_stats(const MonVisArgs& a, hipStream_t s);
int launch_monitor_observe(const MonObserveArgs& a, hipStream_t s);
// viscosity identification: d loss / d nu of an evaluation and the update of theta = ln nu (visc.hip)
constexpr int VISC_STATE = 8;
struct ViscGradArgs {
  long n, npad;                            // points; plane stride of fld and of lap
  const float* fld;                        // [FLD_COUNT][npad] field planes of the evaluation
  const float* lap;                        // [2][npad] Lap u, Lap v of the same evaluation
  const float* w;                          // [n] weights (NULL: 1)
  double w4;                               // the weight of eq4 (0: the plane is not read)
  float* sum_out;                          // one fp32 slot of the loss-sum block
  double* scratch;
};
struct ViscUpdateArgs {
  const float* sum;                        // the (exchanged) slot ViscGradArgs::sum_out named
  double coef, lr, beta1, beta2, eps, theta_min, theta_max;
  double* state;                           // [VISC_STATE]
  float* nu_dev;                           // the fp32 the sweeps read
};
size_t visc_scratch_bytes(long n);
int launch_visc_grad(const ViscGradArgs& a, hipStream_t s);
int launch_visc_update(const ViscUpdateArgs& a, hipStream_t s);
size_t val_scratch_bytes();
int launch_val_stats(const ValStatsArgs& a, hipStream_t s);
int launch_val_keep(const ValKeepArgs& a, hipStream_t s);
// flow diagnostics: stream function, vorticity and vortices of a tensor grid's field planes (flowdiag.hip)
constexpr int FLOW_RECORD = 32, FLOW_STATE = 8;
struct FlowPsiArgs {
  long nx, ny, npad;                       // nodes (node (i, j) = point j nx + i); plane stride of fld
  const float* fld;                        // [FLD_COUNT][npad] field planes of a residual forward on the grid
  const double* ys;                        // [ny]
  double* psi;                             // [ny nx]
};
struct FlowStatsArgs {
  long nx, ny, npad, capacity;             // nodes; plane stride of fld; rows of the history ring
  const float* fld;
  const double *xs, *ys, *psi;             // [nx], [ny], [ny nx] (16-byte aligned)
  double eps, t, every;                    // t < 0: t = (cadence records + 1) * every, from the state
  double *scratch, *state, *ring;
};
size_t flow_scratch_bytes();
int launch_flow_psi(const FlowPsiArgs& a, hipStream_t s);
int launch_flow_stats(const FlowStatsArgs& a, hipStream_t s);
// training-state snapshots: gather / scatter of many buffers with per-segment digests (state.hip)
constexpr int STATE_MAX_SEG = 64;
struct StateSeg {
  const void* rd;                          // what the segment's bytes are read from
  void* wr;                                // where they go (NULL: digest only, nothing is written)
  unsigned long long bytes;                // a multiple of 4
  unsigned long long chunk0;               // index of the segment's first chunk among all chunks of the launch
  unsigned long long pad;                  // pack: bytes to zero behind the segment (up to the next multiple of 256, or the buffer's end)
};
struct StateArgs {
  StateSeg seg[STATE_MAX_SEG];
  int nseg;
  unsigned long long nchunks;              // of all segments
  unsigned long long* digests;             // [nseg][2] (A, B)
  double* scratch;
};
size_t state_scratch_bytes();
unsigned long long state_chunks(unsigned long long bytes);
void state_digest_host(const void* p, unsigned long long bytes, unsigned long long out[2]);
int launch_state_copy(const StateArgs& a, bool pad, hipStream_t s);
