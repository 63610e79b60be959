// Device-resident convergence monitor (include/nsfnet_pinn.h "Convergence monitor").  Two
// launches, both inside the captured step, nothing synchronises:
//   monitor_vis_kernel      over the vis_t plane [n] of the plan that was just evaluated (non-negative entries): the fp64
//                           sum, rounded once to fp32, into a slot of the loss-sum block - so the all-reduce that is sent
//                           anyway makes it global - and, per rank, info = [max (NaN-propagating), entries >= vis_t0,
//                           the fp64 sum, n].  Grid-stride loop of 16-byte loads (the last quad by element: the plane has
//                           n entries), block_fold, per-block partials, the last block folds them by strided_tree_fold.
//                           No float atomics, every sum has a fixed order (fixed_fold.h; bit-reproducible).
//   monitor_observe_kernel  one workgroup, after the optimiser update.  state[0] (the update counter) goes up by one;
//                           unless it is a multiple of `every` nothing else happens.  An observation, everything fp64
//                           from the fp32 sums, one rounding per operation in exactly this order, without contraction:
//     eq_k    = eq[k] / n_eq                                   k = 0..3
//     loss_e  = (eq_0 + eq_1) + eq_2            ev:  ... + w4 eq_3
//     loss_b  = (bc[0] + bc[1]) / n_b
//     loss_s  = (sup[0] + sup[1]) / n_s  [+ sup[2] / n_p where n_p > 0]       (0 without supervised points)
//     loss    = ((w_b loss_b) + (alpha_e loss_e)) + (w_s loss_s)              w_b, w_s = lam[0], lam[1] or alpha_b, alpha_s
//     vis     = eq[4] / n_eq  (ev; else 0)      Re_eff = 1 / (1 / Re + vis)
//   row = [t, loss, loss_e, loss_b, loss_s, eq_0..eq_3, vis, Re_eff, stop code] into the ring at (observations % capacity).
//   A non-finite loss is counted, sets the sticky bit NONFINITE and stays out of the window.  Otherwise Q (loss | loss_e |
//   loss_b) and Re_eff are added to the window sums; when the window holds `window` observations its means
//   (sum / window) are compared with the previous window's - the first complete window only sets them:
//     plateau:  prev == 0 or (prev - mean) / |prev| < min_rel      -> stale + 1, else stale = 0
//     re_eff:   |mean_re - prev_re| / prev_re < re_tol             -> settled + 1, else settled = 0
//   From t >= min_updates on, stale >= patience sets the sticky bit PLATEAU and settled >= patience the sticky bit RE_EFF;
//   the t that set each bit is recorded.  The kernel sets bits and nothing else: the host reads them at log points.
// state, in doubles (PINN_MON_STATE): see include/nsfnet_pinn.h.
#include "fixed_fold.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                            // entries per thread and iteration: one 16-byte load
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBlocks = 512;                    // grid cap: beyond kMaxBlocks * kTile entries the loop repeats
constexpr int kCols = 3;                           // sum, max, count
// scratch, in doubles: [0] ticket [1..7] - [8..] partials [kMaxBlocks][kCols]
constexpr int kTicket = 0, kPart = 8;
constexpr int kScratchDoubles = kPart + kCols * kMaxBlocks;
// state, in doubles
constexpr int S_UPDATES = 0, S_OBS = 1, S_NONFINITE = 2, S_FILL = 3, S_SUM_Q = 4, S_SUM_RE = 5, S_WINDOWS = 6, S_PREV_Q = 7,
              S_PREV_RE = 8, S_STALE = 9, S_SETTLED = 10, S_STOP = 11, S_T_PLATEAU = 12, S_T_RE_EFF = 13, S_T_NONFINITE = 14;

__global__ __launch_bounds__(kThreads) void monitor_vis_kernel(MonVisArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[kThreads / 64];
  __shared__ int flag;
  double acc[kCols] = {0.0, 0.0, 0.0};
  const float cap = a.vis_t0;
  auto entry = [&](float v) {
    acc[0] = acc[0] + (double)v;
    acc[1] = nmax(acc[1], (double)v);
    acc[2] = acc[2] + (v >= cap ? 1.0 : 0.0);
  };
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < a.n; base += (long)gridDim.x * kTile) {
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (base + kPer <= a.n) {                      // base % 4 == 0 and the plane is 16-byte aligned
      q = *reinterpret_cast<const float4*>(a.vis_t + base);
    } else {                                       // the ragged tail: the plane has n entries
      q.x = a.vis_t[base];
      if (base + 1 < a.n) q.y = a.vis_t[base + 1];
      if (base + 2 < a.n) q.z = a.vis_t[base + 2];
    }
    entry(q.x);
    if (base + 1 < a.n) entry(q.y);
    if (base + 2 < a.n) entry(q.z);
    if (base + 3 < a.n) entry(q.w);
  }
  acc[0] = block_fold<FoldSum, kThreads>(acc[0], red);
  acc[1] = block_fold<FoldNanMax, kThreads>(acc[1], red);
  acc[2] = block_fold<FoldSum, kThreads>(acc[2], red);
  double* part = a.scratch + kPart;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) put(part + (size_t)blockIdx.x * kCols + c, acc[c]);
  }
  if (!last_block(a.scratch + kTicket, &flag)) return;
  __shared__ double tree[kThreads][kCols];
  strided_tree_fold<kThreads, FoldSum, FoldNanMax, FoldSum>(
      [&](long b, int c) { return get(part + (size_t)b * kCols + c); }, (long)gridDim.x, tree);
  if (threadIdx.x != 0) return;
  *a.sum_out = (float)tree[0][0];                  // the one rounding to fp32
  a.info[0] = tree[0][1];
  a.info[1] = tree[0][2];
  a.info[2] = tree[0][0];
  a.info[3] = (double)a.n;
}

__device__ __forceinline__ bool finite64(double v) { return v == v && fabs(v) <= 1.79769313486231570815e308; }

__global__ __launch_bounds__(64) void monitor_observe_kernel(MonObserveArgs a) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  double* st = a.state;
  const double t = st[S_UPDATES] + 1.0;
  st[S_UPDATES] = t;
  if ((long long)t % (long long)a.every != 0) return;
  double eq[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) eq[k] = __ddiv_rn((double)a.eq[k], a.n_eq);
  double loss_e = (eq[0] + eq[1]) + eq[2];
  if (a.ev) {
    const double e4 = a.w4 * eq[3];
    loss_e = loss_e + e4;
  }
  const double sb = (double)a.bc[0] + (double)a.bc[1];
  const double loss_b = __ddiv_rn(sb, a.n_b);
  double loss_s = 0.0;
  if (a.sup && a.n_s > 0.0) {
    const double ss = (double)a.sup[0] + (double)a.sup[1];
    loss_s = __ddiv_rn(ss, a.n_s);
    if (a.n_p > 0.0) {
      const double sp = __ddiv_rn((double)a.sup[2], a.n_p);
      loss_s = loss_s + sp;
    }
  }
  const double w_b = a.lam ? (double)a.lam[0] : a.alpha_b, w_s = a.lam ? (double)a.lam[1] : a.alpha_s;
  const double tb = w_b * loss_b, te = a.alpha_e * loss_e, ts = w_s * loss_s;
  const double loss = (tb + te) + ts;
  const double vis = a.ev ? __ddiv_rn((double)a.eq[4], a.n_eq) : 0.0;
  const double inv = __ddiv_rn(1.0, a.Re) + vis;
  const double re_eff = __ddiv_rn(1.0, inv);

  const double nobs = st[S_OBS];
  st[S_OBS] = nobs + 1.0;
  int code = (int)st[S_STOP];
  if (!finite64(loss)) {
    st[S_NONFINITE] += 1.0;
    if (!(code & MON_STOP_NONFINITE)) {
      code |= MON_STOP_NONFINITE;
      st[S_T_NONFINITE] = t;
    }
  } else {
    const double q = a.quantity == 1 ? loss_e : a.quantity == 2 ? loss_b : loss;
    st[S_FILL] += 1.0;
    st[S_SUM_Q] = st[S_SUM_Q] + q;
    st[S_SUM_RE] = st[S_SUM_RE] + re_eff;
    if (st[S_FILL] >= (double)a.window) {
      const double mean = __ddiv_rn(st[S_SUM_Q], (double)a.window), mean_re = __ddiv_rn(st[S_SUM_RE], (double)a.window);
      if (st[S_WINDOWS] >= 1.0) {
        if (a.plateau_on) {
          const double prev = st[S_PREV_Q];
          const double d = prev - mean;
          const bool stale = prev == 0.0 || __ddiv_rn(d, fabs(prev)) < a.min_rel;
          st[S_STALE] = stale ? st[S_STALE] + 1.0 : 0.0;
        }
        if (a.re_on) {
          const double prev = st[S_PREV_RE];
          const double d = mean_re - prev;
          const bool settled = __ddiv_rn(fabs(d), prev) < a.re_tol;
          st[S_SETTLED] = settled ? st[S_SETTLED] + 1.0 : 0.0;
        }
      }
      st[S_PREV_Q] = mean; st[S_PREV_RE] = mean_re;
      st[S_WINDOWS] += 1.0;
      st[S_FILL] = 0.0; st[S_SUM_Q] = 0.0; st[S_SUM_RE] = 0.0;
    }
  }
  if (t >= (double)a.min_updates) {
    if (a.plateau_on && st[S_STALE] >= (double)a.patience && !(code & MON_STOP_PLATEAU)) {
      code |= MON_STOP_PLATEAU;
      st[S_T_PLATEAU] = t;
    }
    if (a.re_on && st[S_SETTLED] >= (double)a.patience && !(code & MON_STOP_RE_EFF)) {
      code |= MON_STOP_RE_EFF;
      st[S_T_RE_EFF] = t;
    }
  }
  st[S_STOP] = (double)code;
  double* row = a.ring + (size_t)((long long)nobs % (long long)a.capacity) * MON_RECORD;
  row[0] = t; row[1] = loss; row[2] = loss_e; row[3] = loss_b; row[4] = loss_s;
  row[5] = eq[0]; row[6] = eq[1]; row[7] = eq[2]; row[8] = eq[3];
  row[9] = vis; row[10] = re_eff; row[11] = (double)code;
}

}  // namespace

size_t monitor_scratch_bytes() { return (size_t)kScratchDoubles * sizeof(double); }

int launch_monitor_vis_stats(const MonVisArgs& a, hipStream_t s) {
  long blocks = (a.n + kTile - 1) / kTile;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(monitor_vis_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  return launch_status();
}

int launch_monitor_observe(const MonObserveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(monitor_observe_kernel, dim3(1), dim3(64), 0, s, a);
  return launch_status();
}
