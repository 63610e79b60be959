// Flow diagnostics on the device: the stream function, the vorticity and the vortices of the
// cavity from the field planes a residual forward left on a tensor grid of nx x ny nodes, node (i, j) = point j nx + i
// (x fastest).  xs [nx], ys [ny] are the fp32 coordinates of the plan widened to fp64, strictly increasing.  Everything
// is fp64 from the fp32 planes, one rounding per operation written; no float atomics, every sum has a fixed order
// (fixed_fold.h); the extrema are order-free (lowest point index on a tie).  The file is compiled with
// -ffp-contract=off (build.py): a product and the sum that takes it stay two roundings.  Three kernels, launch-bound:
//   flow_psi_kernel    one thread per column: psi(i, 0) = 0, psi(i, j) = psi(i, j - 1) + (0.5 (u(i, j) + u(i, j - 1)))
//                      (ys[j] - ys[j - 1]), sequential in j; the loads of kRows rows are issued before their sums
//   flow_stats_kernel  grid-stride loop of 16-byte loads: argmin psi, the argmax psi of every quadrant (lid row out),
//                      sum (u^2 + v^2), sum w^2, sum div^2, max |div|, max |psi| on the lid, the non-finite count;
//                      per-block partials, the last block folds them into scratch
//   flow_count_kernel  the nodes of every quadrant with psi > eps |psi_min| (the threshold is read from scratch); the
//                      last block refines the centres, writes one row of the history ring and updates the state
#include "fixed_fold.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                            // points per thread and iteration: one 16-byte load per fp32 plane
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBlocks = 512;                    // grid cap: beyond kMaxBlocks * kTile points the loop repeats
constexpr int kRows = 8;                           // rows of u in flight per column of the scan
// a block's partials, and (at kOut) the folded results of the last flow_stats launch:
//   [0] psi_min [1] its point  [2 + 2q] psi_max of quadrant q [3 + 2q] its point (q: BL BR TL TR)
//   [10] sum (u^2 + v^2) [11] sum w^2 [12] sum div^2 [13] max |div| [14] max |psi| on the lid [15] non-finite nodes
constexpr int kCols = 16, kPairs = 5, kPlain = 6;
constexpr int P_MIN = 0, P_QMAX = 2, P_KE = 10, P_DIVMAX = 13, P_LID = 14, P_NONFINITE = 15;
// scratch, in doubles: [0] ticket [1..16] the results above [17..20] the quadrant counts [21..31] - ; then partials
constexpr int kTicket = 0, kOut = 1, kCount = 17, kPart = 32;
constexpr int kScratchDoubles = kPart + kCols * kMaxBlocks;
constexpr int S_RECORDS = 0, S_CADENCE = 1, S_NONFINITE = 2;       // state, in doubles (PINN_FLOW_STATE)
constexpr double kNoPoint = 4611686018427387904.0;                 // 2^62: the point of an extremum nothing has taken

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }
__device__ __forceinline__ void unpack(const float4& q, float v[4]) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }

// An extremum with its point: b is taken when it is better, or as good at a lower point (a NaN is never taken)
struct ArgMin {
  __device__ static double identity() { return FoldMin::identity(); }
  __device__ static bool better(double a, double b) { return b < a; }
};
struct ArgMax {
  __device__ static double identity() { return FoldMax::identity(); }
  __device__ static bool better(double a, double b) { return b > a; }
};
template <class Op>
__device__ __forceinline__ void arg_take(double& v, double& at, double bv, double bat) {
  if (Op::better(v, bv) || (bv == v && bat < at)) { v = bv; at = bat; }
}
template <class Op>
__device__ __forceinline__ void arg_wave_fold(double& v, double& at) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double bv = __shfl_down(v, off, 64), bat = __shfl_down(at, off, 64);
    arg_take<Op>(v, at, bv, bat);
  }
}
// over the workgroup, like block_fold; red holds 2 * THREADS / 64 values (valid in thread 0)
template <class Op, int THREADS>
__device__ __forceinline__ void arg_block_fold(double& v, double& at, double* red) {
  arg_wave_fold<Op>(v, at);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = v; red[2 * (threadIdx.x >> 6) + 1] = at; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < THREADS / 64; ++w) arg_take<Op>(v, at, red[2 * w], red[2 * w + 1]);
}

__global__ __launch_bounds__(kThreads) void flow_psi_kernel(FlowPsiArgs a) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.nx) return;
  const float* __restrict__ u = a.fld + FLD_U * a.npad;
  double acc = 0.0, prev = (double)u[i];
  a.psi[i] = 0.0;
  for (long j0 = 1; j0 < a.ny; j0 += kRows) {
    double cur[kRows], dy[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {               // the loads do not depend on the running sum
      const long j = j0 + r;
      if (j < a.ny) { cur[r] = (double)u[j * a.nx + i]; dy[r] = __dsub_rn(a.ys[j], a.ys[j - 1]); }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const long j = j0 + r;
      if (j < a.ny) {
        acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(0.5, __dadd_rn(cur[r], prev)), dy[r]));
        a.psi[j * a.nx + i] = acc;
        prev = cur[r];
      }
    }
  }
}

// the four psi values from base: 16-byte loads for a whole quad, by element for the last one (psi has n entries)
__device__ __forceinline__ void load_psi(const double* psi, long base, long n, double v[4]) {
  if (base + kPer <= n) {
    const double2 lo = *reinterpret_cast<const double2*>(psi + base), hi = *reinterpret_cast<const double2*>(psi + base + 2);
    v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[k] = base + k < n ? psi[base + k] : 0.0;
  }
}

__device__ __forceinline__ double mid(const double* c, long m) { return __dmul_rn(__dadd_rn(c[0], c[m - 1]), 0.5); }
__device__ __forceinline__ int quadrant(const FlowStatsArgs& a, long i, long j, double xm, double ym) {
  return (a.xs[i] >= xm ? 1 : 0) + (a.ys[j] >= ym ? 2 : 0);
}

__global__ __launch_bounds__(kThreads) void flow_stats_kernel(FlowStatsArgs a) {
  __shared__ double red[2 * kThreads / 64];
  __shared__ int flag;
  const long n = a.nx * a.ny;
  const double xm = mid(a.xs, a.nx), ym = mid(a.ys, a.ny);
  double acc[kCols];
  acc[P_MIN] = ArgMin::identity(); acc[P_MIN + 1] = kNoPoint;
#pragma unroll
  for (int q = 0; q < 4; ++q) { acc[P_QMAX + 2 * q] = ArgMax::identity(); acc[P_QMAX + 2 * q + 1] = kNoPoint; }
#pragma unroll
  for (int k = P_KE; k < kCols; ++k) acc[k] = 0.0;
  // base % 4 == 0 and base < n: the 16-byte loads stay inside a plane's row of npad >= ceil4(n) floats
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < n; base += (long)gridDim.x * kTile) {
    float f[6][4];                                  // u, v, u_x, u_y, v_x, v_y: the first six planes
#pragma unroll
    for (int c = 0; c < 6; ++c) unpack(*reinterpret_cast<const float4*>(a.fld + c * a.npad + base), f[c]);
    double ps[4];
    load_psi(a.psi, base, n, ps);
    long j = base / a.nx, i = base - j * a.nx;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (base + k >= n) break;                     // nothing past n reaches a result
      const double p = (double)(base + k);
      const double uu = (double)f[FLD_U][k], vv = (double)f[FLD_V][k];
      const double w = __dsub_rn((double)f[FLD_VX][k], (double)f[FLD_UY][k]);
      const double dv = __dadd_rn((double)f[FLD_UX][k], (double)f[FLD_VY][k]);
      arg_take<ArgMin>(acc[P_MIN], acc[P_MIN + 1], ps[k], p);
      if (j < a.ny - 1) {
        const int q = quadrant(a, i, j, xm, ym);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)              // (a register array: no dynamic index)
          if (q == qq) arg_take<ArgMax>(acc[P_QMAX + 2 * qq], acc[P_QMAX + 2 * qq + 1], ps[k], p);
      } else {
        acc[P_LID] = FoldMax::apply(acc[P_LID], fabs(ps[k]));
      }
      acc[P_KE] = __dadd_rn(acc[P_KE], __dadd_rn(__dmul_rn(uu, uu), __dmul_rn(vv, vv)));
      acc[P_KE + 1] = __dadd_rn(acc[P_KE + 1], __dmul_rn(w, w));
      acc[P_KE + 2] = __dadd_rn(acc[P_KE + 2], __dmul_rn(dv, dv));
      acc[P_DIVMAX] = FoldMax::apply(acc[P_DIVMAX], fabs(dv));
      if (!(finite(ps[k]) && finite(w) && finite(dv))) acc[P_NONFINITE] += 1.0;
      if (++i == a.nx) { i = 0; ++j; }
    }
  }
  arg_block_fold<ArgMin, kThreads>(acc[P_MIN], acc[P_MIN + 1], red);
#pragma unroll
  for (int q = 0; q < 4; ++q) arg_block_fold<ArgMax, kThreads>(acc[P_QMAX + 2 * q], acc[P_QMAX + 2 * q + 1], red);
#pragma unroll
  for (int k = P_KE; k < P_DIVMAX; ++k) acc[k] = block_fold<FoldSum, kThreads>(acc[k], red);
  acc[P_DIVMAX] = block_fold<FoldMax, kThreads>(acc[P_DIVMAX], red);
  acc[P_LID] = block_fold<FoldMax, kThreads>(acc[P_LID], red);
  acc[P_NONFINITE] = block_fold<FoldSum, kThreads>(acc[P_NONFINITE], red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kCols; ++k) put(a.scratch + kPart + (size_t)blockIdx.x * kCols + k, acc[k]);
  }
  if (!last_block(a.scratch + kTicket, &flag)) return;
  // the plain columns by strided_tree_fold; the extrema by the same walk with arg_take
  __shared__ double tree[kThreads][kPlain];
  __shared__ double ext[kThreads][2 * kPairs];
  using S_ = FoldSum; using M_ = FoldMax;
  strided_tree_fold<kThreads, S_, S_, S_, M_, M_, S_>(
      [&](long b, int k) { return get(a.scratch + kPart + (size_t)b * kCols + P_KE + k); }, (long)gridDim.x, tree);
  const int t = threadIdx.x;
  double e[2 * kPairs];
  e[0] = ArgMin::identity(); e[1] = kNoPoint;
#pragma unroll
  for (int q = 1; q < kPairs; ++q) { e[2 * q] = ArgMax::identity(); e[2 * q + 1] = kNoPoint; }
  for (long b = t; b < gridDim.x; b += kThreads) {
    const double* part = a.scratch + kPart + (size_t)b * kCols;
    arg_take<ArgMin>(e[0], e[1], get(part), get(part + 1));
#pragma unroll
    for (int q = 1; q < kPairs; ++q) arg_take<ArgMax>(e[2 * q], e[2 * q + 1], get(part + 2 * q), get(part + 2 * q + 1));
  }
#pragma unroll
  for (int k = 0; k < 2 * kPairs; ++k) ext[t][k] = e[k];
  __syncthreads();
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (t < half) {
      arg_take<ArgMin>(ext[t][0], ext[t][1], ext[t + half][0], ext[t + half][1]);
#pragma unroll
      for (int q = 1; q < kPairs; ++q) arg_take<ArgMax>(ext[t][2 * q], ext[t][2 * q + 1], ext[t + half][2 * q], ext[t + half][2 * q + 1]);
    }
    __syncthreads();
  }
  if (t != 0) return;
  for (int k = 0; k < 2 * kPairs; ++k) a.scratch[kOut + k] = ext[0][k];
  for (int k = 0; k < kPlain; ++k) a.scratch[kOut + P_KE + k] = tree[0][k];
}

// _refine of scripts/flow_topology.py along one axis: the offset 0.5 (a - c) / ((a - 2 b) + c) of the parabola through
// three neighbours, clipped to +-0.5 and 0 on the grid's edge, then c[k] + |d| (c[k2] - c[k]) towards the neighbour k2
__device__ __forceinline__ double refine_axis(const double* psi, long at, long stride, long k, long m, const double* c) {
  double d = 0.0;
  if (k > 0 && k < m - 1) {
    const double lo = psi[at - stride], b = psi[at], hi = psi[at + stride];
    const double den = __dadd_rn(__dsub_rn(lo, __dmul_rn(2.0, b)), hi);
    if (den != 0.0) {
      d = __ddiv_rn(__dmul_rn(0.5, __dsub_rn(lo, hi)), den);
      d = d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
    }
  }
  long k2 = k + (d > 0.0 ? 1 : -1);
  k2 = k2 < 0 ? 0 : (k2 > m - 1 ? m - 1 : k2);
  return __dadd_rn(c[k], __dmul_rn(fabs(d), __dsub_rn(c[k2], c[k])));
}

__global__ __launch_bounds__(kThreads) void flow_count_kernel(FlowStatsArgs a) {
  __shared__ double red[kThreads / 64];
  __shared__ int flag;
  const long n = a.nx * a.ny, nin = n - a.nx;       // the lid row is the last nx points: it is left out
  const double xm = mid(a.xs, a.nx), ym = mid(a.ys, a.ny);
  const double thr = __dmul_rn(a.eps, fabs(a.scratch[kOut + P_MIN]));     // written by the launch before this one
  double cnt[4] = {0.0, 0.0, 0.0, 0.0};
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < nin; base += (long)gridDim.x * kTile) {
    double ps[4];
    load_psi(a.psi, base, n, ps);
    long j = base / a.nx, i = base - j * a.nx;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (base + k >= nin) break;
      if (ps[k] > thr) {
        const int q = quadrant(a, i, j, xm, ym);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          if (q == qq) cnt[qq] += 1.0;
      }
      if (++i == a.nx) { i = 0; ++j; }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q] = block_fold<FoldSum, kThreads>(cnt[q], red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) put(a.scratch + kPart + (size_t)blockIdx.x * kCols + q, cnt[q]);
  }
  if (!last_block(a.scratch + kTicket, &flag)) return;
  __shared__ double tree[kThreads][4];
  using S_ = FoldSum;
  strided_tree_fold<kThreads, S_, S_, S_, S_>(
      [&](long b, int k) { return get(a.scratch + kPart + (size_t)b * kCols + k); }, (long)gridDim.x, tree);
  if (threadIdx.x != 0) return;
  for (int q = 0; q < 4; ++q) a.scratch[kCount + q] = tree[0][q];
  // the record
  const double* R = a.scratch + kOut;
  double* st = a.state;
  const double nrec = st[S_RECORDS];
  double t = a.t;
  if (t < 0.0) {                                    // the cadence case: the position is device state
    t = __dmul_rn(st[S_CADENCE] + 1.0, a.every);
    st[S_CADENCE] += 1.0;
  }
  double* row = a.ring + (size_t)((long long)nrec % (long long)a.capacity) * FLOW_RECORD;
  const double nonfinite = R[P_NONFINITE];
  for (int k = 0; k < FLOW_RECORD; ++k) row[k] = 0.0;
  row[0] = t; row[27] = nonfinite;
  st[S_RECORDS] = nrec + 1.0;
  if (nonfinite > 0.0) {                            // a poisoned field shows no vortex
    st[S_NONFINITE] += 1.0;
    for (int k = 1; k < 27; ++k) row[k] = qnan();
    return;
  }
  const double nn = (double)n;
  const float* __restrict__ uy = a.fld + FLD_UY * a.npad;
  const float* __restrict__ vx = a.fld + FLD_VX * a.npad;
  {
    const long at = (long)R[P_MIN + 1], j = at / a.nx, i = at - j * a.nx;
    row[1] = refine_axis(a.psi, at, 1, i, a.nx, a.xs);
    row[2] = refine_axis(a.psi, at, a.nx, j, a.ny, a.ys);
    row[3] = R[P_MIN];
    row[4] = __dsub_rn((double)vx[at], (double)uy[at]);
  }
  double total = 0.0;
  for (int q = 0; q < 4; ++q) {
    double* e = row + 5 + 4 * q;
    if (R[P_QMAX + 2 * q + 1] < kNoPoint) {
      const long at = (long)R[P_QMAX + 2 * q + 1], j = at / a.nx, i = at - j * a.nx;
      e[0] = refine_axis(a.psi, at, 1, i, a.nx, a.xs);
      e[1] = refine_axis(a.psi, at, a.nx, j, a.ny, a.ys);
      e[2] = R[P_QMAX + 2 * q];
    } else {                                        // a quadrant without nodes below the lid (a coarse non-uniform grid)
      e[0] = e[1] = e[2] = qnan();
    }
    e[3] = __ddiv_rn(tree[0][q], nn);
    total = __dadd_rn(total, e[3]);
  }
  row[21] = total;
  row[22] = R[P_LID];
  row[23] = __ddiv_rn(R[P_KE], nn);
  row[24] = __ddiv_rn(R[P_KE + 1], nn);
  row[25] = __dsqrt_rn(__ddiv_rn(R[P_KE + 2], nn));
  row[26] = R[P_DIVMAX];
}

long stats_blocks(long n) {
  long blocks = (n + kTile - 1) / kTile;
  return blocks > kMaxBlocks ? kMaxBlocks : blocks;
}

}  // namespace

size_t flow_scratch_bytes() { return (size_t)kScratchDoubles * sizeof(double); }

int launch_flow_psi(const FlowPsiArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(flow_psi_kernel, dim3((unsigned)((a.nx + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  return launch_status();
}

int launch_flow_stats(const FlowStatsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(flow_stats_kernel, dim3((unsigned)stats_blocks(a.nx * a.ny)), dim3(kThreads), 0, s, a);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(flow_count_kernel, dim3((unsigned)stats_blocks(a.nx * (a.ny - 1))), dim3(kThreads), 0, s, a);
  return launch_status();
}
