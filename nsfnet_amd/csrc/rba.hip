// Residual-based attention weights on the collocation points (RBA: Anagnostopoulos, Toscano,
// Stergiopulos & Karniadakis 2024).  State per local point i of the resident store:
//   lam [N] fp32   the attention multiplier
//   s   [N] fp32   the static weights given to set_collocation (SDF weights); absent = 1
//   w   [N] fp32   the effective weight the residual kernels read, w_i = s_i lam_i^2
// After an evaluation has written the unweighted residual planes eq1..eq4 of its n points (i = idx[j], or i = j):
//   e2_j   = eq1^2 + eq2^2 + eq3^2 + w4 eq4^2      (w4 = eq4_weight for ev, 0 for plain NSFnet)
//   r_j    = sqrt(e2_j)
//   rmax   = max_j r_j                              (NaN-propagating; over ALL ranks)
//   lam_i <- gamma lam_i + eta r_j / rmax
//   w_i   <- s_i lam_i^2
// Everything per point is fp64 from the fp32 inputs in exactly this order, without contraction, and rounded to fp32
// once on store (w from the stored lam).  rmax not finite or 0: nothing is written, the record's skip count goes up
// by one (the convention of balance_update_kernel).  The weights evaluation k uses are those made after evaluation
// k - 1: the fused forward + reverse kernel needs w before the residual exists.
// Three kernels, bandwidth-bound; no float atomics, every sum has a fixed order (bit-reproducible):
//   rba_stats_kernel   rmax and the unweighted sums of eq1^2..eq4^2: grid-stride loop of 16-byte loads, wave trees,
//                      per-block partials, the last block to finish folds them in block order
//   rba_apply_kernel   the update with rmax read from scratch (a MAX all-reduce of that word may sit in between);
//                      min / max / sum of the lam values it wrote, folded the same way, go to the record
//   rba_fill_kernel    lam = init, w = s init^2
#include "kernels.h"
#include "xwg_fold.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                            // points per thread and iteration: one 16-byte load per plane
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBlocks = 512;                    // grid cap: beyond kMaxBlocks * kTile points the loop repeats
// scratch, in doubles: [0] rmax [1..4] sums [5] ticket of the stats kernel [6] ticket of the apply kernel [7] -
constexpr int kTicketStats = 5, kTicketApply = 6;
constexpr int kPartStats = 8;                      // [kMaxBlocks][5] max, sum eq1^2 .. eq4^2
constexpr int kPartApply = kPartStats + 5 * kMaxBlocks;   // [kMaxBlocks][4] min, max, sum, count of lam written
constexpr int kScratchDoubles = kPartApply + 4 * kMaxBlocks;

__device__ __forceinline__ double sq(float v) { return __dmul_rn((double)v, (double)v); }   // exact
// NaN-propagating max of non-negative values
__device__ __forceinline__ double nmax(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double e2_of(float e1, float e2, float e3, float e4, double w4) {
  double s = __dadd_rn(__dadd_rn(sq(e1), sq(e2)), sq(e3));
  return __dadd_rn(s, __dmul_rn(w4, sq(e4)));       // w4 = 0: e4 is 0 as well (the plane is not read)
}

// op 0: sum, 1: NaN-propagating max, 2: min, 3: max
template <int OP>
__device__ __forceinline__ double comb(double a, double b) {
  if (OP == 0) return __dadd_rn(a, b);
  if (OP == 1) return nmax(a, b);
  if (OP == 2) return b < a ? b : a;
  return b > a ? b : a;
}
// over the workgroup in a fixed order: wave shuffle tree, then the wave results in wave order (valid in thread 0)
template <int OP>
__device__ __forceinline__ double block_fold(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = comb<OP>(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();                                  // red may still be read from the previous fold
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double t = red[0];
  if (threadIdx.x == 0)
    for (int i = 1; i < kThreads / 64; ++i) t = comb<OP>(t, red[i]);
  return t;
}

// the four residual values of points base .. base + 3 (base % 4 == 0 and base < n <= npad, npad % 4 == 0: in bounds)
__device__ __forceinline__ void load_eq(const float* __restrict__ fld, long npad, long base, bool with4, float v[4][4]) {
  const float4 q1 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ1 * npad + base);
  const float4 q2 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ2 * npad + base);
  const float4 q3 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ3 * npad + base);
  float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (with4) q4 = *reinterpret_cast<const float4*>(fld + (size_t)FLD_EQ4 * npad + base);
  v[0][0] = q1.x; v[0][1] = q1.y; v[0][2] = q1.z; v[0][3] = q1.w;
  v[1][0] = q2.x; v[1][1] = q2.y; v[1][2] = q2.z; v[1][3] = q2.w;
  v[2][0] = q3.x; v[2][1] = q3.y; v[2][2] = q3.z; v[2][3] = q3.w;
  v[3][0] = q4.x; v[3][1] = q4.y; v[3][2] = q4.z; v[3][3] = q4.w;
}

__global__ __launch_bounds__(kThreads) void rba_stats_kernel(const float* __restrict__ fld, long npad, long n, double w4,
                                                             double* scratch) {
  __shared__ double red[kThreads / 64];
  __shared__ int flag;
  const bool with4 = w4 != 0.0;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};       // max r, sums of eq1^2 .. eq4^2
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < n; base += (long)gridDim.x * kTile) {
    float v[4][4];
    load_eq(fld, npad, base, with4, v);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (base + j >= n) break;
      acc[0] = nmax(acc[0], __dsqrt_rn(e2_of(v[0][j], v[1][j], v[2][j], v[3][j], w4)));
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[1 + c] = __dadd_rn(acc[1 + c], sq(v[c][j]));
    }
  }
  acc[0] = block_fold<1>(acc[0], red);
#pragma unroll
  for (int c = 1; c < 5; ++c) acc[c] = block_fold<0>(acc[c], red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) put(scratch + kPartStats + (size_t)blockIdx.x * 5 + c, acc[c]);
  }
  if (!last_block(scratch + kTicketStats, &flag)) return;
  // thread t: blocks t, t + 256, ... in order; then a fixed pairwise tree (thread i takes i + half)
  __shared__ double tree[kThreads][5];
  double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < (int)gridDim.x; b += kThreads) {
    f[0] = nmax(f[0], get(scratch + kPartStats + (size_t)b * 5));
#pragma unroll
    for (int c = 1; c < 5; ++c) f[c] = __dadd_rn(f[c], get(scratch + kPartStats + (size_t)b * 5 + c));
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) tree[threadIdx.x][c] = f[c];
  __syncthreads();
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (threadIdx.x < half) {
      tree[threadIdx.x][0] = nmax(tree[threadIdx.x][0], tree[threadIdx.x + half][0]);
#pragma unroll
      for (int c = 1; c < 5; ++c) tree[threadIdx.x][c] = __dadd_rn(tree[threadIdx.x][c], tree[threadIdx.x + half][c]);
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double mx = tree[0][0];
  if (mx != mx) mx = __longlong_as_double(0x7ff8000000000000LL);     // the positive quiet NaN: integer MAX propagates it
  scratch[0] = mx;
#pragma unroll
  for (int c = 1; c < 5; ++c) scratch[c] = tree[0][c];
}

__global__ __launch_bounds__(kThreads) void rba_apply_kernel(RbaApplyArgs a) {
  __shared__ double red[kThreads / 64];
  __shared__ int flag;
  const double rmax = a.scratch[0];
  if (!(rmax > 0.0 && rmax <= 1.79769313486231570815e308)) {         // 0, NaN or infinite: skipped
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a.record[0] = rmax;
      for (int c = 1; c < 5; ++c) a.record[c] = a.scratch[c];
      a.record[10] += 1.0;
    }
    return;
  }
  const bool with4 = a.w4 != 0.0;
  // the lam values this thread wrote: min, max, sum, count
  double lo = __longlong_as_double(0x7ff0000000000000LL), hi = -lo, sm = 0.0, cnt = 0.0;
  auto upd = [&](float e1, float e2, float e3, float e4, float lam_old, float sw, float& lam_new, float& w_new) {
    const double r = __dsqrt_rn(e2_of(e1, e2, e3, e4, a.w4));
    const double l = __dadd_rn(__dmul_rn(a.gamma, (double)lam_old), __ddiv_rn(__dmul_rn(a.eta, r), rmax));
    lam_new = (float)l;
    const double ls = (double)lam_new;
    w_new = (float)__dmul_rn((double)sw, __dmul_rn(ls, ls));
    lo = ls < lo ? ls : lo; hi = ls > hi ? ls : hi; sm = __dadd_rn(sm, ls); cnt += 1.0;
  };
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < a.n; base += (long)gridDim.x * kTile) {
    float v[4][4];
    load_eq(a.fld, a.npad, base, with4, v);
    if (!a.idx && base + kPer <= a.n) {             // identity, a whole quad: n <= n_store, 16-byte lam / s / w
      const float4 l4 = *reinterpret_cast<const float4*>(a.lam + base);
      const float4 s4 = a.s ? *reinterpret_cast<const float4*>(a.s + base) : make_float4(1.f, 1.f, 1.f, 1.f);
      float4 ln, wn;
      upd(v[0][0], v[1][0], v[2][0], v[3][0], l4.x, s4.x, ln.x, wn.x);
      upd(v[0][1], v[1][1], v[2][1], v[3][1], l4.y, s4.y, ln.y, wn.y);
      upd(v[0][2], v[1][2], v[2][2], v[3][2], l4.z, s4.z, ln.z, wn.z);
      upd(v[0][3], v[1][3], v[2][3], v[3][3], l4.w, s4.w, ln.w, wn.w);
      *reinterpret_cast<float4*>(a.lam + base) = ln;
      *reinterpret_cast<float4*>(a.w + base) = wn;
      continue;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (base + j >= a.n) break;
      const long long i = a.idx ? a.idx[base + j] : (long long)(base + j);
      if (i < 0 || i >= (long long)a.n_store) continue;
      float ln, wn;
      upd(v[0][j], v[1][j], v[2][j], v[3][j], a.lam[i], a.s ? a.s[i] : 1.f, ln, wn);
      a.lam[i] = ln;
      a.w[i] = wn;
    }
  }
  lo = block_fold<2>(lo, red);
  hi = block_fold<3>(hi, red);
  sm = block_fold<0>(sm, red);
  cnt = block_fold<0>(cnt, red);
  double* part = a.scratch + kPartApply;
  if (threadIdx.x == 0) {
    put(part + (size_t)blockIdx.x * 4, lo); put(part + (size_t)blockIdx.x * 4 + 1, hi);
    put(part + (size_t)blockIdx.x * 4 + 2, sm); put(part + (size_t)blockIdx.x * 4 + 3, cnt);
  }
  if (!last_block(a.scratch + kTicketApply, &flag)) return;
  __shared__ double tree[kThreads][4];
  double f[4] = {__longlong_as_double(0x7ff0000000000000LL), -__longlong_as_double(0x7ff0000000000000LL), 0.0, 0.0};
  for (int b = threadIdx.x; b < (int)gridDim.x; b += kThreads) {
    f[0] = comb<2>(f[0], get(part + (size_t)b * 4)); f[1] = comb<3>(f[1], get(part + (size_t)b * 4 + 1));
    f[2] = __dadd_rn(f[2], get(part + (size_t)b * 4 + 2)); f[3] = __dadd_rn(f[3], get(part + (size_t)b * 4 + 3));
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) tree[threadIdx.x][c] = f[c];
  __syncthreads();
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (threadIdx.x < half) {
      double* p = tree[threadIdx.x];
      const double* q = tree[threadIdx.x + half];
      p[0] = comb<2>(p[0], q[0]); p[1] = comb<3>(p[1], q[1]);
      p[2] = __dadd_rn(p[2], q[2]); p[3] = __dadd_rn(p[3], q[3]);
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  a.record[0] = rmax;
  for (int c = 1; c < 5; ++c) a.record[c] = a.scratch[c];
  for (int c = 0; c < 4; ++c) a.record[5 + c] = tree[0][c];
  a.record[9] += 1.0;
}

__global__ __launch_bounds__(kThreads) void rba_fill_kernel(long n, double init, const float* __restrict__ sw,
                                                            float* __restrict__ lam, float* __restrict__ w) {
  const float l = (float)init;
  const double l2 = __dmul_rn((double)l, (double)l);
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    lam[i] = l;
    w[i] = (float)__dmul_rn(sw ? (double)sw[i] : 1.0, l2);
  }
}

int status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

}  // namespace

long rba_blocks(long n) {
  const long b = (n + kTile - 1) / kTile;
  return b < kMaxBlocks ? b : kMaxBlocks;
}

size_t rba_scratch_bytes(long) { return (size_t)kScratchDoubles * sizeof(double); }

int launch_rba_stats(long n, const float* fld, long npad, double w4, double* scratch, hipStream_t s) {
  hipLaunchKernelGGL(rba_stats_kernel, dim3((unsigned)rba_blocks(n)), dim3(kThreads), 0, s, fld, npad, n, w4, scratch);
  return status();
}

int launch_rba_apply(const RbaApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(rba_apply_kernel, dim3((unsigned)rba_blocks(a.n)), dim3(kThreads), 0, s, a);
  return status();
}

int launch_rba_fill(long n, double init, const float* sw, float* lam, float* w, hipStream_t s) {
  long blocks = (n + kThreads - 1) / kThreads;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(rba_fill_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, n, init, sw, lam, w);
  return status();
}
