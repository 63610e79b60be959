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
// Three kernels, bandwidth-bound; no float atomics, every sum has a fixed order (fixed_fold.h; bit-reproducible):
//   rba_stats_kernel   rmax and the unweighted sums of eq1^2..eq4^2: grid-stride loop of 16-byte loads, block_fold,
//                      per-block partials, the last block to finish folds them by strided_tree_fold
//   rba_apply_kernel   the update with rmax read from scratch (a MAX all-reduce of that word may sit in between);
//                      min / max / sum of the lam values it wrote, folded the same way, go to the record
//   rba_fill_kernel    lam = init, w = s init^2
#include "fixed_fold.h"
#include "residual_planes.h"

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
  acc[0] = block_fold<FoldNanMax, kThreads>(acc[0], red);
#pragma unroll
  for (int c = 1; c < 5; ++c) acc[c] = block_fold<FoldSum, kThreads>(acc[c], red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) put(scratch + kPartStats + (size_t)blockIdx.x * 5 + c, acc[c]);
  }
  if (!last_block(scratch + kTicketStats, &flag)) return;
  __shared__ double tree[kThreads][5];
  strided_tree_fold<kThreads, FoldNanMax, FoldSum, FoldSum, FoldSum, FoldSum>(
      [&](long b, int c) { return get(scratch + kPartStats + (size_t)b * 5 + c); }, (long)gridDim.x, tree);
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
  double lo = FoldMin::identity(), hi = FoldMax::identity(), sm = 0.0, cnt = 0.0;
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
  lo = block_fold<FoldMin, kThreads>(lo, red);
  hi = block_fold<FoldMax, kThreads>(hi, red);
  sm = block_fold<FoldSum, kThreads>(sm, red);
  cnt = block_fold<FoldSum, kThreads>(cnt, red);
  double* part = a.scratch + kPartApply;
  if (threadIdx.x == 0) {
    put(part + (size_t)blockIdx.x * 4, lo); put(part + (size_t)blockIdx.x * 4 + 1, hi);
    put(part + (size_t)blockIdx.x * 4 + 2, sm); put(part + (size_t)blockIdx.x * 4 + 3, cnt);
  }
  if (!last_block(a.scratch + kTicketApply, &flag)) return;
  __shared__ double tree[kThreads][4];
  strided_tree_fold<kThreads, FoldMin, FoldMax, FoldSum, FoldSum>(
      [&](long b, int c) { return get(part + (size_t)b * 4 + c); }, (long)gridDim.x, tree);
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

}  // namespace

long rba_blocks(long n) {
  const long b = (n + kTile - 1) / kTile;
  return b < kMaxBlocks ? b : kMaxBlocks;
}

size_t rba_scratch_bytes(long) { return (size_t)kScratchDoubles * sizeof(double); }

int launch_rba_stats(long n, const float* fld, long npad, double w4, double* scratch, hipStream_t s) {
  hipLaunchKernelGGL(rba_stats_kernel, dim3((unsigned)rba_blocks(n)), dim3(kThreads), 0, s, fld, npad, n, w4, scratch);
  return launch_status();
}

int launch_rba_apply(const RbaApplyArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(rba_apply_kernel, dim3((unsigned)rba_blocks(a.n)), dim3(kThreads), 0, s, a);
  return launch_status();
}

int launch_rba_fill(long n, double init, const float* sw, float* lam, float* w, hipStream_t s) {
  long blocks = (n + kThreads - 1) / kThreads;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(rba_fill_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, n, init, sw, lam, w);
  return launch_status();
}
