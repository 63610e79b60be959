// Validation error on the device and the best-weights snapshot.  After a value forward has
// written the prediction planes u^, v^, p^ of the n validation points, per channel c over its valid points (a target
// that is NaN or not finite masks the point for that channel, the rule of pinn_value_forward):
//   sum (c^ - c)^2, sum c^2, the valid count; for p also sum d and sum p with d = p^ - p
//   e_c  = sqrt(sum (c^ - c)^2 / sum c^2)                                    (a fraction, not percent)
//   e_p0 = sqrt((sum d^2 - (sum d)^2 / n_p) / (sum p^2 - (sum p)^2 / n_p))   (the pressure up to a constant)
//   uv   = sqrt((sum (u^ - u)^2 + sum (v^ - v)^2) / (sum u^2 + sum v^2))
// Everything is fp64 from the fp32 inputs, one rounding per operation written (d^2 enters its sum by one fma); no float
// atomics, every sum has a fixed order (fixed_fold.h; bit-reproducible).  Two kernels, launch-bound:
//   val_stats_kernel   grid-stride loop of 16-byte loads, block_fold, per-block partials; the last block to finish
//                      folds them by strided_tree_fold, finishes the record, writes one row of the history ring and
//                      updates the monitor state - all device memory, so one captured launch serves every replay
//   val_keep_kernel    copies up to two fp32 segments when the state's `improved` word is 1, nothing otherwise
#include "fixed_fold.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                            // points per thread and iteration: one 16-byte load per plane
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBlocks = 512;                    // grid cap: beyond kMaxBlocks * kTile points the loop repeats
// the sums: [0..2] u: sum d^2, sum c^2, count  [3..5] v  [6..8] p  [9] sum d_p  [10] sum p  [11] -
constexpr int kSums = 12;
// scratch, in doubles: [0] ticket [1..11] the sums of the last launch (slot k at 1 + k) [12..15] - ; then partials
constexpr int kTicket = 0, kOut = 1, kPart = 16;
constexpr int kScratchDoubles = kPart + kSums * kMaxBlocks;
// state, in doubles (PINN_VAL_STATE)
constexpr int S_RECORDS = 0, S_BEST = 1, S_BEST_T = 2, S_STALE = 3, S_NONFINITE = 4, S_IMPROVED = 5, S_CADENCE = 6;

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool valid_target(float t) { return t == t && fabsf(t) <= 3.0e38f; }

__device__ __forceinline__ void unpack(const float4& q, float v[4]) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }

// sqrt(a / b), NaN without valid points
__device__ __forceinline__ double ratio(double a, double b, double cnt) {
  return cnt > 0.0 ? __dsqrt_rn(__ddiv_rn(a, b)) : qnan();
}

__global__ __launch_bounds__(kThreads) void val_stats_kernel(ValStatsArgs a) {
  __shared__ double red[kThreads / 64];
  __shared__ int flag;
  const bool with_p = a.pred[2] != nullptr;
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  // base % 4 == 0 and base < n: the 16-byte load stays inside the plane's row of ceil4(n) floats
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < a.n; base += (long)gridDim.x * kTile) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c == 2 && !with_p) break;
      float ph[4], tg[4];
      unpack(*reinterpret_cast<const float4*>(a.pred[c] + base), ph);
      unpack(*reinterpret_cast<const float4*>(a.tgt[c] + base), tg);
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        if (base + j >= a.n) break;                 // nothing past n reaches a result
        if (!valid_target(tg[j])) continue;
        const double t = (double)tg[j];
        const double d = __dsub_rn((double)ph[j], t);
        acc[3 * c] = __fma_rn(d, d, acc[3 * c]);      // one rounding: d d is not exact (t t below is)
        acc[3 * c + 1] = __dadd_rn(acc[3 * c + 1], __dmul_rn(t, t));
        acc[3 * c + 2] += 1.0;
        if (c == 2) {
          acc[9] = __dadd_rn(acc[9], d);
          acc[10] = __dadd_rn(acc[10], t);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kSums - 1; ++k) acc[k] = block_fold<FoldSum, kThreads>(acc[k], red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kSums - 1; ++k) put(a.scratch + kPart + (size_t)blockIdx.x * kSums + k, acc[k]);
  }
  if (!last_block(a.scratch + kTicket, &flag)) return;
  __shared__ double tree[kThreads][kSums];
  using S_ = FoldSum;
  strided_tree_fold<kThreads, S_, S_, S_, S_, S_, S_, S_, S_, S_, S_, S_>(
      [&](long b, int k) { return get(a.scratch + kPart + (size_t)b * kSums + k); }, (long)gridDim.x, tree);
  if (threadIdx.x != 0) return;
  const double* S = tree[0];
  for (int k = 0; k < kSums - 1; ++k) a.scratch[kOut + k] = S[k];
  // the record
  const double e_u = ratio(S[0], S[1], S[2]), e_v = ratio(S[3], S[4], S[5]), e_p = ratio(S[6], S[7], S[8]);
  double e_p0 = qnan();
  if (S[8] > 0.0) {
    double num = __dsub_rn(S[6], __ddiv_rn(__dmul_rn(S[9], S[9]), S[8]));
    const double den = __dsub_rn(S[7], __ddiv_rn(__dmul_rn(S[10], S[10]), S[8]));
    if (num < 0.0) num = 0.0;                       // rounding of a difference of sums (a NaN stays one)
    e_p0 = __dsqrt_rn(__ddiv_rn(num, den));
  }
  double metric;
  switch (a.metric) {
    case 1: metric = e_u; break;
    case 2: metric = e_v; break;
    case 3: metric = e_p; break;
    case 4: metric = e_p0; break;
    default: metric = (S[2] > 0.0 && S[5] > 0.0) ? __dsqrt_rn(__ddiv_rn(__dadd_rn(S[0], S[3]), __dadd_rn(S[1], S[4]))) : qnan();
  }
  double* st = a.state;
  const double nrec = st[S_RECORDS];
  double t = a.t;
  if (t < 0.0) {                                    // the cadence case: the position is device state
    t = __dmul_rn(st[S_CADENCE] + 1.0, a.every);
    st[S_CADENCE] += 1.0;
  }
  const bool finite = metric == metric && fabs(metric) <= 1.79769313486231570815e308;
  const bool improved = finite && metric < st[S_BEST];
  if (improved) {
    st[S_BEST] = metric; st[S_BEST_T] = t; st[S_STALE] = 0.0;
  } else {
    st[S_STALE] += 1.0;
  }
  if (!finite) st[S_NONFINITE] += 1.0;
  st[S_IMPROVED] = improved ? 1.0 : 0.0;
  st[S_RECORDS] = nrec + 1.0;
  double* row = a.ring + (size_t)((long long)nrec % (long long)a.capacity) * VAL_RECORD;
  row[0] = t; row[1] = e_u; row[2] = e_v; row[3] = e_p; row[4] = e_p0; row[5] = metric;
  row[6] = improved ? 1.0 : 0.0; row[7] = S[8];
}

__global__ __launch_bounds__(kThreads) void val_keep_kernel(ValKeepArgs a) {
  if (a.state[S_IMPROVED] != 1.0) return;           // device memory decides: the launch is the same every time
  const long tid = (long)blockIdx.x * kThreads + threadIdx.x, nthr = (long)gridDim.x * kThreads;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float* __restrict__ src = a.src[s];
    float* __restrict__ dst = a.dst[s];
    const long n = a.n[s];
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
      const long nq = n / 4;                        // whole quads by 16 bytes, the tail by element
      for (long i = tid; i < nq; i += nthr)
        reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
      for (long i = nq * 4 + tid; i < n; i += nthr) dst[i] = src[i];
    } else {
      for (long i = tid; i < n; i += nthr) dst[i] = src[i];
    }
  }
}

}  // namespace

size_t val_scratch_bytes() { return (size_t)kScratchDoubles * sizeof(double); }

int launch_val_stats(const ValStatsArgs& a, hipStream_t s) {
  long blocks = (a.n + kTile - 1) / kTile;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(val_stats_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  return launch_status();
}

int launch_val_keep(const ValKeepArgs& a, hipStream_t s) {
  long blocks = (a.n[0] + a.n[1] + kTile - 1) / kTile;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(val_keep_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  return launch_status();
}
