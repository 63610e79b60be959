// Residual-based resampling of the collocation points (RAD): selection of M pool points with density
// proportional to |r|^k / mean|r|^k + c by systematic resampling, and the gather that writes the
// selected points into a live plan's buffers.  Bandwidth-bound; no floating-point atomics, no look-back:
// every sum has a fixed order, so the selection is bit-reproducible from run to run.
//
//   e2_i = eq1^2 + eq2^2 + eq3^2 + w4 eq4^2        (fp64 from the fp32 field planes, no contraction)
//   a_i  = e2_i^(k/2)    (k = 0: 1, k = 1: sqrt, k = 2: e2_i - correctly rounded, no pow ulps; k = 0 and a
//                        non-finite e2_i: NaN, so that S reports it)
//   S = sum a_i ;  S == 0: a_i = 1 (so S = N)
//   b_i = a_i + c S / N ;  C_i = inclusive prefix sum of b ;  T = C_{N-1}
//   o_i = min(M, floor(C_i M / T + U)),  o_{-1} = 0, o_{N-1} = M ;  point i fills out[o_{i-1} .. o_i)
//
// Three passes over fixed partitions of RS_BLOCK points (one workgroup each):
//   1. rs_partial_kernel   per-block fp64 sums of a
//   2. rs_scan_kernel      one workgroup: S, the block sums of b and their exclusive prefix P (P[nb] = T)
//   3. rs_emit_kernel      each block recomputes a, scans its b and writes its points' indices (the block's slots are
//                          shared among all its threads)
// Rounding may order two sums of the same numbers differently; o is kept monotone without changing it
// anywhere else: P is made non-decreasing by an (exact) running max, each block clamps its o into
// [o(P_b), o(P_b+1)] and takes an (exact) integer running max.  So every output slot is written by
// exactly one point, whatever the rounding.
#include "fixed_fold.h"
#include "residual_planes.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PER = 4;                          // points per thread: one 16-byte load per eq plane
constexpr int RS_BLOCK = RS_THREADS * RS_PER;

// a_i from e2_i (kmode: 0 -> 1, 1 -> sqrt, 2 -> e2, 3 -> pow(e2, k / 2))
__device__ __forceinline__ double a_of(double s, int kmode, double half_k) {
  if (kmode == 0) return s <= 1.79769313486231570815e308 ? 1.0 : __builtin_nan("");   // a non-finite residual still reaches S
  if (kmode == 1) return __dsqrt_rn(s);
  if (kmode == 2) return s;
  return pow(s, half_k);
}

// the four a values of this thread's points (0 past n)
__device__ __forceinline__ void load_a(const float* __restrict__ fld, long npad, long n, long base, double w4, int kmode,
                                       double half_k, double a[RS_PER]) {
#pragma unroll
  for (int j = 0; j < RS_PER; ++j) a[j] = 0.0;
  if (base >= n) return;
  float v[4][4];
  load_eq(fld, npad, base, w4 != 0.0, v);
#pragma unroll
  for (int j = 0; j < RS_PER; ++j)
    if (base + j < n) a[j] = a_of(e2_of(v[0][j], v[1][j], v[2][j], v[3][j], w4), kmode, half_k);
}

// o(C) = min(M, floor(C M / T + U)); 0 for a NaN or a negative value
__device__ __forceinline__ long o_of(double C, double Md, double T, double U, long M) {
  const double v = __dadd_rn(__ddiv_rn(__dmul_rn(C, Md), T), U);
  if (v >= Md) return M;
  if (!(v > 0.0)) return 0;
  const long o = (long)floor(v);
  return o < M ? o : M;
}

__global__ __launch_bounds__(RS_THREADS) void rs_partial_kernel(const float* __restrict__ fld, long npad, long n, double w4,
                                                               int kmode, double half_k, double* __restrict__ partial) {
  __shared__ double red[RS_THREADS / 64];
  double a[RS_PER];
  load_a(fld, npad, n, (long)blockIdx.x * RS_BLOCK + RS_PER * threadIdx.x, w4, kmode, half_k, a);
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < RS_PER; ++j) s = __dadd_rn(s, a[j]);
  s = block_fold<FoldSum, RS_THREADS>(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup.  st[0] = S (as summed, before the S == 0 rule), st[1] = T, st[2] = c S_eff / N, st[3] = 1 if S == 0.
// P[b] = sum of b over blocks < b (P[0] = 0, P[nb] = T), non-decreasing.
__global__ __launch_bounds__(RS_THREADS) void rs_scan_kernel(const double* __restrict__ partial, long nb, long n, double c,
                                                            double* __restrict__ st, double* __restrict__ P) {
  __shared__ double red[RS_THREADS];
  __shared__ double sh[2];
  const int t = threadIdx.x;
  const long ch = (nb + RS_THREADS - 1) / RS_THREADS;          // the chunks of chunk_fold
  const long lo = t * ch < nb ? t * ch : nb, hi = lo + ch < nb ? lo + ch : nb;
  const double S = chunk_fold<RS_THREADS, FoldSum>([&](long b) { return partial[b]; }, nb, red);
  if (t == 0) {
    const bool zero = S == 0.0;
    st[0] = S;
    st[3] = zero ? 1.0 : 0.0;
    sh[0] = __ddiv_rn(__dmul_rn(c, zero ? (double)n : S), (double)n);
    sh[1] = zero ? 1.0 : 0.0;
  }
  __syncthreads();
  const double cs = sh[0];
  const bool zero = sh[1] != 0.0;
  auto bsum = [&](long b) {
    const long cnt = (b + 1) * RS_BLOCK <= n ? RS_BLOCK : n - b * RS_BLOCK;
    const double as = zero ? (double)cnt : partial[b];
    return __dadd_rn(as, __dmul_rn(cs, (double)cnt));
  };
  double tot = 0.0;
  for (long b = lo; b < hi; ++b) tot = __dadd_rn(tot, bsum(b));
  __syncthreads();
  red[t] = tot;
  __syncthreads();
  if (t == 0) {                   // exclusive prefix of the chunk totals, in thread order
    double q = 0.0;
    for (int i = 0; i < RS_THREADS; ++i) { const double v = red[i]; red[i] = q; q = __dadd_rn(q, v); }
  }
  __syncthreads();
  double q = red[t];
  for (long b = lo; b < hi; ++b) { P[b] = q; q = __dadd_rn(q, bsum(b)); }
  if (hi == nb && lo < hi) P[nb] = q;
  __syncthreads();
  red[t] = lo < hi ? q : 0.0;     // last value of the chunk (its running values never decrease)
  __syncthreads();
  if (t == 0) {                   // exclusive running max of the chunk ends
    double mx = 0.0;
    for (int i = 0; i < RS_THREADS; ++i) { const double v = red[i]; red[i] = mx; mx = fmax(mx, v); }
  }
  __syncthreads();
  const double mx = red[t];
  for (long b = lo; b < hi; ++b) P[b] = fmax(P[b], mx);
  if (hi == nb && lo < hi) {
    P[nb] = fmax(P[nb], mx);
    st[1] = P[nb];
  }
  if (t == 0) st[2] = cs;
}

__global__ __launch_bounds__(RS_THREADS) void rs_emit_kernel(const float* __restrict__ fld, long npad, long n, double w4,
                                                            int kmode, double half_k, const double* __restrict__ st,
                                                            const double* __restrict__ P, long nb, long M, double U,
                                                            long long* __restrict__ out) {
  __shared__ double wtot[RS_THREADS / 64];
  __shared__ long wmax[RS_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long b = blockIdx.x;
  const double cs = st[2], T = P[nb], Md = (double)M;
  const bool zero = st[3] != 0.0;
  const double Pb = P[b];
  const long o_lo = b == 0 ? 0 : o_of(Pb, Md, T, U, M);
  const long o_hi = b == nb - 1 ? M : o_of(P[b + 1], Md, T, U, M);
  const long base = b * RS_BLOCK + RS_PER * threadIdx.x;
  double a[RS_PER];
  load_a(fld, npad, n, base, w4, kmode, half_k, a);
  // this thread's points in order, then an exclusive scan of the thread totals (wave, then the four waves)
  double loc[RS_PER], run = 0.0;
#pragma unroll
  for (int j = 0; j < RS_PER; ++j) {
    const double bj = base + j < n ? __dadd_rn(zero ? 1.0 : a[j], cs) : 0.0;
    run = __dadd_rn(run, bj);
    loc[j] = run;
  }
  double incl = run;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double v = __shfl_up(incl, off, 64);
    if (lane >= off) incl = __dadd_rn(v, incl);
  }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  double wex = 0.0;
  for (int i = 0; i < w; ++i) wex = __dadd_rn(wex, wtot[i]);
  const double up = __shfl_up(incl, 1, 64);
  const double start = __dadd_rn(Pb, __dadd_rn(wex, lane == 0 ? 0.0 : up));
  long o[RS_PER];
#pragma unroll
  for (int j = 0; j < RS_PER; ++j) {
    const long i = base + j;
    long v = o_of(__dadd_rn(start, loc[j]), Md, T, U, M);       // non-decreasing in j
    v = v < o_lo ? o_lo : v > o_hi ? o_hi : v;
    if (i >= n - 1 || (i + 1) % RS_BLOCK == 0) v = o_hi;       // a block's last point ends where the next block starts
    o[j] = v;
  }
  // exclusive running max of the thread ends (exact, order-free), starting at o_lo
  long m = o[RS_PER - 1];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long v = __shfl_up(m, off, 64);
    if (lane >= off && v > m) m = v;
  }
  if (lane == 63) wmax[w] = m;
  __syncthreads();
  long prev = o_lo;
  for (int i = 0; i < w; ++i) prev = wmax[i] > prev ? wmax[i] : prev;
  {
    const long mup = __shfl_up(m, 1, 64);
    if (lane > 0 && mup > prev) prev = mup;
  }
  // final, non-decreasing o of the block's points (points past n hold o_hi), then the whole block fills the block's
  // slots [o_lo, o_hi): slot s belongs to the first point with o > s (binary search in LDS), so a point that takes many
  // copies is written by all 256 threads, not by its own lane
  __shared__ int os[RS_BLOCK];
#pragma unroll
  for (int j = 0; j < RS_PER; ++j) {
    prev = o[j] > prev ? o[j] : prev;
    os[RS_PER * threadIdx.x + j] = (int)prev;
  }
  __syncthreads();                                              // os[RS_BLOCK - 1] == o_hi
  for (long s = o_lo + threadIdx.x; s < o_hi; s += RS_THREADS) {
    int lo = 0, hi = RS_BLOCK - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (os[mid] > s) hi = mid; else lo = mid + 1;
    }
    out[s] = b * RS_BLOCK + lo;
  }
}

constexpr int RG_THREADS = 256;
constexpr int RG_MAX_BLOCKS = 1024;

// dst[j - lo] = src[idx[j]] for j in [lo, lo + cnt); block g owns the contiguous range [g per, (g + 1) per)
__global__ __launch_bounds__(RG_THREADS) void rs_gather_kernel(const long long* __restrict__ idx, long cnt, long per, long n_pool,
                                                              const float* __restrict__ sx, const float* __restrict__ sy,
                                                              const float* __restrict__ sw, const float* __restrict__ sv,
                                                              float* __restrict__ dx, float* __restrict__ dy,
                                                              float* __restrict__ dw, float* __restrict__ dv,
                                                              double* __restrict__ wpart) {
  __shared__ double red[RG_THREADS / 64];
  const long lo = blockIdx.x * per, hi = lo + per < cnt ? lo + per : cnt;
  double s = 0.0;
  for (long j = lo + threadIdx.x; j < hi; j += RG_THREADS) {
    const long long p = idx[j];
    if (p < 0 || p >= n_pool) continue;
    dx[j] = sx[p];
    dy[j] = sy[p];
    if (dw) { const float v = sw[p]; dw[j] = v; s = __dadd_rn(s, (double)v); }
    if (dv) dv[j] = sv[p];
  }
  if (!wpart) return;
  s = block_fold<FoldSum, RS_THREADS>(s, red);
  if (threadIdx.x == 0) wpart[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void rs_wsum_kernel(const double* __restrict__ wpart, int nparts, double* __restrict__ w_sum) {
  if (threadIdx.x != 0) return;
  *w_sum = ordered_fold<FoldSum>(0.0, wpart, nparts);
}

}  // namespace

// scratch: [0, 32) st | [32, ..) partial[nb] | P[nb + 1] | gather partials[RG_MAX_BLOCKS]
static size_t rs_nblocks(long n) { return (size_t)((n + RS_BLOCK - 1) / RS_BLOCK); }
static size_t rs_off_partial() { return 32; }
static size_t rs_off_P(long n) { return rs_off_partial() + 8 * rs_nblocks(n); }
static size_t rs_off_gather(long n) { return rs_off_P(n) + 8 * (rs_nblocks(n) + 1); }

size_t resample_scratch_bytes(long n_pool) { return (rs_off_gather(n_pool) + 8 * RG_MAX_BLOCKS + 255) / 256 * 256; }

int launch_resample_select(long n, const float* fields, long npad, double w4, double k, double c, double u, long m,
                           void* scratch, long long* out, hipStream_t s) {
  char* base = reinterpret_cast<char*>(scratch);
  double* st = reinterpret_cast<double*>(base);
  double* partial = reinterpret_cast<double*>(base + rs_off_partial());
  double* P = reinterpret_cast<double*>(base + rs_off_P(n));
  const long nb = (long)rs_nblocks(n);
  const int kmode = k == 0.0 ? 0 : k == 1.0 ? 1 : k == 2.0 ? 2 : 3;
  const double half_k = 0.5 * k;
  hipLaunchKernelGGL(rs_partial_kernel, dim3((unsigned)nb), dim3(RS_THREADS), 0, s, fields, npad, n, w4, kmode, half_k, partial);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(RS_THREADS), 0, s, partial, nb, n, c, st, P);
  if ((rc = launch_status())) return rc;
  hipLaunchKernelGGL(rs_emit_kernel, dim3((unsigned)nb), dim3(RS_THREADS), 0, s, fields, npad, n, w4, kmode, half_k, st, P, nb,
                     m, u, out);
  return launch_status();
}

int launch_resample_gather(const long long* idx, long lo, long hi, long n_pool, const float* sx, const float* sy,
                           const float* sw, const float* sv, float* dx, float* dy, float* dw, float* dv, void* scratch,
                           double* w_sum, hipStream_t s) {
  const long cnt = hi - lo;
  long blocks = (cnt + RG_THREADS - 1) / RG_THREADS;
  if (blocks > RG_MAX_BLOCKS) blocks = RG_MAX_BLOCKS;
  const long per = (cnt + blocks - 1) / blocks;
  double* wpart = w_sum ? reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + rs_off_gather(n_pool)) : nullptr;
  hipLaunchKernelGGL(rs_gather_kernel, dim3((unsigned)blocks), dim3(RG_THREADS), 0, s, idx + lo, cnt, per, n_pool, sx, sy, sw, sv,
                     dx, dy, dw, dv, wpart);
  int rc = launch_status();
  if (rc || !w_sum) return rc;
  hipLaunchKernelGGL(rs_wsum_kernel, dim3(1), dim3(64), 0, s, wpart, (int)blocks, w_sum);
  return launch_status();
}
