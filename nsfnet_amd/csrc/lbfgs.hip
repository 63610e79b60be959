// L-BFGS direction by the compact representation (Byrd, Nocedal & Schnabel 1994) for full-batch training stages.
// torch.optim.LBFGS semantics (history of pairs (s, y) accepted when y's > 1e-10, oldest dropped at history_size,
// H0 = gamma I with gamma = y's / y'y of the newest accepted pair); the direction
//
//   a = S'g, b = Y'g, R_ij = s_i'y_j (i <= j), D = diag(s_i'y_i)
//   u = R^-1 a ,  p = R^-T ((D + gamma Y'Y) u - gamma b) ,  d = -(gamma g + S p - gamma Y u)
//
// equals the two-loop recursion's with two streaming passes over the history instead of 2m dependent reductions.
// No floating-point atomics: every sum is fp64 in a fixed order, so the result is bit-reproducible and the same on
// every rank that holds the same gradient.
//
// Launches of one direction call:
//   lb_pass_a      s = t d_prev, y = g - g_prev into the staging slot; per-block partials of y's, y'y, s'g, y'g and of
//                  s_j'y, y_j'y, s_j'g, y_j'g for every live pair j (one read of the live history)
//   lb_colsum      one workgroup per partial column, fixed-order sum
//   lb_update      one workgroup: accept / reject on the device, R and Y'Y columns, gamma, the two triangular solves,
//                  the 2k + 1 combination coefficients
//   lb_pass_c      d from the coefficients (fp64 accumulation), g_prev = g; partials of g'd, max|d|, |g|_1, max|g|
//   lb_finish      one workgroup: the result block
// The first call after a reset (t_prev = 0) runs only lb_update (empty history, gamma = 1) and lb_pass_c: d = -g.
// t_prev < 0 offers a zero step (a line search that accepted t = 0): torch forms s = 0 and rejects the pair.
#include "fixed_fold.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_TILE = LB_THREADS * 4;            // one float4 per thread
constexpr int LB_UNROLL = 4;                       // live pairs per reduction round (8 loads in flight per thread)

// workspace header (at offset 0): int32 words
struct LbHead {
  int count;         // live pairs
  int staging;       // physical slot that receives the next (s, y)
  int accepted;      // last update: 1 accepted, 0 rejected, -1 first iteration
  int pad;
  double gamma;      // H_diag
  double ys;         // y's of the last candidate pair
  double pad2;
};

struct LbLayout {
  long n, np4, m, m1, nb, ncol;
  size_t o_order, o_R, o_YY, o_coef, o_partA, o_col, o_partC, o_gprev, o_S, o_Y, total;
};

size_t al256(size_t v) { return (v + 255) / 256 * 256; }

LbLayout layout(long n, long m) {
  LbLayout L;
  L.n = n; L.np4 = (n + 3) / 4 * 4; L.m = m; L.m1 = m + 1;
  L.nb = (L.np4 + LB_TILE - 1) / LB_TILE;
  L.ncol = 4 * (m + 1);
  size_t o = al256(sizeof(LbHead));
  L.o_order = o; o = al256(o + sizeof(int) * (size_t)L.m1);
  L.o_R = o;     o = al256(o + sizeof(double) * (size_t)L.m1 * L.m1);
  L.o_YY = o;    o = al256(o + sizeof(double) * (size_t)L.m1 * L.m1);
  L.o_coef = o;  o = al256(o + sizeof(double) * (size_t)(2 * m + 1));
  L.o_partA = o; o = al256(o + sizeof(double) * (size_t)L.ncol * L.nb);
  L.o_col = o;   o = al256(o + sizeof(double) * (size_t)L.ncol);
  L.o_partC = o; o = al256(o + sizeof(double) * 4 * (size_t)L.nb);
  L.o_gprev = o; o = al256(o + sizeof(float) * (size_t)L.np4);
  L.o_S = o;     o = al256(o + sizeof(float) * (size_t)L.np4 * L.m1);
  L.o_Y = o;     o = al256(o + sizeof(float) * (size_t)L.np4 * L.m1);
  L.total = o;
  return L;
}

template <typename T> __device__ __forceinline__ T* at(void* ws, size_t off) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off);
}

// four consecutive elements of a caller vector of length n (zeros past n; 16-byte load when whole)
__device__ __forceinline__ float4 load4(const float* __restrict__ v, long e, long n) {
  if (e + 3 < n) return *reinterpret_cast<const float4*>(v + e);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < n) r.x = v[e];
  if (e + 1 < n) r.y = v[e + 1];
  if (e + 2 < n) r.z = v[e + 2];
  return r;
}

__device__ __forceinline__ double dot4(float4 a, float4 b) {
  double s = __dmul_rn((double)a.x, (double)b.x);
  s = __fma_rn((double)a.y, (double)b.y, s);
  s = __fma_rn((double)a.z, (double)b.z, s);
  return __fma_rn((double)a.w, (double)b.w, s);
}

// Pass A.  grid = nb blocks of LB_THREADS; partial column c of block b at partA[c * nb + b]:
// c = 0..3: y's, y'y, s'g, y'g of the candidate; c = 4 (j + 1) + k: s_j'y, y_j'y, s_j'g, y_j'g of live pair j.
__global__ __launch_bounds__(LB_THREADS) void lb_pass_a(void* ws, LbLayout L, const float* __restrict__ g,
                                                         const float* __restrict__ d_prev, float t_prev) {
  __shared__ double red[LB_THREADS / 64][4 * LB_UNROLL];
  const LbHead* h = at<LbHead>(ws, 0);
  const int* order = at<int>(ws, L.o_order);
  const int count = h->count;
  float* S = at<float>(ws, L.o_S);
  float* Y = at<float>(ws, L.o_Y);
  double* part = at<double>(ws, L.o_partA);
  const float* gprev = at<float>(ws, L.o_gprev);
  const long e = ((long)blockIdx.x * LB_THREADS + threadIdx.x) * 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool live = e < L.np4;
  float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), yv = gv, sv = gv;
  if (live) {
    gv = load4(g, e, L.n);
    const float4 gp = *reinterpret_cast<const float4*>(gprev + e);
    const float4 dp = load4(d_prev, e, L.n);
    yv = make_float4(gv.x - gp.x, gv.y - gp.y, gv.z - gp.z, gv.w - gp.w);
    sv = make_float4(t_prev * dp.x, t_prev * dp.y, t_prev * dp.z, t_prev * dp.w);
    const size_t st = (size_t)h->staging * L.np4 + e;
    *reinterpret_cast<float4*>(S + st) = sv;
    *reinterpret_cast<float4*>(Y + st) = yv;
  }
  // candidate: column group 0; then the live pairs LB_UNROLL at a time
  for (int j0 = -1; j0 < count; j0 += (j0 < 0 ? 1 : LB_UNROLL)) {
    const int nj = j0 < 0 ? 1 : (count - j0 < LB_UNROLL ? count - j0 : LB_UNROLL);
    double v[4 * LB_UNROLL];
    if (j0 < 0) {
      v[0] = dot4(yv, sv); v[1] = dot4(yv, yv); v[2] = dot4(sv, gv); v[3] = dot4(yv, gv);
    } else {
      float4 sj[LB_UNROLL], yj[LB_UNROLL];
#pragma unroll
      for (int u = 0; u < LB_UNROLL; ++u) {
        sj[u] = yj[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u < nj && live) {
          const size_t r = (size_t)order[j0 + u] * L.np4 + e;
          sj[u] = *reinterpret_cast<const float4*>(S + r);
          yj[u] = *reinterpret_cast<const float4*>(Y + r);
        }
      }
#pragma unroll
      for (int u = 0; u < LB_UNROLL; ++u) {
        v[4 * u + 0] = dot4(sj[u], yv); v[4 * u + 1] = dot4(yj[u], yv);
        v[4 * u + 2] = dot4(sj[u], gv); v[4 * u + 3] = dot4(yj[u], gv);
      }
    }
#pragma unroll
    for (int q = 0; q < 4 * LB_UNROLL; ++q) {
      if (q < 4 * nj) {
        const double s = wave_fold<FoldSum>(v[q]);
        if (lane == 0) red[w][q] = s;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < 4 * nj) {
      const int q = threadIdx.x;
      const double s = ordered_fold<FoldSum>(red[0][q], &red[1][q], LB_THREADS / 64 - 1, 4 * LB_UNROLL);   // wave order
      const long col = (j0 < 0 ? 0 : 4 * (j0 + 1)) + q;
      part[col * L.nb + blockIdx.x] = s;
    }
    __syncthreads();
  }
}

// one workgroup per column of nb partials: contiguous chunks per thread in order, then the chunk sums in thread order
__global__ __launch_bounds__(LB_THREADS) void lb_colsum(void* ws, LbLayout L) {
  __shared__ double red[LB_THREADS];
  const LbHead* h = at<LbHead>(ws, 0);
  const long col = blockIdx.x;
  if (col >= 4L * (h->count + 1)) return;
  const double* part = at<double>(ws, L.o_partA) + col * L.nb;
  const double t = chunk_fold<LB_THREADS, FoldSum>([&](long b) { return part[b]; }, L.nb, red);
  if (threadIdx.x == 0) at<double>(ws, L.o_col)[col] = t;
}

// One workgroup: the history update and the dense part.  first != 0: empty history, gamma = 1 (d = -g).
__global__ __launch_bounds__(LB_THREADS) void lb_update(void* ws, LbLayout L, int first) {
  extern __shared__ double sh[];                  // a, b, u, rhs: 4 (m + 1) doubles; order: m + 1 ints
  double* a = sh;
  double* b = a + L.m1;
  double* u = b + L.m1;
  double* rhs = u + L.m1;
  int* ord = reinterpret_cast<int*>(rhs + L.m1);
  __shared__ int s_k;
  __shared__ double s_gamma;
  LbHead* h = at<LbHead>(ws, 0);
  int* order = at<int>(ws, L.o_order);
  double* R = at<double>(ws, L.o_R);
  double* YY = at<double>(ws, L.o_YY);
  double* coef = at<double>(ws, L.o_coef);
  const double* col = at<double>(ws, L.o_col);
  const int tid = threadIdx.x;
  const long M1 = L.m1;
  if (first) {
    if (tid == 0) {
      h->count = 0; h->staging = 0; h->accepted = -1; h->gamma = 1.0; h->ys = 0.0;
      coef[0] = -1.0;
    }
    return;
  }
  const int count = h->count;
  const double ys = col[0], yy = col[1];
  const bool acc = ys > 1e-10;                     // (a NaN y's is rejected, as in torch)
  const int drop = acc && count == L.m ? 1 : 0;
  const int k = acc ? count - drop + 1 : count;
  const int stg = h->staging;
  const int dropped = drop ? order[0] : stg;       // read before any thread rewrites order[]
  // live pairs after the update, oldest first: old pairs drop.., then the candidate
  for (int j = tid; j < k; j += LB_THREADS) {
    const int jo = j + drop;                        // index among the old pairs
    if (acc && j == k - 1) {
      ord[j] = stg; a[j] = col[2]; b[j] = col[3];
    } else {
      ord[j] = order[jo]; a[j] = col[4 * (jo + 1) + 2]; b[j] = col[4 * (jo + 1) + 3];
    }
  }
  __syncthreads();
  if (acc) {                                       // new column of R and row / column of Y'Y (physical slots)
    for (int j = tid; j < k - 1; j += LB_THREADS) {
      const int jo = j + drop, pj = ord[j];
      R[(size_t)pj * M1 + stg] = col[4 * (jo + 1) + 0];
      const double v = col[4 * (jo + 1) + 1];
      YY[(size_t)pj * M1 + stg] = v;
      YY[(size_t)stg * M1 + pj] = v;
    }
    if (tid == 0) { R[(size_t)stg * M1 + stg] = ys; YY[(size_t)stg * M1 + stg] = yy; }
  }
  __syncthreads();
  if (tid == 0) {
    s_k = k;
    s_gamma = acc ? __ddiv_rn(ys, yy) : h->gamma;
  }
  __syncthreads();
  const double gamma = s_gamma;
  auto Rl = [&](int i, int j) { return R[(size_t)ord[i] * M1 + ord[j]]; };
  // u = R^-1 a (back substitution, column-oriented: step i fixes u_i and updates rows < i in a fixed order)
  for (int j = tid; j < k; j += LB_THREADS) rhs[j] = a[j];
  __syncthreads();
  for (int i = k - 1; i >= 0; --i) {
    const double ui = __ddiv_rn(rhs[i], Rl(i, i));
    for (int j = tid; j < i; j += LB_THREADS) rhs[j] = __fma_rn(-Rl(j, i), ui, rhs[j]);
    if (tid == 0) u[i] = ui;
    __syncthreads();
  }
  // rhs = (D + gamma Y'Y) u - gamma b
  for (int i = tid; i < k; i += LB_THREADS) {
    double s = 0.0;
    for (int j = 0; j < k; ++j) s = __fma_rn(YY[(size_t)ord[i] * M1 + ord[j]], u[j], s);
    rhs[i] = __fma_rn(Rl(i, i), u[i], __dmul_rn(gamma, __dadd_rn(s, -b[i])));
  }
  __syncthreads();
  // p = R^-T rhs (forward substitution); p overwrites a
  for (int i = 0; i < k; ++i) {
    const double pi = __ddiv_rn(rhs[i], Rl(i, i));
    for (int j = i + 1 + tid; j < k; j += LB_THREADS) rhs[j] = __fma_rn(-Rl(i, j), pi, rhs[j]);
    if (tid == 0) a[i] = pi;
    __syncthreads();
  }
  // coefficients: d = c0 g + sum_j cs_j s_j + cy_j y_j
  for (int j = tid; j < k; j += LB_THREADS) {
    coef[1 + j] = -a[j];
    coef[1 + L.m + j] = __dmul_rn(gamma, u[j]);
    order[j] = ord[j];
  }
  if (tid == 0) {
    coef[0] = -gamma;
    h->count = k;
    h->staging = acc ? (drop ? dropped : k) : stg;     // slots 0..m: before the first drop they fill in order
    h->accepted = acc ? 1 : 0;
    h->gamma = gamma;
    h->ys = ys;
  }
}

// Pass C (write_d) and the probe (!write_d): partials of g'd, max|d|, |g|_1, max|g| at partC[c * nb + b].
__global__ __launch_bounds__(LB_THREADS) void lb_pass_c(void* ws, LbLayout L, const float* __restrict__ g, float* d,
                                                         int write_d) {
  __shared__ double redd[LB_THREADS / 64][2];
  __shared__ float redf[LB_THREADS / 64][2];
  const long e = ((long)blockIdx.x * LB_THREADS + threadIdx.x) * 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), dv = gv;
  if (e < L.np4) {
    gv = load4(g, e, L.n);
    if (write_d) {
      const LbHead* h = at<LbHead>(ws, 0);
      const int* order = at<int>(ws, L.o_order);
      const double* coef = at<double>(ws, L.o_coef);
      const float* S = at<float>(ws, L.o_S);
      const float* Y = at<float>(ws, L.o_Y);
      const int k = h->count;
      const double c0 = coef[0];
      double acc[4] = {__dmul_rn(c0, (double)gv.x), __dmul_rn(c0, (double)gv.y), __dmul_rn(c0, (double)gv.z),
                       __dmul_rn(c0, (double)gv.w)};
      for (int j = 0; j < k; ++j) {
        const size_t r = (size_t)order[j] * L.np4 + e;
        const float4 sj = *reinterpret_cast<const float4*>(S + r);
        const float4 yj = *reinterpret_cast<const float4*>(Y + r);
        const double cs = coef[1 + j], cy = coef[1 + L.m + j];
        acc[0] = __fma_rn(cy, (double)yj.x, __fma_rn(cs, (double)sj.x, acc[0]));
        acc[1] = __fma_rn(cy, (double)yj.y, __fma_rn(cs, (double)sj.y, acc[1]));
        acc[2] = __fma_rn(cy, (double)yj.z, __fma_rn(cs, (double)sj.z, acc[2]));
        acc[3] = __fma_rn(cy, (double)yj.w, __fma_rn(cs, (double)sj.w, acc[3]));
      }
      dv = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
      if (e + 3 < L.n) {
        *reinterpret_cast<float4*>(d + e) = dv;
      } else {
        if (e < L.n) d[e] = dv.x;
        if (e + 1 < L.n) d[e + 1] = dv.y;
        if (e + 2 < L.n) d[e + 2] = dv.z;
        dv = make_float4(e < L.n ? dv.x : 0.f, e + 1 < L.n ? dv.y : 0.f, e + 2 < L.n ? dv.z : 0.f, 0.f);
      }
      *reinterpret_cast<float4*>(at<float>(ws, L.o_gprev) + e) = gv;
    } else {
      dv = load4(d, e, L.n);
    }
  }
  double gtd = dot4(gv, dv);
  double g1 = __dadd_rn(__dadd_rn((double)fabsf(gv.x), (double)fabsf(gv.y)),
                        __dadd_rn((double)fabsf(gv.z), (double)fabsf(gv.w)));
  // NaN-propagating: max|d| and max|g| must report a NaN, as torch's do
  float dm = nmax(nmax(fabsf(dv.x), fabsf(dv.y)), nmax(fabsf(dv.z), fabsf(dv.w)));
  float gm = nmax(nmax(fabsf(gv.x), fabsf(gv.y)), nmax(fabsf(gv.z), fabsf(gv.w)));
  gtd = wave_fold<FoldSum>(gtd); g1 = wave_fold<FoldSum>(g1); dm = wave_fold<FoldNanMax>(dm); gm = wave_fold<FoldNanMax>(gm);
  if (lane == 0) { redd[w][0] = gtd; redd[w][1] = g1; redf[w][0] = dm; redf[w][1] = gm; }
  __syncthreads();
  if (threadIdx.x == 0) {
    constexpr int W = LB_THREADS / 64;              // the wave results in wave order
    const double s0 = ordered_fold<FoldSum>(redd[0][0], &redd[1][0], W - 1, 2);
    const double s1 = ordered_fold<FoldSum>(redd[0][1], &redd[1][1], W - 1, 2);
    const float m0 = ordered_fold<FoldNanMax>(redf[0][0], &redf[1][0], W - 1, 2);
    const float m1 = ordered_fold<FoldNanMax>(redf[0][1], &redf[1][1], W - 1, 2);
    double* part = at<double>(ws, L.o_partC);
    part[0 * L.nb + blockIdx.x] = s0;
    part[1 * L.nb + blockIdx.x] = (double)m0;
    part[2 * L.nb + blockIdx.x] = s1;
    part[3 * L.nb + blockIdx.x] = (double)m1;
  }
}

// result[0..3] = g'd, max|d|, |g|_1, max|g|; with_state: result[4..7] = accepted, count, gamma, y's
__global__ __launch_bounds__(LB_THREADS) void lb_finish(void* ws, LbLayout L, double* result, int with_state) {
  __shared__ double red[4][LB_THREADS];
  const double* part = at<double>(ws, L.o_partC);
  // chunk_fold of the four columns at once: lane 0 of wave c finishes column c
  static_assert(LB_THREADS / 64 == 4, "one wave per column");
  for (int c = 0; c < 4; ++c) {
    auto load = [&](long b) { return part[c * L.nb + b]; };
    red[c][threadIdx.x] = (c & 1) ? chunk_partial<LB_THREADS, FoldNanMax>(load, L.nb) : chunk_partial<LB_THREADS, FoldSum>(load, L.nb);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    const int c = threadIdx.x >> 6;
    result[c] = (c & 1) ? ordered_fold<FoldNanMax>(0.0, red[c], LB_THREADS) : ordered_fold<FoldSum>(0.0, red[c], LB_THREADS);
  }
  if (with_state && threadIdx.x == 0) {
    const LbHead* h = at<LbHead>(ws, 0);
    result[4] = (double)h->accepted;
    result[5] = (double)h->count;
    result[6] = h->gamma;
    result[7] = h->ys;
  }
}

}  // namespace

size_t lbfgs_workspace_bytes(long n, long m) { return layout(n, m).total; }

int launch_lbfgs_reset(void* ws, long n, long m, hipStream_t s) {
  (void)n; (void)m;
  return (int)hipMemsetAsync(ws, 0, sizeof(LbHead), s);
}

int launch_lbfgs_direction(void* ws, long n, long m, const float* g, float t_prev, float* d, double* result,
                           hipStream_t s) {
  const LbLayout L = layout(n, m);
  const int first = t_prev == 0.f ? 1 : 0;
  if (!first) {        // t_prev < 0: a zero step (s = 0, y's = 0: the pair is rejected, the history kept)
    hipLaunchKernelGGL(lb_pass_a, dim3((unsigned)L.nb), dim3(LB_THREADS), 0, s, ws, L, g, (const float*)d,
                       t_prev < 0.f ? 0.f : t_prev);
    hipLaunchKernelGGL(lb_colsum, dim3((unsigned)L.ncol), dim3(LB_THREADS), 0, s, ws, L);
  }
  const size_t shm = sizeof(double) * 4 * (size_t)L.m1 + sizeof(int) * (size_t)L.m1;
  hipLaunchKernelGGL(lb_update, dim3(1), dim3(LB_THREADS), shm, s, ws, L, first);
  hipLaunchKernelGGL(lb_pass_c, dim3((unsigned)L.nb), dim3(LB_THREADS), 0, s, ws, L, g, d, 1);
  hipLaunchKernelGGL(lb_finish, dim3(1), dim3(LB_THREADS), 0, s, ws, L, result, 1);
  return launch_status();
}

int launch_lbfgs_probe(void* ws, long n, long m, const float* g, const float* d, double* result, hipStream_t s) {
  const LbLayout L = layout(n, m);
  hipLaunchKernelGGL(lb_pass_c, dim3((unsigned)L.nb), dim3(LB_THREADS), 0, s, ws, L, g, const_cast<float*>(d), 0);
  hipLaunchKernelGGL(lb_finish, dim3(1), dim3(LB_THREADS), 0, s, ws, L, result, 0);
  return launch_status();
}
