// The fixed-order reductions of the small kernels (balance, confgrad, rba, validate, optim, rwf, resample, lbfgs): every
// order the project promises to be bit-reproducible and equal on all ranks is written here once, and modelled once in
// tests/fold_model.py.  No floating-point atomics anywhere.
//   wave_fold          64 lanes: lane i takes lane i + 32, then + 16, ... + 1; lane 0 holds the result
//   block_fold         wave_fold, then the wave results in wave order starting from wave 0's
//   strided_tree_fold  C columns of nblk partials: thread t takes partials t, t + THREADS, ... in order, then a pairwise
//                      tree over the threads (thread i takes thread i + half)
//   chunk_fold         nblk partials: thread t takes a contiguous chunk in order, then the chunk results in thread order
//   put / get / last_block / last_ticket   partials that cross workgroups inside one launch
//   launch_status      the host tail of a launcher
#pragma once
#include <hip/hip_runtime.h>

// NaN-propagating max of non-negative values: a NaN entry must reach the result
__device__ __forceinline__ double nmax(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ float nmax(float a, float b) { return (b > a || b != b) ? b : a; }

// The operations: identity() starts a thread's accumulator, apply(a, b) takes b into a
struct FoldSum {
  __device__ static double identity() { return 0.0; }
  __device__ static double apply(double a, double b) { return __dadd_rn(a, b); }
};
struct FoldNanMax {                                  // of non-negative values, so 0 is its identity
  __device__ static double identity() { return 0.0; }
  __device__ static double apply(double a, double b) { return nmax(a, b); }
  __device__ static float apply(float a, float b) { return nmax(a, b); }
};
struct FoldMin {
  __device__ static double identity() { return __longlong_as_double(0x7ff0000000000000LL); }
  __device__ static double apply(double a, double b) { return b < a ? b : a; }
};
struct FoldMax {
  __device__ static double identity() { return -__longlong_as_double(0x7ff0000000000000LL); }
  __device__ static double apply(double a, double b) { return b > a ? b : a; }
};

// over the 64 lanes of a full wave; lane 0 holds the result
template <class Op, class T>
__device__ __forceinline__ T wave_fold(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = Op::apply(v, __shfl_down(v, off, 64));
  return v;
}

// init, then p[0], p[stride], ... p[(n - 1) stride] in that order
template <class Op, class T>
__device__ __forceinline__ T ordered_fold(T init, const T* p, int n, int stride = 1) {
  for (int i = 0; i < n; ++i) init = Op::apply(init, p[(size_t)i * stride]);
  return init;
}

// over the workgroup: wave_fold, then the wave results in wave order starting from red[0] (valid in thread 0).
// red holds THREADS / 64 values; calls may follow each other on the same red.
template <class Op, int THREADS>
__device__ __forceinline__ double block_fold(double v, double* red) {
  v = wave_fold<Op>(v);
  __syncthreads();                                  // red may still be read from the previous fold
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
  if (threadIdx.x == 0) t = ordered_fold<Op>(t, red + 1, THREADS / 64 - 1);
  return t;
}

// a[c] = Ops_c::apply(a[c], b(c)) for every column c
template <class... Ops, class Rhs>
__device__ __forceinline__ void fold_columns(double* a, Rhs b) {
  int c = 0;
  ((a[c] = Ops::apply(a[c], b(c)), ++c), ...);
}

// One workgroup of THREADS folds sizeof...(Ops) columns of nblk partials, column c with Ops_c: thread t takes
// load(b, c) for b = t, t + THREADS, ... in order from the identity, then the pairwise tree in tree[THREADS][W >= C].
// The results are tree[0][c], for thread 0.
template <int THREADS, class... Ops, class Load, int W>
__device__ __forceinline__ void strided_tree_fold(Load load, long nblk, double (*tree)[W]) {
  constexpr int C = sizeof...(Ops);
  static_assert(C <= W, "tree rows hold every column");
  const int t = threadIdx.x;
  double f[C] = {Ops::identity()...};
  for (long b = t; b < nblk; b += THREADS) fold_columns<Ops...>(f, [&](int c) { return load(b, c); });
#pragma unroll
  for (int c = 0; c < C; ++c) tree[t][c] = f[c];
  __syncthreads();
  for (int half = THREADS / 2; half > 0; half >>= 1) {
    if (t < half) fold_columns<Ops...>(tree[t], [&](int c) { return tree[t + half][c]; });
    __syncthreads();
  }
}

// thread t's part of chunk_fold: partials [t ch, (t + 1) ch) with ch = ceil(nblk / THREADS), in order from the identity
template <int THREADS, class Op, class Load>
__device__ __forceinline__ double chunk_partial(Load load, long nblk) {
  const long ch = (nblk + THREADS - 1) / THREADS;
  const long lo = threadIdx.x * ch < nblk ? threadIdx.x * ch : nblk, hi = lo + ch < nblk ? lo + ch : nblk;
  double s = Op::identity();
  for (long b = lo; b < hi; ++b) s = Op::apply(s, load(b));
  return s;
}

// One workgroup of THREADS folds nblk partials: chunk_partial, then the chunk results in thread order from the identity
// (valid in thread 0).  red holds THREADS values and must be free on entry.
template <int THREADS, class Op, class Load>
__device__ __forceinline__ double chunk_fold(Load load, long nblk, double* red) {
  red[threadIdx.x] = chunk_partial<THREADS, Op>(load, nblk);
  __syncthreads();
  return threadIdx.x == 0 ? ordered_fold<Op>(Op::identity(), red, THREADS) : Op::identity();
}

// block partials cross workgroups (and XCDs, whose L2s are private) inside one launch: agent-scope accesses
__device__ __forceinline__ void put(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double get(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// For thread 0 alone, after a __syncthreads(): true in the last workgroup of the launch to get here, which has then seen
// what every other one did before its own ticket.  The ticket word is 0 between launches.
__device__ __forceinline__ bool last_ticket(void* ticket_word) {
  unsigned long long* ticket = reinterpret_cast<unsigned long long*>(ticket_word);
  __threadfence();
  const bool last = atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1;
  if (last) *ticket = 0;
  return last;
}

// True in every thread of the last workgroup to get here, after which it may read what the others put()
__device__ __forceinline__ bool last_block(double* ticket_word, int* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = last_ticket(ticket_word);
    __threadfence();
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

// the host tail of a launcher: 0, or -(the HIP error) of the launch just made
static inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
