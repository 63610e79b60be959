// Stochastic mini-batching of the collocation term: the store of N points stays resident, a
// batch of B points is drawn from it on the device for every Adam evaluation.  Two kernels, all in integers:
//   batch_draw_kernel     slot j draws one index from stratum [floor(j N / B), floor((j + 1) N / B)) with word 0 of
//                         Philox4x32-10 (counter (j, t), key (seed, rank)), writes it to idx and gathers x, y, w and
//                         vis_t_minus of that point into the batch buffers; the last workgroup to finish advances
//                         the draw counter t, which lives in device memory (as adam_dev_kernel keeps its step count)
//   batch_scatter_kernel  the batch's updated vis_t_minus back to the store at idx (distinct indices: no atomics)
// They move about 40 bytes per drawn point and are launch-bound: one launch each, not one per array.
#include "kernels.h"

namespace {

constexpr int kThreads = 256;

// Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011), word 0 of the output block
__device__ __forceinline__ unsigned philox4x32_10_w0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                     unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += W0; k1 += W1;
  }
  return c0;
}

__global__ __launch_bounds__(kThreads) void batch_draw_kernel(BatchDrawArgs a) {
  const unsigned long long t = (unsigned long long)__atomic_load_n(a.counter, __ATOMIC_RELAXED);
  const unsigned long long j = blockIdx.x * (unsigned long long)kThreads + threadIdx.x;
  if (j < (unsigned long long)a.b) {
    const unsigned long long n = (unsigned long long)a.n, b = (unsigned long long)a.b;
    const unsigned long long lo = j * n / b, hi = (j + 1) * n / b;      // j, n <= 2^30: no overflow
    const unsigned r = philox4x32_10_w0((unsigned)j, (unsigned)(j >> 32), (unsigned)t, (unsigned)(t >> 32), a.seed,
                                        a.rank);
    const unsigned long long i = lo + __umulhi(r, (unsigned)(hi - lo));   // lo <= i < hi <= n
    a.idx[j] = (long long)i;
    a.dx[j] = a.sx[i];
    a.dy[j] = a.sy[i];
    if (a.sw) a.dw[j] = a.sw[i];
    if (a.sv) a.dv[j] = a.sv[i];
  }
  // the last workgroup to get here has seen every other one read the counter: it advances it
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* ticket = reinterpret_cast<unsigned long long*>(a.counter + 1);
    __threadfence();
    if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1) {
      *ticket = 0;
      a.counter[0] = (long long)(t + 1);
    }
  }
}

__global__ __launch_bounds__(kThreads) void batch_scatter_kernel(const long long* __restrict__ idx, long b, long n,
                                                                 const float* __restrict__ src,
                                                                 float* __restrict__ dst) {
  const long j = blockIdx.x * (long)kThreads + threadIdx.x;
  if (j >= b) return;
  const long long i = idx[j];
  if (i >= 0 && i < n) dst[i] = src[j];
}

}  // namespace

int launch_batch_draw(const BatchDrawArgs& a, hipStream_t s) {
  const int blocks = (int)((a.b + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(batch_draw_kernel, dim3(blocks), dim3(kThreads), 0, s, a);
  return launch_status();
}

int launch_batch_scatter(const long long* idx, long b, long n, const float* src, float* dst, hipStream_t s) {
  const int blocks = (int)((b + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(batch_scatter_kernel, dim3(blocks), dim3(kThreads), 0, s, idx, b, n, src, dst);
  return launch_status();
}
