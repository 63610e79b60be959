// Learning-rate schedules and global-norm gradient clipping for the Adam stages.  Both live on
// the device so that a captured training step replays with no host scalar changing between steps:
//   grad_sqnorm_kernel   the fp64 sum of squares of up to two fp32 vectors (main net, entropy net) into scratch[0]:
//                        grid-stride loop of 16-byte loads, block_fold, per-block partials (vector 0's blocks numbered
//                        before vector 1's); the last block to finish folds them by strided_tree_fold (fixed_fold.h).
//                        No float atomics.
//   adam_sched_kernel    adam_dev_kernel (misc.hip; the update body of both is adam_update, optim.h) with lr = the fp32 value of lr_e (optim.h) at the epoch counter e
//                        read from device memory and, when a squared norm is given, the gradient scaled by the
//                        clip_grad_norm_ coefficient.  Its last workgroup advances Adam's t, on request e, and
//                        writes the record.
#include "fixed_fold.h"
#include "optim.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                            // entries per thread and iteration: one 16-byte load
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBlocksVec = 256;                 // grid cap per vector: beyond kMaxBlocksVec * kTile entries the loop repeats
// scratch, in doubles: [0] the sum [1] ticket [2..7] - then [2 * kMaxBlocksVec] block partials
constexpr int kTicket = 1, kPart = 8;
constexpr int kScratchDoubles = kPart + 2 * kMaxBlocksVec;

__host__ __device__ inline long blocks_of(long n) {
  const long b = (n + kTile - 1) / kTile;
  return b < kMaxBlocksVec ? b : kMaxBlocksVec;
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_kernel(const float* __restrict__ g0, long n0,
                                                               const float* __restrict__ g1, long n1, double* scratch) {
  __shared__ double red[kThreads / 64];
  __shared__ double tree[kThreads][1];
  __shared__ int flag;
  const long nb0 = blocks_of(n0);
  const bool second = (long)blockIdx.x >= nb0;
  const float* __restrict__ g = second ? g1 : g0;
  const long n = second ? n1 : n0;
  const long nb = second ? (long)gridDim.x - nb0 : nb0, b = second ? (long)blockIdx.x - nb0 : (long)blockIdx.x;
  const bool aligned = reinterpret_cast<uintptr_t>(g) % 16 == 0;
  double acc = 0.0;
  for (long base = (b * kThreads + threadIdx.x) * kPer; base < n; base += nb * kTile) {
    float q[kPer] = {0.f, 0.f, 0.f, 0.f};           // entries past n add an exact 0
    if (aligned && base + kPer <= n) {
      const float4 t = *reinterpret_cast<const float4*>(g + base);
      q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (base + j < n) q[j] = g[base + j];
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) acc += (double)q[j] * (double)q[j];      // the product is exact in fp64
  }
  acc = block_fold<FoldSum, kThreads>(acc, red);
  if (threadIdx.x == 0) put(scratch + kPart + blockIdx.x, acc);
  if (!last_block(scratch + kTicket, &flag)) return;
  strided_tree_fold<kThreads, FoldSum>([&](long k, int) { return get(scratch + kPart + k); }, (long)gridDim.x, tree);
  if (threadIdx.x == 0) scratch[0] = tree[0][0];
}

template <bool CLIP>
__global__ void adam_sched_kernel(AdamSchedArgs a) {
  const long long e = __atomic_load_n(a.epoch, __ATOMIC_RELAXED);
  const float lr = (float)lr_schedule_value(a.sched, a.lr0, e);
  double norm = 0.0;
  float coef = 1.f;
  if (CLIP) {
    norm = sqrt(a.sq[0]);
    const double c = a.max_norm / (norm + 1e-6);
    coef = (float)(c > 1.0 ? 1.0 : c);              // a NaN norm stays NaN
  }
  float step_size, bc2_sqrt;
  adam_bias_correction(lr, a.b1, a.b2, a.step_counter, step_size, bc2_sqrt);
  adam_update<CLIP>(a.p, a.g, a.m, a.v, blockIdx.x * (long)blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x,
                    a.n, step_size, a.b1, a.b2, a.eps, bc2_sqrt, coef);
  // the last workgroup to get here has seen every other one read both counters: it advances them
  __syncthreads();
  if (threadIdx.x == 0 && last_ticket(a.step_counter + 1)) {
    a.step_counter[0] = a.step_counter[0] + 1;
    a.record[0] = (double)e;
    a.record[1] = (double)lr;
    a.record[2] = norm;
    a.record[3] = (double)coef;
    if (a.advance) {
      a.epoch[0] = e + 1;
      if (coef < 1.f) a.record[4] += 1.0;
      a.record[5] += 1.0;
    }
  }
}

}  // namespace

size_t grad_sqnorm_scratch_bytes() { return (size_t)kScratchDoubles * sizeof(double); }

int launch_grad_sqnorm(const float* g0, long n0, const float* g1, long n1, double* scratch, hipStream_t s) {
  const long blocks = blocks_of(n0) + (n1 > 0 ? blocks_of(n1) : 0);      // <= 2 kMaxBlocksVec partials
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, g0, n0, g1, n1, scratch);
  return launch_status();
}

int launch_adam_sched(const AdamSchedArgs& a, hipStream_t s) {
  if (a.n <= 0) return 0;
  int blocks = (int)((a.n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  if (a.sq) hipLaunchKernelGGL(adam_sched_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(adam_sched_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
  return launch_status();
}
