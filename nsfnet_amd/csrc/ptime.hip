// Pseudo-time stepping of the residual loss (include/nsfnet_pinn.h "Pseudo-time stepping"): the
// per-update record and the anchor refresh.  State per local collocation point i:
//   anchor [3][npad] fp32   u*, v*, p*: the fields at i when the anchors were last refreshed
// After an optimiser update, over the planes U, V, P, EQ1..EQ3 the last evaluation left (the steady residuals) and the
// weights w (absent = 1), with du = u - u*, dv = v - v*, dp = p - p*:
//   record[0..2] = sum_i w_i eq_k^2                     the steady sums
//   record[3]    = sum_i w_i (du^2 + dv^2)
//   record[4]    = sum_i w_i dp^2
//   record[5]    = max_i max(|du|, |dv|)                NaN-propagating
//   record[6]    = updates since the last refresh, after this call
//   record[7]    = refreshes made
// Everything per point is fp64 from the fp32 inputs in exactly this order, without contraction.  When record[6] + 1 >=
// every (every >= 1), or force != 0, each thread overwrites the anchors of the quads it just read with the current U, V,
// P (whole quads of four points: the planes and the anchors are padded alike), and the last block zeroes [6] and
// increments [7]; otherwise [6] goes up by one.  The condition is read from device memory at kernel entry, before any
// block can have written it: one captured launch serves a whole stage.
// One kernel, bandwidth-bound; no float atomics, every sum has a fixed order (fixed_fold.h; bit-reproducible):
// grid-stride loop of 16-byte loads, block_fold, per-block partials, the last block to finish folds them by
// strided_tree_fold.
#include "fixed_fold.h"
#include "residual_planes.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                            // points per thread and iteration: one 16-byte load per plane
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBlocks = 512;                    // grid cap: beyond kMaxBlocks * kTile points the loop repeats
constexpr int kCols = 6;                           // the record's entries 0..5
// scratch, in doubles: [0] ticket [1..7] - [8..] partials [kMaxBlocks][kCols]
constexpr int kTicket = 0, kPart = 8;
constexpr int kScratchDoubles = kPart + kCols * kMaxBlocks;

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__global__ __launch_bounds__(kThreads) void ptime_advance_kernel(PtimeArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[kThreads / 64];
  __shared__ int flag;
  const double since = get(a.record + 6);
  const bool refresh = a.force != 0 || (a.every >= 1.0 && since + 1.0 >= a.every);
  const size_t np = (size_t)a.npad;
  double acc[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // (plain operators under the pragma: the rounding intrinsics are ordinary products and sums to the compiler, which
  // would contract w e^2 + acc into one fma)
  auto point = [&](float e1, float e2, float e3, float u, float v, float p, float ua, float va, float pa, float wf) {
    const double w = (double)wf;
    const double s1 = w * sq(e1), s2 = w * sq(e2), s3 = w * sq(e3);
    acc[0] = acc[0] + s1; acc[1] = acc[1] + s2; acc[2] = acc[2] + s3;
    const double du = (double)u - (double)ua, dv = (double)v - (double)va, dp = (double)p - (double)pa;
    const double du2 = du * du, dv2 = dv * dv, dp2 = dp * dp;
    const double d2 = du2 + dv2;
    const double s4 = w * d2, s5 = w * dp2;
    acc[3] = acc[3] + s4; acc[4] = acc[4] + s5;
    acc[5] = nmax(nmax(acc[5], fabs(du)), fabs(dv));
  };
  for (long base = ((long)blockIdx.x * kThreads + threadIdx.x) * kPer; base < a.n; base += (long)gridDim.x * kTile) {
    // base % 4 == 0 and base < n <= npad, npad % 4 == 0: the planes' and the anchors' quads are in bounds
    const float4 e1 = load4(a.fld + FLD_EQ1 * np + base), e2 = load4(a.fld + FLD_EQ2 * np + base);
    const float4 e3 = load4(a.fld + FLD_EQ3 * np + base);
    const float4 u = load4(a.fld + FLD_U * np + base), v = load4(a.fld + FLD_V * np + base);
    const float4 p = load4(a.fld + FLD_P * np + base);
    const float4 ua = load4(a.anchor + base), va = load4(a.anchor + np + base), pa = load4(a.anchor + 2 * np + base);
    float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
    if (a.w) {
      if (base + kPer <= a.n) {
        w = load4(a.w + base);
      } else {                                     // the ragged tail: w has n entries
        w.x = a.w[base];
        if (base + 1 < a.n) w.y = a.w[base + 1];
        if (base + 2 < a.n) w.z = a.w[base + 2];
      }
    }
    point(e1.x, e2.x, e3.x, u.x, v.x, p.x, ua.x, va.x, pa.x, w.x);
    if (base + 1 < a.n) point(e1.y, e2.y, e3.y, u.y, v.y, p.y, ua.y, va.y, pa.y, w.y);
    if (base + 2 < a.n) point(e1.z, e2.z, e3.z, u.z, v.z, p.z, ua.z, va.z, pa.z, w.z);
    if (base + 3 < a.n) point(e1.w, e2.w, e3.w, u.w, v.w, p.w, ua.w, va.w, pa.w, w.w);
    if (refresh) {
      *reinterpret_cast<float4*>(a.anchor + base) = u;
      *reinterpret_cast<float4*>(a.anchor + np + base) = v;
      *reinterpret_cast<float4*>(a.anchor + 2 * np + base) = p;
    }
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) acc[c] = block_fold<FoldSum, kThreads>(acc[c], red);
  acc[5] = block_fold<FoldNanMax, kThreads>(acc[5], red);
  double* part = a.scratch + kPart;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) put(part + (size_t)blockIdx.x * kCols + c, acc[c]);
  }
  if (!last_block(a.scratch + kTicket, &flag)) return;
  __shared__ double tree[kThreads][kCols];
  strided_tree_fold<kThreads, FoldSum, FoldSum, FoldSum, FoldSum, FoldSum, FoldNanMax>(
      [&](long b, int c) { return get(part + (size_t)b * kCols + c); }, (long)gridDim.x, tree);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int c = 0; c < kCols; ++c) a.record[c] = tree[0][c];
  a.record[6] = refresh ? 0.0 : since + 1.0;
  if (refresh) a.record[7] += 1.0;
}

long ptime_blocks(long n) {
  const long b = (n + kTile - 1) / kTile;
  return b < kMaxBlocks ? b : kMaxBlocks;
}

}  // namespace

size_t ptime_scratch_bytes(long) { return (size_t)kScratchDoubles * sizeof(double); }

int launch_ptime_advance(const PtimeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ptime_advance_kernel, dim3((unsigned)ptime_blocks(a.n)), dim3(kThreads), 0, s, a);
  return launch_status();
}
