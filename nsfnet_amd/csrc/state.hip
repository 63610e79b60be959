// Training-state snapshots: gather up to STATE_MAX_SEG device buffers of any size into one
// staging buffer (pack) or scatter the staging buffer back into the live buffers (unpack), and digest every segment, in
// one launch.  A segment's digest reads its bytes as little-endian 32-bit words w_0 .. w_{n-1}:
//   A = sum w_i mod 2^64        B = sum (i + 1) w_i mod 2^64
// Modular integer sums: the result does not depend on the order, the grid or who adds what (no float atomics, nothing
// to round).  pinn_state_digest_host is the same function on host memory.
//   state_copy_kernel<PAD>   one template for both directions.  The segment table comes by value in the kernel
//                            arguments.  Every segment is cut into chunks of kChunk bytes; the chunks of all segments
//                            form one index space that a bounded grid strides over, so a 100 MB history and an 8-byte
//                            counter share the launch and no workgroup is spent on an empty or tiny segment beyond its
//                            one chunk.  A chunk moves by 16-byte accesses when the read and the write pointer are both
//                            16-byte aligned (chunk offsets are multiples of kChunk, so the segment's pointers decide),
//                            else, and for a tail, by 4-byte ones.  A workgroup's chunks ascend, so it meets each
//                            segment in one run: it folds that run's (A, B) and puts one partial per (segment,
//                            workgroup); the last workgroup to finish (the ticket of fixed_fold.h) adds the partials of
//                            exactly the workgroups that met each segment.  PAD: the workgroup that moves a segment's
//                            last chunk zeroes the `pad` bytes behind it (up to the next multiple of 256).
// All index arithmetic is 64-bit.
#include "fixed_fold.h"
#include "kernels.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr u64 kChunk = 16384;                      // bytes: four 16-byte accesses per thread
constexpr int kMaxBlocks = 1024;                   // grid cap (4 workgroups per CU): beyond it the chunk loop repeats
// scratch, in 8-byte words: [0] ticket [1] - ; then the partials (A, B) of (segment k, workgroup b) at kPart + 2 (k kMaxBlocks + b)
constexpr int kTicket = 0, kPart = 2;
constexpr size_t kScratchWords = kPart + (size_t)2 * STATE_MAX_SEG * kMaxBlocks;

__host__ __device__ inline u64 chunks_of(u64 bytes) { return (bytes + kChunk - 1) / kChunk; }

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ void put_word(double* p, u64 v) { put(p, __longlong_as_double((long long)v)); }
__device__ __forceinline__ u64 get_word(const double* p) { return (u64)__double_as_longlong(get(p)); }

// one word of the chunk: l1 = its index in the chunk + 1 (at most kChunk / 4, so l1 w < 2^44)
__device__ __forceinline__ void take(unsigned w, unsigned l1, u64& a, u64& b) {
  a += w;
  b += (u64)l1 * w;
}

template <bool PAD>
__global__ __launch_bounds__(kThreads) void state_copy_kernel(StateArgs a) {
  __shared__ u64 red[2 * kWaves];
  __shared__ int flag;
  const unsigned t = threadIdx.x;
  int k = 0;                                        // the segment of the current run (uniform in the workgroup)
  bool open = false;
  u64 A = 0, B = 0;                                 // this thread's share of the run's digest

  // the run of segment k ends: fold it over the workgroup and put the partial
  auto flush = [&]() {
    const u64 wa = wave_sum(A), wb = wave_sum(B);
    __syncthreads();                                // red may still be read from the previous flush
    if ((t & 63) == 0) { red[2 * (t >> 6)] = wa; red[2 * (t >> 6) + 1] = wb; }
    __syncthreads();
    if (t == 0) {
      u64 sa = 0, sb = 0;
      for (int w = 0; w < kWaves; ++w) { sa += red[2 * w]; sb += red[2 * w + 1]; }
      double* p = a.scratch + kPart + 2 * ((size_t)k * kMaxBlocks + blockIdx.x);
      put_word(p, sa);
      put_word(p + 1, sb);
    }
    A = B = 0;
  };

  for (u64 c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    int k2 = k;
    while (k2 < a.nseg - 1 && c >= a.seg[k2].chunk0 + chunks_of(a.seg[k2].bytes)) ++k2;      // c < nchunks: some segment holds it
    if (k2 != k) {
      if (open) flush();
      k = k2;
    }
    open = true;
    const u64 bytes = a.seg[k].bytes;
    const u64 off = (c - a.seg[k].chunk0) * kChunk;                        // of the chunk in the segment
    const u64 len = bytes - off < kChunk ? bytes - off : kChunk;            // a multiple of 4
    const char* rd = static_cast<const char*>(a.seg[k].rd) + off;
    char* wr = a.seg[k].wr ? static_cast<char*>(a.seg[k].wr) + off : nullptr;
    const unsigned nw = (unsigned)(len / 4);
    u64 ca = 0, cb = 0;                                                     // of this chunk, indices from the chunk's start
    unsigned w0 = 0;                                                        // words moved by 16-byte accesses
    if (((reinterpret_cast<uintptr_t>(rd) | reinterpret_cast<uintptr_t>(wr)) & 15) == 0) {
      const unsigned nq = nw / 4;
      for (unsigned q = t; q < nq; q += kThreads) {
        const uint4 v = reinterpret_cast<const uint4*>(rd)[q];
        if (wr) reinterpret_cast<uint4*>(wr)[q] = v;
        take(v.x, 4 * q + 1, ca, cb);
        take(v.y, 4 * q + 2, ca, cb);
        take(v.z, 4 * q + 3, ca, cb);
        take(v.w, 4 * q + 4, ca, cb);
      }
      w0 = nq * 4;
    }
    for (unsigned i = w0 + t; i < nw; i += kThreads) {                      // unaligned pointers, and tails
      const unsigned v = reinterpret_cast<const unsigned*>(rd)[i];
      if (wr) reinterpret_cast<unsigned*>(wr)[i] = v;
      take(v, i + 1, ca, cb);
    }
    A += ca;
    B += cb + (off / 4) * ca;                                               // (off / 4 + l + 1) w = (off / 4) w + (l + 1) w
    if (PAD && wr && off + len == bytes) {                                  // the padding behind the segment: < 256 bytes
      const unsigned pad = (unsigned)(a.seg[k].pad / 4);
      if (t < pad) reinterpret_cast<unsigned*>(wr + len)[t] = 0u;
    }
  }
  if (open) flush();

  if (!last_block(a.scratch + kTicket, &flag)) return;
  // segment k was met by min(its chunks, the grid) workgroups: (chunk0 + j) % grid for j below that.  One wave per
  // segment in turn; the sums are modular, so any order gives the same words.
  const u64 grid = gridDim.x;
  for (int s = t >> 6; s < a.nseg; s += kWaves) {
    const u64 nc = chunks_of(a.seg[s].bytes), met = nc < grid ? nc : grid;
    u64 sa = 0, sb = 0;
    for (u64 j = t & 63; j < met; j += 64) {
      const u64 b = (a.seg[s].chunk0 + j) % grid;
      const double* p = a.scratch + kPart + 2 * ((size_t)s * kMaxBlocks + b);
      sa += get_word(p);
      sb += get_word(p + 1);
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    if ((t & 63) == 0) { a.digests[2 * s] = sa; a.digests[2 * s + 1] = sb; }
  }
}

}  // namespace

size_t state_scratch_bytes() { return kScratchWords * 8; }

unsigned long long state_chunks(unsigned long long bytes) { return chunks_of(bytes); }

void state_digest_host(const void* p, unsigned long long bytes, unsigned long long out[2]) {
  const unsigned char* q = static_cast<const unsigned char*>(p);
  u64 A = 0, B = 0;
  for (u64 i = 0; i < bytes / 4; ++i) {
    const u64 w = (u64)q[4 * i] | (u64)q[4 * i + 1] << 8 | (u64)q[4 * i + 2] << 16 | (u64)q[4 * i + 3] << 24;
    A += w;
    B += (i + 1) * w;
  }
  out[0] = A;
  out[1] = B;
}

int launch_state_copy(const StateArgs& a, bool pad, hipStream_t s) {
  u64 blocks = a.nchunks < (u64)kMaxBlocks ? a.nchunks : (u64)kMaxBlocks;
  if (blocks < 1) blocks = 1;                       // only empty segments: the last block still writes their digests
  if (pad)
    hipLaunchKernelGGL(state_copy_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(state_copy_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  return launch_status();
}
