// Folding per-workgroup partial results inside one launch: every workgroup put()s its partial, takes a ticket, and the
// last one to arrive get()s them all.  Used by the fixed-order fp64 reductions of rba.hip and optim.hip.
#pragma once
#include <hip/hip_runtime.h>

// block partials cross workgroups (and XCDs, whose L2s are private) inside one launch: agent-scope accesses
__device__ __forceinline__ void put(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double get(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// True in every thread of the last workgroup to get here, after which it may read what the others put()
__device__ __forceinline__ bool last_block(double* ticket_word, int* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* ticket = reinterpret_cast<unsigned long long*>(ticket_word);
    __threadfence();
    const bool last = atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1;
    if (last) *ticket = 0;                          // 0 between calls
    __threadfence();
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}
