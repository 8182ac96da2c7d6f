// Everything workgroups of one launch do with each other (gfx950): agent-scope loads, the
// XCD a workgroup runs on, and the arrival barrier of the cooperative kernels (eig.hip,
// svm.hip). What a lane does with its own wave or workgroup is in wave.h.
#pragma once
#include <hip/hip_runtime.h>

// relaxed agent-scope loads: they bypass the CU's L1, so they see what other CUs of the
// same XCD stored (one L2)
__device__ __forceinline__ double ld_agent(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_agent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// HW_REG_XCC_ID (hardware register 20, offset 0, 4 bits): the XCD this wave runs on in its
// low bits. Callers mask it themselves.
__device__ __forceinline__ int xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20); }

// Spin budget of grid_arrive: iterations of load + s_sleep(1), about a second.
constexpr long kGridSpinBudget = 1L << 22;

// Arrival barrier of `target` workgroup arrivals on the counter cnt (the caller passes
// participants x number of this sync, so the counter is never reset). All threads of the
// workgroup call it. Contract:
//  * every thread's earlier stores are complete (s_waitcnt 0, then the workgroup barrier)
//    before thread 0 adds the workgroup's arrival;
//  * thread 0 spins on an agent-scope load of cnt (the callers' participants claim their
//    slots on one XCD, so counter and data live in one L2);
//  * it gives up when the spin budget runs out or when the error word err is already set,
//    and then raises err, so every other participant leaves at its next look;
//  * returns false to all threads after a failure (s_ok is one int of LDS): the caller
//    returns, and the host finds err set.
__device__ __forceinline__ bool grid_arrive(int* cnt, int target, int* err, int* s_ok) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(cnt, 1);
    int ok = 1;
    long spin = 0;
    while (ld_agent(cnt) < target) {
      if (++spin > kGridSpinBudget || ld_agent(err)) {
        ok = 0;
        atomicExch(err, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    *s_ok = ok;
  }
  __syncthreads();
  return *s_ok != 0;
}
