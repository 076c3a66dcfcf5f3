// ksim_xchg.h — the 8-byte words the kernels exchange through memory: relaxed atomic store / load
// per scope, the class granule's fields, and a 64-bit readfirstlane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ksimx {

// A global (not flat) pointer.  The helpers below access memory through the pointer type they are
// given: a kernel whose exchange must compile to global_load / global_store casts its uint64_t* to
// gu64* at the call, the others pass the flat pointer.
typedef __attribute__((address_space(1))) uint64_t gu64;

// agent scope: words exchanged between the workgroups of one device
template <class P>
__device__ __forceinline__ void store_agent(P* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class P>
__device__ __forceinline__ uint64_t load_agent(P* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// system scope: fine-grained buffers written by peer devices over xGMI
template <class P>
__device__ __forceinline__ void store_system(P* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <class P>
__device__ __forceinline__ uint64_t load_system(P* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The class granule of the persistent and general persistent kernels:
// tag:8 | fit count:12 | count at max:12 | max score:32.
__device__ __forceinline__ uint32_t gtag(uint64_t v) { return (uint32_t)(v >> 56); }
__device__ __forceinline__ int32_t gfit(uint64_t v) { return (int32_t)((v >> 44) & 0xFFF); }
__device__ __forceinline__ int32_t gcnt(uint64_t v) { return (int32_t)((v >> 32) & 0xFFF); }
__device__ __forceinline__ int32_t gscore(uint64_t v) { return (int32_t)(uint32_t)v; }

// a wave-uniform 64-bit value into scalar registers
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace ksimx
