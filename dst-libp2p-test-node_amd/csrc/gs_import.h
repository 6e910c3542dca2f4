// gs_import.h — device helpers shared by the imports of a caller's graph (gs_topology.hip,
// DESIGN.md §2.1) and of a caller's mesh (gs_meshimport.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs {

// A defect is one word, kind << IMP_KIND_SHIFT | index, reduced with atomicMin: the smallest
// kind and, of that kind, the smallest index, whatever order the threads run in.
constexpr int IMP_KIND_SHIFT = 48;
constexpr uint64_t IMP_NONE = ~0ull;

__device__ inline void imp_defect(unsigned long long* err, uint64_t kind, uint64_t idx) {
  atomicMin(err, (unsigned long long)((kind << IMP_KIND_SHIFT) | idx));
}

__device__ inline uint64_t imp_mix(uint64_t x) {  // splitmix64's finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

}  // namespace gs
