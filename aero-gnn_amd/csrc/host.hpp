// Host-side helpers shared by every translation unit of the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace agn {

// Compute units of the current device, queried once per process (256 when no device answers).
// Defined in mlp.hip; hidden, so the library's exported symbols stay those of include/aerognn.h.
__attribute__((visibility("hidden"))) int cu_count();

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the status every launching entry point returns: 0, or the HIP error of the launch
static inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// Blocks of a persistent tile kernel (one per CU) for `units` tiles or rounds, `per_block` of them
// per block and walk step: every CU once there is work for all of them, else the blocks needed
// rounded up to a multiple of 8 (at least 8), so that the XCD-grouped walk (tile32.hpp Walk) applies.
static inline int tile_blocks(int units, int per_block) {
  const int cus = cu_count();
  const int need = (units + per_block - 1) / per_block;
  if (need >= cus) return cus;
  const int n = (need + 7) / 8 * 8;
  return n < 8 ? 8 : n;
}

}  // namespace agn
