// What the kernels that enumerate triangles over the rank-oriented lists share: lpa_tc.hip
// (triangles per vertex) and lpa_scan.hip (common neighbours per edge).  The build of those
// lists is tc_build (lpa_internal.h; lpa_tc.hip's header describes it and the row forms).
// Included after lpa_device.h and lpa_algo.h.
#pragma once

#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

// is x in the ascending list p[0, n)?
template <typename P>
__device__ __forceinline__ bool tc_has(P p, int32_t n, int32_t x) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const int32_t y = p[mid];
    if (y == x) return true;
    if (y < x) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// where x lies in the ascending list p[0, n), -1 if it does not
template <typename P>
__device__ __forceinline__ int32_t tc_pos(P p, int32_t n, int32_t x) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const int32_t y = p[mid];
    if (y == x) return mid;
    if (y < x) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// LDS of one team, in 8-byte words: rpv[T] (first col[] index of each out-neighbour's
// list), pre[T + 1] (+ 1 pad: their scanned lengths), nu[cap] (N+(u), LDS forms only)
template <int T>
constexpr int64_t tc_team_words(int64_t cap) { return T + (T + 2) / 2 + (cap + 1) / 2; }

template <int T>
__device__ __forceinline__ void tc_team_sync() {
  if (T == 256) {
    __syncthreads();
  } else {
    // one wave: its LDS operations complete in order; nothing may move across
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace lpa
