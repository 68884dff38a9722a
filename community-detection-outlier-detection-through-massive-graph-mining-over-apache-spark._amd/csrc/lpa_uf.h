// The concurrent union-find of lpa_cc.hip (connected components) and lpa_scan.hip (clusters of
// cores): find with path halving, link of the LARGER root under the SMALLER one.  lpa_cc.hip's
// header states the invariant, the progress argument and why relaxed agent-scope atomics
// suffice; every root is the minimum of its tree, so the flattened value is the smallest id
// of the set.  Included after lpa_device.h and lpa_algo.h.
#pragma once

#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

__device__ __forceinline__ int32_t cc_load(int32_t* p) { return __hip_atomic_load(p, LPA_RLX_AGENT); }

// root of x's tree, p = a value read from parent[x]; halves the path on the way (x's
// parent := its grandparent), x's own pointer included, so that a vertex met again shows
// a parent nearer the root -- in the end the root, which is what lets most edges of a
// large component leave at the equal-parents test
__device__ __forceinline__ int32_t cc_find(int32_t* __restrict__ parent, int32_t x, int32_t p) {
  while (p != x) {
    const int32_t gp = cc_load(parent + p);
    if (gp == p) return p;
    __hip_atomic_store(parent + x, gp, LPA_RLX_AGENT);
    x = gp;
    p = cc_load(parent + x);
  }
  return x;
}

// join the trees of u and w; a, b = values read from parent[u], parent[w]
__device__ __forceinline__ void cc_link(int32_t* __restrict__ parent, int32_t u, int32_t a, int32_t w, int32_t b) {
  while (true) {
    const int32_t ru = cc_find(parent, u, a), rw = cc_find(parent, w, b);
    if (ru == rw) return;
    const int32_t hi = ru > rw ? ru : rw, lo = ru > rw ? rw : ru;
    int32_t expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, LPA_RLX_AGENT)) return;
    u = hi;   // hi was linked meanwhile: go on from its new parent (< hi)
    a = expect;
    w = lo;
    b = cc_load(parent + lo);
  }
}

// One edge: skipped early when it is a self-loop or both endpoints already show the same
// parent.
__device__ __forceinline__ void cc_union(int32_t* __restrict__ parent, int32_t u, int32_t w) {
  if (u == w) return;
  const int32_t a = cc_load(parent + u), b = cc_load(parent + w);
  if (a != b) cc_link(parent, u, a, w, b);
}

// after the kernel that links: parent[] is final, read with plain loads
__device__ __forceinline__ int32_t cc_root(const int32_t* __restrict__ parent, int32_t v) {
  int32_t x = v, p = parent[x];
  while (p != x) {
    x = p;
    p = parent[x];
  }
  return x;
}

}  // namespace lpa
