// What the algorithm calls (lpa_cc.hip .. lpa_kcore.hip, lpa_adj.hip, lpa_outlier.hip) share
// on the host side of a launch: grid sizes, loop macros, the call-scoped temporaries and
// the radix sort's shift table.  Included after lpa_device.h.
#pragma once

#include "lpa_device.h"

namespace lpa {

inline unsigned grid_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > 65536) b = 65536;
  return (unsigned)b;
}
// block-aggregated / block-reduced passes: few blocks, each over a long stretch of the input;
// a grid that depends on n alone (the reductions' shape)
inline unsigned grid_bh(int64_t n) {
  const unsigned g = grid_for(n);
  return g < 2048u ? g : 2048u;
}
// per_block rows to a block, at most cap blocks
inline unsigned grid_rows(int64_t nrows, int per_block, int64_t cap) {
  int64_t b = (nrows + per_block - 1) / per_block;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

#define GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)
// the whole block runs every trip (ballots, shuffles and barriers inside)
#define BLOCK_STRIDE(b, n) \
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x; b < (n); b += (int64_t)gridDim.x * blockDim.x)

// order and scope of the atomics on words that other CUs touch inside the same kernel
#define LPA_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

typedef unsigned long long ull;

constexpr int kShortLanes = 8;      // lanes per row of the short forms
constexpr int kBlockThreads = 1024; // threads per row of the block forms

// Stream-ordered temporaries of one call, and its pinned host words; all freed by the destructor.
struct Tmp {
  static constexpr int kCap = 64;
  hipStream_t s;
  void* ptrs[kCap];
  int n = 0;
  void* pinned = nullptr;
  explicit Tmp(hipStream_t st) : s(st) {}
  Tmp(const Tmp&) = delete;
  Tmp& operator=(const Tmp&) = delete;
  // count <= 0 allocates one element
  template <typename T>
  int get(T** p, int64_t count) {
    if (n == kCap) {
      set_error("more than %d temporaries alive in one call", kCap);
      return LPA_EOVERFLOW;
    }
    LPA_TRY(tmp_alloc((void**)p, sizeof(T) * (size_t)(count > 0 ? count : 1), s));
    ptrs[n++] = *p;
    return LPA_OK;
  }
  // the call's one pinned host array (the counters a loop reads back)
  template <typename T>
  int pin(T** p, int64_t count) {
    if (pinned) {
      set_error("a call pins one host array");
      return LPA_EINVAL;
    }
    LPA_HIP(hipHostMalloc(&pinned, sizeof(T) * (size_t)(count > 0 ? count : 1), hipHostMallocDefault));
    *p = static_cast<T*>(pinned);
    return LPA_OK;
  }
  // frees p now (in stream order) instead of at the call's end
  void drop(void* p) {
    for (int i = 0; i < n; ++i)
      if (ptrs[i] == p) {
        tmp_free(p, s);
        ptrs[i] = ptrs[--n];
        return;
      }
  }
  ~Tmp() {
    for (int i = 0; i < n; ++i) tmp_free(ptrs[i], s);
    if (pinned) (void)hipHostFree(pinned);
  }
};

// The radix sort's 8-bit digits for u64 keys whose 32-bit halves hold values of `bits` bits:
// lo() the ns digits of the low half, hi() those of the high half, both() the 2 ns of a sort
// over the whole key (low half first: least significant digit first).
struct HalfShifts {
  int shifts[8], ns = 0;
  explicit HalfShifts(int bits) {
    for (int b = 0; b < bits; b += 8) ++ns;
    for (int i = 0; i < ns; ++i) {
      shifts[i] = 8 * i;
      shifts[ns + i] = 32 + 8 * i;
    }
  }
  const int* lo() const { return shifts; }
  const int* hi() const { return shifts + ns; }
  const int* both() const { return shifts; }
};

}  // namespace lpa
