// What the tally stage (in lpa_iter.hip) and the refresh stage (lpa_refresh.hip) share
// beyond lpa_device.h: the 2-bit giant-code format, the rebuild test, the bin bounds a
// kernel takes by value, and the grid cap of their launches.  Included by those two
// files only; the unnamed namespace keeps every item internal to each of them, as it was
// in the one file they came from (and keeps the kernels' mangled names).
#pragma once

#include "lpa_internal.h"

namespace lpa {
namespace {

// the bin bounds bin_begin[0 .. LPA_NBINS] as a kernel argument (k_frontier_lists, k_diff,
// k_code_partial_rows)
struct BinBounds {
  int64_t b[LPA_NBINS + 1];
};

// rebuild al[] when the changed vertices touch more than `thr` arcs (host-set)
__device__ __forceinline__ bool rebuild_wanted(const unsigned long long* counters, int64_t thr) {
  return (int64_t)counters[1] > thr;
}

// ---------------------------------------------------------------------------
// Giant codes (round 5): the refresh after superstep 1 without the labels-mode al[]
// rebuild.  On R-MAT the labels L1 of superstep 1 already have a giant label G (the
// label of ~97 % of the 1,024 top hubs, ~37 % of the arcs' columns) but not on half the
// hot slots, so that refresh gathered a full 4-B label per arc (C3: 2.35 ms, 3.6x its
// algorithmic bytes in L2-missing lines), and superstep 2 read them back only to
// decide nearly every row for G: a row's G votes above every bucket of a label hash of
// its other votes make G its strict mode (giant_count; oracle, R-MAT-22: 98 % of the
// arcs sit in rows so decided with 16 buckets, 100 % of the rows above 64 arcs).
// A bucket only needs a FUNCTION of the label -- and three buckets suffice (oracle,
// R-MAT-21 superstep 2: rows of 65-1024 arcs holding 99.9 % of their arcs, every hub row,
// 90 % of the 9-64-arc rows' arcs decided; 63 buckets: 100 / 100 / 99.4 %) -- so the
// refresh writes 2-bit codes, 0 = (label == G), else 1 + a hash of the label mod 3:
//   code2     per slot, 16 to a word (k_code_build): 4 MB at C3, one XCD's L2
//   al2[i]    per arc of the rows above the cut, code2[col[i]], 16 arcs to a word
//             (k_code_rebuild; the 655,360 hottest slots' codes in LDS)
//   al[i]     per arc of the rows below the cut (code_lbin: <= 64 arcs on a label vector
//             of <= 64 MB, else <= 8), their labels
// and superstep 2 decides the hub rows (k_lpa_units_code2 + k_hub_decide) and the rows of
// the other coded rows (k_code_settle) by popcounts of the code words -- no
// table, no atomics; only the rows left undecided get their al[] entries gathered
// (k_code_partial_*) and are tallied exactly, in list mode.  Exact for any G and any hash
// (a label's count is at most its bucket's); gword[GW_CODE] marks the refresh taken, so the
// labels-mode rebuild is skipped and superstep 2's refresh rebuilds al[] whatever the
// change count.
// (Round 5 first shipped 8-bit codes with 64-bucket LDS histograms: C3 code rebuild 1.41
// ms, code settle 0.63 ms -- the histogram atomics and the 16 MB code array's L2 misses.)
// ---------------------------------------------------------------------------
__device__ __forceinline__ u32 giant_code2(u32 x, u32 G) {
  return x == G ? 0u : 1u + ((((x * 0x9E3779B1u) >> 24) * 3u) >> 8);
}

// the four codes' counts among the fields of w whose low bits fm selects:
// c0 | c1 << 16 (x) and c2 | c3 << 16 (y)
__device__ __forceinline__ void code2_counts(u32 w, u32 fm, u32& x, u32& y) {
  const u32 lo = w & fm, hi = (w >> 1) & fm;
  x += (u32)__popc(fm & ~(lo | hi)) | ((u32)__popc(lo & ~hi) << 16);
  y += (u32)__popc(hi & ~lo) | ((u32)__popc(lo & hi) << 16);
}
// low bits of the fields of word wi that hold arcs [b, e)
__device__ __forceinline__ u32 code2_fmask(int64_t wi, int64_t b, int64_t e) {
  const int64_t base = wi * 16;
  const int64_t l0 = b - base, h0 = e - base;
  const int lo = (int)(l0 < 0 ? 0 : l0 > 16 ? 16 : l0), hi = (int)(h0 < 0 ? 0 : h0 > 16 ? 16 : h0);
  const u32 mh = hi >= 16 ? 0xFFFFFFFFu : ((1u << (2 * hi)) - 1u);
  const u32 ml = lo >= 16 ? 0xFFFFFFFFu : ((1u << (2 * lo)) - 1u);
  return mh & ~ml & 0x55555555u;
}
// G decided from summed counts: its votes above every bucket
__device__ __forceinline__ bool code2_decided(u32 x, u32 y) {
  const u32 c0 = x & 0xFFFFu, c1 = x >> 16, c2 = y & 0xFFFFu, c3 = y >> 16;
  return c0 > max(c1, max(c2, c3));
}
__device__ __forceinline__ u32 spread16(u32 v) {
  v = (v | (v << 8)) & 0x00FF00FFu;
  v = (v | (v << 4)) & 0x0F0F0F0Fu;
  v = (v | (v << 2)) & 0x33333333u;
  return (v | (v << 1)) & 0x55555555u;
}
// the 2-bit codes r[k] of arcs b + 64 k + lane (b a multiple of 512) -> 32 words at
// al2[b / 16 ..): two ballots per chunk, lane l < 32 assembles word l (chunk l / 4)
__device__ __forceinline__ void store_code2(uint32_t* __restrict__ al2, int64_t b, const int32_t (&r)[8], int lane) {
  u64 m0 = 0, m1 = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const u64 b0 = __ballot(r[k] & 1), b1 = __ballot((r[k] >> 1) & 1);
    if ((lane >> 2) == k) {
      m0 = b0;
      m1 = b1;
    }
  }
  const int sh = (lane & 3) * 16;
  const u32 w = spread16((u32)(m0 >> sh) & 0xFFFFu) | (spread16((u32)(m1 >> sh) & 0xFFFFu) << 1);
  if (lane < 32) al2[(b >> 4) + lane] = w;
}

// grid of a grid-stride launch: `want` blocks, at least one and at most `cap`
inline unsigned cap_grid(int64_t want, int64_t cap) {
  if (want < 1) want = 1;
  return (unsigned)(want < cap ? want : cap);
}

}  // namespace
}  // namespace lpa
