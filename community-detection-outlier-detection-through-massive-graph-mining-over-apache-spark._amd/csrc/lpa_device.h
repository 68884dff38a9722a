// Device helpers shared by the superstep kernels (lpa_iter.hip, lpa_refresh.hip, lpa_hub.hip)
// and the other stages' kernels.
//
// A vote tally is packed into one 64-bit word  (count << 32) | ~label : the
// maximum word is the highest count and, among equal counts, the smallest label,
// so "mode with smallest-label tie-break"  is a plain u64
// max-reduction; an empty slot is 0 (label 0xFFFFFFFF never occurs).
#pragma once

#include "lpa_internal.h"

namespace lpa {
namespace dev {

constexpr u32 kNone = 0xFFFFFFFFu;  // empty lane

__device__ __forceinline__ u32 ld_stream(const int32_t* p) {
  return (u32)__builtin_nontemporal_load(p);
}

// ---------------------------------------------------------------------------
// Votes from a possibly sparse al[] (gword[GW_AL_SPARSE], lpa_internal.h): arc i votes Gb
// when its arc giant bit is set, al[i] otherwise.  `on` is all ones while al[] is sparse
// and 0 while it is dense: the bit word is then read at index 0 and masked off, so a
// reader issues the same loads either way (no branch around a load: the tallies' rings
// count on exact vmcnt tracking) and a dense al[] costs one cached word per chunk.
// ---------------------------------------------------------------------------
struct ArcLabels {
  const int32_t* p;
  const uint32_t* bits;
  u32 on, Gb, last;
};
__device__ __forceinline__ ArcLabels arc_labels(const ArcSrc& s) {
  ArcLabels A;
  A.p = s.p;
  A.bits = s.bits;
  A.on = s.gword[GW_AL_SPARSE] != 0 ? ~0u : 0u;
  A.Gb = (u32)s.gword[GW_AL_GB];
  A.last = s.last;
  return A;
}
// one arc's vote, both loads issued at once (the readers that use a label where they load it)
__device__ __forceinline__ u32 arc_label(const ArcLabels& A, int64_t i) {
  const u32 x = ld_stream(A.p + i);
  const u32 w = A.bits[(u32)(i >> 5) & A.on] & A.on;
  return ((w >> ((u32)i & 31u)) & 1u) ? A.Gb : x;
}
// The ring readers (a wave per row or unit, its arcs [base, base + 64 NC) lane-consecutive)
// load the bit words with the labels -- lane l the word (base >> 5) + l, 2 NC + 1 of them,
// one register per ring slot -- and apply them where the labels are tallied, so no wait
// lands between a slot's loads and its use.
template <int NC>
__device__ __forceinline__ u32 arc_bits_load(const ArcLabels& A, int64_t base, int lane) {
  const u32 l = (u32)lane < 2u * NC ? (u32)lane : 2u * NC;
  u32 idx = (u32)(base >> 5) + l;
  idx = idx < A.last ? idx : A.last;
  return A.bits[idx & A.on];
}
template <int NC>
__device__ __forceinline__ void arc_bits_apply(u32 (&lab)[NC], u32 bw, const ArcLabels& A, int64_t base) {
  if (A.on == 0u) return;  // dense (uniform; no load inside the branch): nothing to apply
  const u32 o = (u32)__builtin_amdgcn_readfirstlane((int)((u32)base & 31u));
  const u64 on = ~0ull;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const u64 w0 = (u32)__builtin_amdgcn_readlane((int)bw, 2 * c);
    const u64 w1 = (u32)__builtin_amdgcn_readlane((int)bw, 2 * c + 1);
    const u64 w2 = (u32)__builtin_amdgcn_readlane((int)bw, 2 * c + 2);
    const u64 m = ((((w1 << 32) | w0) >> o) | (((w2 << 32) << (32u - o)))) & on;
    lab[c] = __builtin_amdgcn_inverse_ballot_w64(m) ? A.Gb : lab[c];
  }
}

__device__ __forceinline__ u64 tally(u32 cnt, u32 label) {
  return ((u64)cnt << 32) | (u64)(u32)(~label);
}

__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

// Wave reductions over a FULL wave (every call site has all 64 lanes active):
// DPP within each 16-lane row (xor 1, xor 2, half-row mirror, row mirror: every
// lane ends with its row's result, VALU only, no LDS round trip), then the four
// row results via readlane (uniform result).
template <int kCtrl>
__device__ __forceinline__ u32 dpp_u32(u32 v) {
  return (u32)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}
template <int kCtrl>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
  return ((u64)dpp_u32<kCtrl>((u32)(v >> 32)) << 32) | (u64)dpp_u32<kCtrl>((u32)v);
}
__device__ __forceinline__ u64 readlane_u64(u64 v, int l) {
  return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l) << 32) |
         (u64)(u32)__builtin_amdgcn_readlane((int)(u32)v, l);
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
  v = umax64(v, dpp_u64<0xB1>(v));   // quad_perm [1,0,3,2]
  v = umax64(v, dpp_u64<0x4E>(v));   // quad_perm [2,3,0,1]
  v = umax64(v, dpp_u64<0x141>(v));  // row_half_mirror
  v = umax64(v, dpp_u64<0x140>(v));  // row_mirror
  return umax64(umax64(readlane_u64(v, 0), readlane_u64(v, 16)),
                umax64(readlane_u64(v, 32), readlane_u64(v, 48)));
}

__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
  v += dpp_u32<0xB1>(v);
  v += dpp_u32<0x4E>(v);
  v += dpp_u32<0x141>(v);
  v += dpp_u32<0x140>(v);
  return (u32)__builtin_amdgcn_readlane((int)v, 0) + (u32)__builtin_amdgcn_readlane((int)v, 16) +
         (u32)__builtin_amdgcn_readlane((int)v, 32) + (u32)__builtin_amdgcn_readlane((int)v, 48);
}

__device__ __forceinline__ u32 wave_max_u32(u32 v) {
  v = max(v, dpp_u32<0xB1>(v));
  v = max(v, dpp_u32<0x4E>(v));
  v = max(v, dpp_u32<0x141>(v));
  v = max(v, dpp_u32<0x140>(v));
  return max(max((u32)__builtin_amdgcn_readlane((int)v, 0), (u32)__builtin_amdgcn_readlane((int)v, 16)),
             max((u32)__builtin_amdgcn_readlane((int)v, 32), (u32)__builtin_amdgcn_readlane((int)v, 48)));
}
// u64 max as two 32-bit reductions (the high words, then the low words of the lanes
// holding that high word): each DPP step is one v_max_u32 instead of two moves, a
// 64-bit compare and two selects -- fewer VALU issues, a longer dependent chain, so it
// serves only the issue-bound g64 row hash (C2 60.4 -> 61.6 GTEPS; as every kernel's
// wave max, C3's latency-bound converged supersteps lost 1.5 %)
__device__ __forceinline__ u64 wave_max_u64_split(u64 v) {
  const u32 hi = wave_max_u32((u32)(v >> 32));
  const u32 lo = wave_max_u32((u32)(v >> 32) == hi ? (u32)v : 0u);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ int64_t readlane_i64(int64_t x, int l) {
  return (int64_t)readlane_u64((u64)x, l);
}

// ---------------------------------------------------------------------------
// Row spans: a wave that owns one long row reads the row's elements [i0, last] of an
// array (bit words, per-unit counts) K x 64 at a time.  span_load issues the loads of one
// step back to back and the caller masks by span_idx after them -- so the first use waits
// once and the K loads are in flight together, where a `for (i = i0 + lane; i <= last;
// i += 64)` loop pays one memory latency per 64 elements.  Inside the row's last round an
// index past `last` is clamped to `last` (in bounds); a round that lies past `last`
// altogether is not issued (a uniform branch: i0 and last are the same in every lane) and
// reads as 0 -- most hub rows are short, and K clamped rounds for a row that needs one
// measured slower than the loop they replaced (rejected table of round 13).
// The lanes address the row by a 32-bit offset from its uniform base, one register per
// load.  The row must not be empty (last >= i0 for the first step) and shorter than 2^31.
// ---------------------------------------------------------------------------
constexpr int kSpanK = 8;
template <int K, typename T>
__device__ __forceinline__ void span_load(T (&x)[K], const T* __restrict__ p, int64_t i0, int64_t last,
                                          int lane) {
  const T* __restrict__ row = p + i0;   // uniform
  const int64_t n1 = last - i0;         // uniform: the last element's offset; < 0 past the row
  const u32 cap = (u32)(n1 > 0 ? n1 : 0);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    x[k] = T(0);
    if ((int64_t)k * 64 <= n1) {        // uniform
      const u32 o = (u32)(k * 64 + lane);
      x[k] = row[o < cap ? o : cap];
    }
  }
}
// element k of this lane in the step at i0: its index, and whether it lies inside the row
__device__ __forceinline__ int64_t span_idx(int64_t i0, int k, int lane) { return i0 + k * 64 + lane; }

// Bounds off[v], off[v + 1] of 64 rows of a wave in one load pair per lane: lane k holds
// row v0 + k * stride (0, 0 past n).  A row takes its bounds by readlane (span_pair_at),
// so they are in registers long before the row's turn and no bounds load sits between
// two rows' span loads (as span_batch for the wave bins).
struct SpanPair {
  int64_t b, e;
};
__device__ __forceinline__ SpanPair span_pair_batch(const int64_t* __restrict__ off, int64_t v0, int64_t stride,
                                                    int64_t n, int lane) {
  SpanPair s;
  s.b = s.e = 0;
  const int64_t v = v0 + (int64_t)lane * stride;
  if (v < n) {
    s.b = off[v];
    s.e = off[v + 1];
  }
  return s;
}
__device__ __forceinline__ SpanPair span_pair_at(const SpanPair& s, int q) {
  SpanPair r;
  r.b = readlane_i64(s.b, q);
  r.e = readlane_i64(s.e, q);
  return r;
}

// A hub row's giant-decision sums over its units [u0, u1) (k_lpa_units_giant /
// k_lpa_units_code2 left ugc[u] = the unit's G votes, umx[u] = its rivals' bound): wave
// sums of ugc (sg) and of umx, whole (sm) and as the three 10-bit bucket counts of the
// 2-bit codes (s1..s3).  Each is at most the row's degree (< 2^31), so 32 bits hold it.
// Called by a full wave; 2 x kSpanK loads in flight per 512 units.
struct UnitSums {
  u32 sg, sm, s1, s2, s3;
};
__device__ __forceinline__ UnitSums span_unit_sums(const uint32_t* __restrict__ ugc,
                                                   const uint32_t* __restrict__ umx, int64_t u0, int64_t u1,
                                                   int lane) {
  constexpr int K = kSpanK;
  UnitSums r = {0u, 0u, 0u, 0u, 0u};
  if (u1 > u0) {  // uniform (a hub row has >= 2 units; span_load needs a last element)
#pragma unroll 1
    for (int64_t i0 = u0; i0 < u1; i0 += K * 64) {
      u32 g[K], m[K];
      span_load<K>(g, ugc, i0, u1 - 1, lane);
      span_load<K>(m, umx, i0, u1 - 1, lane);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const bool in = span_idx(i0, k, lane) < u1;
        const u32 mm = in ? m[k] : 0u;
        r.sg += in ? g[k] : 0u;
        r.sm += mm;
        r.s1 += mm & 1023u;
        r.s2 += (mm >> 10) & 1023u;
        r.s3 += mm >> 20;
      }
    }
  }
  r.sg = wave_sum_u32(r.sg);
  r.sm = wave_sum_u32(r.sm);
  r.s1 = wave_sum_u32(r.s1);
  r.s2 = wave_sum_u32(r.s2);
  r.s3 = wave_sum_u32(r.s3);
  return r;
}

__device__ __forceinline__ u32 hash_slot(u32 label, int shift) {
  return (label * 0x9E3779B1u) >> shift;
}

__device__ __forceinline__ int ceil_log2(u32 x) { return x <= 1 ? 0 : 32 - __clz(x - 1); }

// Insert `cnt` votes for `label` into an LDS open-addressing table of (mask+1)
// slots (never full: callers size it >= 2x the distinct labels).  Returns the
// slot index when this call claimed an empty slot, else -1.
__device__ __forceinline__ int lds_insert(u64* tab, int shift, u32 mask, u32 label, u32 cnt) {
  const u32 key = ~label;
  u32 h = hash_slot(label, shift);
  while (true) {
    u64 old = atomicCAS(&tab[h], 0ull, ((u64)cnt << 32) | key);
    if (old == 0ull) return (int)h;
    if ((u32)old == key) {
      atomicAdd(&tab[h], (u64)cnt << 32);
      return -1;
    }
    h = (h + 1u) & mask;
  }
}

// Bounded variant for tables whose load is not guaranteed by construction: after
// a full sweep it raises bit 2 of *err and drops the vote.
__device__ __forceinline__ int lds_insert_bounded(u64* tab, int shift, u32 mask, u32 label, u32 cnt,
                                                  int32_t* err) {
  const u32 key = ~label;
  u32 h = hash_slot(label, shift);
  for (u32 probe = 0; probe <= mask; ++probe) {
    u64 old = atomicCAS(&tab[h], 0ull, ((u64)cnt << 32) | key);
    if (old == 0ull) return (int)h;
    if ((u32)old == key) {
      atomicAdd(&tab[h], (u64)cnt << 32);
      return -1;
    }
    h = (h + 1u) & mask;
  }
  atomicOr(err, 2);
  return -1;
}

// Continue an LDS insert of `word` whose probe at slot h hit another key (the tally
// kernels' wave-owned tables, never full; lds_probe_word<false> below is the same walk
// with the error word's plumbing, kept apart so that those kernels' code stays as it is).
__device__ __forceinline__ int lds_probe(u64* tab, u32 mask, u64 word, u32 h) {
  const u32 key = (u32)word;
  while (true) {
    h = (h + 1u) & mask;
    const u64 old = atomicCAS(&tab[h], 0ull, word);
    if (old == 0ull) return (int)h;
    if ((u32)old == key) {
      atomicAdd(&tab[h], word & 0xFFFFFFFF00000000ull);
      return -1;
    }
  }
}

// Continue the insert of tally word `word` (count << 32 | ~label) whose first
// probe at slot h hit another key: linear probing.  Returns the claimed slot or
// -1 (merged into an existing key).  kBounded: give up after a full sweep, raise
// bit 2 of *err and drop the votes (tables whose load is not bounded by design).
template <bool kBounded>
__device__ __forceinline__ int lds_probe_word(u64* tab, u32 mask, u64 word, u32 h, int32_t* err) {
  const u32 key = (u32)word;
  for (u32 probe = 0; !kBounded || probe < mask; ++probe) {
    h = (h + 1u) & mask;
    const u64 old = atomicCAS(&tab[h], 0ull, word);
    if (old == 0ull) return (int)h;
    if ((u32)old == key) {
      atomicAdd(&tab[h], word & 0xFFFFFFFF00000000ull);
      return -1;
    }
  }
  atomicOr(err, 2);
  return -1;
}

// Batched insert of NC chunks of tally words (this lane inserts wv[c] when bit c of
// its `lmask` is set): every first-probe CAS is issued before any is resolved, so
// NC independent LDS atomics per lane are in flight instead of one dependent chain
// per word; a key match adds the count (no return value), a collision probes on.
// slot[c] = the slot this lane claimed, or -1.
template <int NC, bool kBounded = false>
__device__ __forceinline__ void insert_words(u64* tab, int shift, u32 mask, const u64 (&wv)[NC],
                                             u32 lmask, int (&slot)[NC], int32_t* err) {
  u64 old[NC];
  u32 hh[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    old[c] = 0ull;
    hh[c] = 0u;
    if ((lmask >> c) & 1u) {
      hh[c] = hash_slot(~(u32)wv[c], shift);
      old[c] = atomicCAS(&tab[hh[c]], 0ull, wv[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    slot[c] = -1;
    if ((lmask >> c) & 1u) {
      if (old[c] == 0ull) {
        slot[c] = (int)hh[c];
      } else if ((u32)old[c] == (u32)wv[c]) {
        atomicAdd(&tab[hh[c]], wv[c] & 0xFFFFFFFF00000000ull);
      } else {
        slot[c] = lds_probe_word<kBounded>(tab, mask, wv[c], hh[c], err);
      }
    }
  }
}

// Weighted peel over NC chunks of tally words with per-lane state (bit c of
// `lmask`: word c still untallied): each round takes the first untallied label of
// the first lane holding one, sums its words' counts (VALU + DPP wave sums, no
// per-chunk scalar mask chains) and retires them; repeated while a round retires
// >= 2 words, up to `rounds`.  Round p's tally word ends in lane p's *pw; *best is
// the maximum; returns the number of rounds.
template <int NC>
__device__ __forceinline__ int peel_words(const u64 (&wv)[NC], u32& lmask, u64& best, u64& pw,
                                          int lane, int rounds) {
  int np = 0;
#pragma unroll 1
  for (int p = 0; p < rounds; ++p) {
    const u64 live = __ballot(lmask != 0u);
    if (live == 0ull) break;
    u32 cand = 0u;
#pragma unroll
    for (int c = NC - 1; c >= 0; --c)
      if ((lmask >> c) & 1u) cand = ~(u32)wv[c];
    const u32 x = (u32)__builtin_amdgcn_readlane((int)cand, __ffsll((unsigned long long)live) - 1);
    u32 m = 0u, cs = 0u;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (((lmask >> c) & 1u) && ~(u32)wv[c] == x) {
        m |= 1u << c;
        cs += (u32)(wv[c] >> 32);
      }
    }
    lmask &= ~m;
    const u32 k = wave_sum_u32((u32)__popc(m));
    const u64 tw = tally(wave_sum_u32(cs), x);
    best = umax64(best, tw);
    if (lane == p) pw = tw;
    np = p + 1;
    if (k < 2) break;
  }
  return np;
}

// Append the claimed slots of NC chunks to a block-shared LDS list with ONE
// returning LDS atomic per wave.
template <int NC>
__device__ __forceinline__ void list_append_n(uint16_t* lst, int* lcount, const int (&slot)[NC],
                                              int lane) {
  u64 cm[NC];
  int tot = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    cm[c] = __ballot(slot[c] >= 0);
    tot += __popcll(cm[c]);
  }
  if (tot == 0) return;  // uniform over the wave
  int base = 0;
  if (lane == 0) base = atomicAdd(lcount, tot);
  base = __builtin_amdgcn_readfirstlane(base);
  const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (slot[c] >= 0) lst[base + __popcll(cm[c] & lt)] = (uint16_t)slot[c];
    base += __popcll(cm[c]);
  }
}

// Wave-aggregated append of claimed slots to an LDS list (one LDS atomic per wave).
__device__ __forceinline__ void list_append(uint16_t* lst, int* lcount, int slot, int lane) {
  const u64 cm = __ballot(slot >= 0);
  if (cm == 0ull) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(lcount, __popcll(cm));
  base = __builtin_amdgcn_readfirstlane(base);
  if (slot >= 0) lst[base + __popcll(cm & ((1ull << lane) - 1ull))] = (uint16_t)slot;
}

// ---------------------------------------------------------------------------
// Block-aggregated histogram: hist[key] += val over a stream of (key, val) without
// the two costs of plain device atomics here -- same-address serialisation (hub
// degrees, giant communities: every wave adding into one counter) and one
// memory-side atomic per element.  The block sums into a small LDS open-addressing
// table (kBhSlots keys, at most kBhProbes probes per key) and flushes it at the end
// with one device atomic per distinct key; a key that finds no slot goes straight
// to the device histogram.  add1 first merges the lanes of a wave that hold the same
// key (ballot rounds), so a hub repeated across a wave is one LDS atomic.
// Every lane of the block must call init / add* / flush (they contain barriers or
// wave-wide ballots); keys must differ from kBhEmpty.
// ---------------------------------------------------------------------------
constexpr int kBhLg = 12;
constexpr int kBhSlots = 1 << kBhLg;
constexpr int kBhProbes = 8;
constexpr u32 kBhEmpty = 0xFFFFFFFFu;
// Once a key has failed every probe the table is taken as saturated (random keys:
// most later keys would fail too) and later keys probe their home slot only, where
// the block's early (hub) keys mostly sit.
template <typename T>
struct BlockHist {
  u32* key;  // LDS [kBhSlots]
  T* val;    // LDS [kBhSlots]
  int* sat;  // LDS: the table has overflowed
  __device__ __forceinline__ void init() {
    for (int i = threadIdx.x; i < kBhSlots; i += blockDim.x) {
      key[i] = kBhEmpty;
      val[i] = (T)0;
    }
    if (threadIdx.x == 0) *sat = 0;
    __syncthreads();
  }
  __device__ __forceinline__ bool lds_add(u32 k, T v) {
    u32 h = (k * 0x9E3779B1u) >> (32 - kBhLg);
    const int np = *sat ? 1 : kBhProbes;
#pragma unroll 1
    for (int p = 0; p < np; ++p) {
      const u32 old = atomicCAS(&key[h], kBhEmpty, k);
      if (old == kBhEmpty || old == k) {
        atomicAdd(&val[h], v);
        return true;
      }
      h = (h + 1u) & (u32)(kBhSlots - 1);
    }
    *sat = 1;
    return false;
  }
  // weighted: lanes with act add v to hist[k]
  __device__ __forceinline__ void addw(T* __restrict__ hist, bool act, u32 k, T v) {
    if (act && !lds_add(k, v)) atomicAdd(&hist[k], v);
  }
  // count: lanes with act add 1 to hist[k] (all 64 lanes of the wave call it)
  __device__ __forceinline__ void add1(T* __restrict__ hist, bool act, u32 k, int lane) {
    bool mine = act;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const u64 pend = __ballot(mine);
      if (pend == 0ull) return;  // uniform
      const int lead = __ffsll((unsigned long long)pend) - 1;
      const u32 kk = (u32)__builtin_amdgcn_readlane((int)k, lead);
      const bool eq = mine && k == kk;
      const u64 em = __ballot(eq);
      if (lane == lead) addw(hist, true, kk, (T)__popcll(em));
      if (eq) mine = false;
    }
    addw(hist, mine, k, (T)1);
  }
  __device__ __forceinline__ void flush(T* __restrict__ hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < kBhSlots; i += blockDim.x)
      if (key[i] != kBhEmpty) atomicAdd(&hist[key[i]], val[i]);
  }
};

}  // namespace dev
}  // namespace lpa
