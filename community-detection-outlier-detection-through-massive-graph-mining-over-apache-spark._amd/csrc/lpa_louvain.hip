// Louvain community detection on the handle's symmetrised multigraph (lpa_louvain): the
// synchronous, deterministic form include/lpa.h specifies, in exact int64 arithmetic.
//
// Stages (every array a stream-ordered temporary; nothing of the LPA state is read):
//   keys     level 0: every kept edge (u, v) gives the keys (u, v) and (v, u), weight 1;
//            a later level: every arc (row, col, w) of the level below gives
//            (id[c[row]], id[c[col]], w) and every vertex its self weight on the diagonal
//   build    one routine for every level (build_level): diagonal keys are peeled into s[]
//            with int64 adds, the rest is compacted, sorted with its weights
//            (radix_sort_u64_kv) and run-reduced to the level's CSR (off, row, col, w) and k[]
//   forms    rows by list length: short (kShortLanes lanes a row), wave (a wave a row, a
//            per-wave LDS table), block (a block a row, a block LDS table); a row of more
//            than half its form's table slots takes its own region of a global table
//            instead (the spill: sized from the row, 2 len rounded up to a power of two, so
//            it holds every distinct neighbour community at a load of at most 1/2)
//   round    the move kernels write prop[u] (the proposed community or -1) from the state
//            at the round's start; k_lv_apply builds the trial labels and recounts D and
//            size; k_lv_intra streams the arcs once for I; k_lv_sq sums D^2 and s.  The
//            host reads four words (proposals, proposals to a smaller id, I, sum D^2)
//            through pinned memory and accepts, retries the damped subset, or ends the
//            phase.  An accepted round swaps pointers; a rejected one costs nothing.
//   flatten  member[v] (the vertex of the current level that holds v) is carried through
//            the aggregations; comm[v] = the smallest v' with member[v'] == member[v]
//
// Integer sums are order-free, and the argmax is over a total order (score, then the
// smaller community id), so the result does not depend on the schedule, on the table a row
// took or on the order of the input edges.
#include <vector>

#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

namespace {

constexpr int kShortStage = 32;      // entries of a short row staged in LDS (longer: re-read from memory)
constexpr u64 kNoKey = ~0ull;        // a dropped edge / an absent diagonal
constexpr int32_t kNoCand = 0x7FFFFFFF;
constexpr int64_t kNoScore = INT64_MIN;   // no real score: |score| <= A^2 < 2^63
constexpr int64_t kMaxArcs = 3037000499ll;

// the call's counters (ull): proposals, proposals to a smaller id, I, sum of D^2, kept edges
enum { C_PROP = 0, C_DOWN = 1, C_INTRA = 2, C_SQ = 3, C_KEPT = 4, C_LEN = 8 };

// slots of a spilled row's table: 2 len rounded up to a power of two (< 4 len)
__host__ __device__ inline u64 spill_slots(int64_t len) {
  u64 x = 2ull * (u64)len, p = 2;
  while (p < x) p <<= 1;
  return p;
}

// sums of a 256-thread block into two counters
__device__ __forceinline__ void block_add2(ull a, ull b, ull* pa, ull* pb) {
  __shared__ ull ws[2][4];
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    ws[0][threadIdx.x >> 6] = a;
    ws[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
    b = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
    if (a) atomicAdd(pa, a);
    if (b) atomicAdd(pb, b);
  }
}

// ---------------------------------------------------------------------------
// keys and the level build
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_keys0(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                  int64_t m, u32 V, u64* __restrict__ keys, int64_t* __restrict__ wt,
                                                  ull* __restrict__ acc) {
  ull kept = 0;
  GRID_STRIDE(i, m) {
    const u32 a = (u32)__builtin_nontemporal_load(src + i), b = (u32)__builtin_nontemporal_load(dst + i);
    const bool ok = a < V && b < V;
    keys[2 * i] = ok ? ((u64)a << 32) | b : kNoKey;
    keys[2 * i + 1] = ok ? ((u64)b << 32) | a : kNoKey;
    wt[2 * i] = 1;
    wt[2 * i + 1] = 1;
    kept += ok ? 1ull : 0ull;
  }
  block_add2(kept, 0ull, acc + C_KEPT, acc + C_KEPT);
}

// the next level's keys: the arcs between the communities, then every vertex's self weight
__global__ __launch_bounds__(256) void k_lv_agg_keys(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                     const int64_t* __restrict__ w, int64_t nnz,
                                                     const int64_t* __restrict__ s, int64_t n,
                                                     const int32_t* __restrict__ c, const u32* __restrict__ id,
                                                     u64* __restrict__ keys, int64_t* __restrict__ wt) {
  GRID_STRIDE(j, nnz + n) {
    if (j < nnz) {
      keys[j] = ((u64)id[c[row[j]]] << 32) | id[c[col[j]]];
      wt[j] = w[j];
    } else {
      const int64_t u = j - nnz;
      const u32 x = id[c[u]];
      keys[j] = s[u] > 0 ? ((u64)x << 32) | x : kNoKey;
      wt[j] = s[u];
    }
  }
}

// diagonal keys go to s[]; flag = the key stays (an arc between two vertices)
__global__ __launch_bounds__(256) void k_lv_peel(const u64* __restrict__ keys, const int64_t* __restrict__ wt, int64_t M,
                                                 ull* __restrict__ s, uint8_t* __restrict__ flag) {
  GRID_STRIDE(i, M) {
    const u64 k = keys[i];
    const u32 hi = (u32)(k >> 32), lo = (u32)k;
    const bool diag = k != kNoKey && hi == lo;
    if (diag) atomicAdd(s + hi, (ull)wt[i]);
    flag[i] = k != kNoKey && !diag ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_lv_compact(const u64* __restrict__ keys, const int64_t* __restrict__ wt,
                                                    const uint8_t* __restrict__ flag, const u32* __restrict__ pos,
                                                    int64_t M, u64* __restrict__ okeys, u64* __restrict__ owt) {
  GRID_STRIDE(i, M) {
    if (flag[i]) {
      okeys[pos[i]] = keys[i];
      owt[pos[i]] = (u64)wt[i];
    }
  }
}

__global__ __launch_bounds__(256) void k_lv_heads(const u64* __restrict__ keys, int64_t M, uint8_t* __restrict__ flag) {
  GRID_STRIDE(i, M) flag[i] = i == 0 || keys[i - 1] != keys[i] ? 1 : 0;
}

// sorted keys -> the CSR entries: entry pos[i] + flag[i] - 1 is key i's run
__global__ __launch_bounds__(256) void k_lv_reduce(const u64* __restrict__ keys, const u64* __restrict__ wt,
                                                   const uint8_t* __restrict__ flag, const u32* __restrict__ pos,
                                                   int64_t M, int32_t* __restrict__ row, int32_t* __restrict__ col,
                                                   ull* __restrict__ w, ull* __restrict__ k) {
  GRID_STRIDE(i, M) {
    const u64 key = keys[i];
    const u32 hi = (u32)(key >> 32);
    const u32 e = pos[i] + flag[i] - 1u;
    if (flag[i]) {
      row[e] = (int32_t)hi;
      col[e] = (int32_t)(u32)key;
    }
    atomicAdd(w + e, (ull)wt[i]);
    atomicAdd(k + hi, (ull)wt[i]);
  }
}

// off[r] = the entry of the first sorted key of a row >= r (pos[M] = the entry count)
__global__ __launch_bounds__(256) void k_lv_bounds(const u64* __restrict__ keys, const u32* __restrict__ pos, int64_t M,
                                                   int64_t n, int64_t* __restrict__ off) {
  GRID_STRIDE(r, n + 1) {
    const u64 want = (u64)r << 32;
    int64_t lo = 0, hi = M;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    off[r] = (int64_t)pos[lo];
  }
}

// ---------------------------------------------------------------------------
// row forms
// ---------------------------------------------------------------------------
struct Forms {
  int32_t lv_short, lv_wave;   // list lengths up to which a row takes the short / the wave form
  u32 wave_slots, block_slots; // LDS table slots of the wave / the block form (powers of two, or 0)
};

__device__ __forceinline__ int form_of(const Forms& f, int64_t len) {
  return len <= f.lv_short ? 0 : len <= f.lv_wave ? 1 : 2;
}
__device__ __forceinline__ bool spills(const Forms& f, int form, int64_t len) {
  return form != 0 && 2 * len > (int64_t)(form == 1 ? f.wave_slots : f.block_slots);
}

__global__ __launch_bounds__(256) void k_lv_forms(const int64_t* __restrict__ off, int64_t n, Forms f,
                                                  uint8_t* __restrict__ fw, uint8_t* __restrict__ fb,
                                                  int64_t* __restrict__ need) {
  GRID_STRIDE(u, n) {
    const int64_t len = off[u + 1] - off[u];
    const int form = form_of(f, len);
    fw[u] = form == 1 ? 1 : 0;
    fb[u] = form == 2 ? 1 : 0;
    need[u] = spills(f, form, len) ? (int64_t)spill_slots(len) : 0;
  }
}

// ---------------------------------------------------------------------------
// the move kernels
// ---------------------------------------------------------------------------
struct Move {
  const int64_t* off;
  const int32_t* col;
  const int64_t* w;
  const int64_t* k;
  const int32_t* c;
  const int64_t* D;
  const int32_t* size;
  int32_t* prop;
  ull* acc;
  int64_t A, n;
  Forms f;
  const int64_t* spoff;   // [n + 1] first slot of a spilled row's region
  int32_t* sp_keys;
  ull* sp_vals;
};

__device__ __forceinline__ bool better(int64_t sc, int32_t x, int64_t bsc, int32_t bx) {
  return sc > bsc || (sc == bsc && x < bx);
}

// the proposal of row u from its own weight and its best other community
__device__ __forceinline__ int32_t decide(const Move& m, int64_t u, int32_t a, int64_t kown, int64_t bsc, int32_t bx) {
  if (bx == kNoCand) return -1;
  const int64_t ku = m.k[u];
  const int64_t sc_a = m.A * kown - ku * (m.D[a] - ku);
  if (!(bsc > sc_a)) return -1;
  if (m.size[a] == 1 && m.size[bx] == 1 && bx > a) return -1;
  return bx;
}

// every row in id order, kShortLanes lanes each; a longer row is not this form's.  A lane
// takes the entries sub, sub + G, ... and sums for each the weight of every entry of the row
// in the same community (len^2 / G steps, no table): from the group's LDS stage for rows of
// up to kShortStage entries, from memory for longer ones (an overridden boundary).
__global__ __launch_bounds__(256) void k_lv_move_short(Move m) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  __shared__ int32_t xs[kRows][kShortStage];
  __shared__ int64_t wsh[kRows][kShortStage];
  const int sub = threadIdx.x & (G - 1), grp = threadIdx.x / G, lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < m.n; base += (int64_t)gridDim.x * kRows) {
    const int64_t u = base + grp;
    int64_t b = 0, len = -1;
    int32_t a = 0;
    if (u < m.n) {
      b = m.off[u];
      len = m.off[u + 1] - b;
      if (len > m.f.lv_short) len = -1;
      a = m.c[u];
    }
    const bool staged = len > 0 && len <= kShortStage;
    if (staged)
      for (int64_t j = sub; j < len; j += G) {
        xs[grp][j] = m.c[m.col[b + j]];
        wsh[grp][j] = m.w[b + j];
      }
    __syncthreads();
    int64_t kown = 0, bsc = kNoScore;
    int32_t bx = kNoCand;
    if (len > 0) {
      const int64_t ku = m.k[u];
      for (int64_t j = sub; j < len; j += G) {
        const int32_t x = staged ? xs[grp][j] : m.c[m.col[b + j]];
        int64_t K = 0;
        if (staged) {
          for (int i = 0; i < (int)len; ++i) K += xs[grp][i] == x ? wsh[grp][i] : 0;
        } else {
          for (int64_t i = 0; i < len; ++i) K += m.c[m.col[b + i]] == x ? m.w[b + i] : 0;
        }
        if (x == a) {
          kown = K;
        } else {
          const int64_t sc = m.A * K - ku * m.D[x];
          if (better(sc, x, bsc, bx)) {
            bsc = sc;
            bx = x;
          }
        }
      }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
      const int64_t osc = __shfl_xor(bsc, o, 64), ok = __shfl_xor(kown, o, 64);
      const int32_t ox = __shfl_xor(bx, o, 64);
      if (better(osc, ox, bsc, bx)) {
        bsc = osc;
        bx = ox;
      }
      kown = ok > kown ? ok : kown;
    }
    int32_t p = -1;
    if (sub == 0 && len >= 0) {
      p = len > 0 ? decide(m, u, a, kown, bsc, bx) : -1;
      m.prop[u] = p;
    }
    const u64 want = __ballot(p >= 0), down = __ballot(p >= 0 && p < a);
    if (lane == 0) {
      if (want) atomicAdd(m.acc + C_PROP, (ull)__popcll(want));
      if (down) atomicAdd(m.acc + C_DOWN, (ull)__popcll(down));
    }
    __syncthreads();
  }
}

// A row's tally table: open addressing over (community, summed weight), never more than
// half full.  kGlobal: the row's region of the spill table, every access an agent-scope
// atomic (other lanes insert at the memory side); otherwise LDS.
template <bool kGlobal>
struct Tab {
  int32_t* keys;
  ull* vals;
  u64 mask;
  __device__ __forceinline__ void clear(u64 i) const {
    if constexpr (kGlobal) {
      __hip_atomic_store(keys + i, -1, LPA_RLX_AGENT);
      __hip_atomic_store(vals + i, 0ull, LPA_RLX_AGENT);
    } else {
      keys[i] = -1;
      vals[i] = 0ull;
    }
  }
  __device__ __forceinline__ void add(int32_t x, ull wt) const {
    u64 h = (((u64)(u32)x * 0x9E3779B97F4A7C15ull) >> 32) & mask;
    while (true) {
      int32_t old;
      if constexpr (kGlobal) {
        old = -1;
        if (__hip_atomic_compare_exchange_strong(keys + h, &old, x, __ATOMIC_RELAXED, LPA_RLX_AGENT)) old = -1;
      } else {
        old = atomicCAS(keys + h, -1, x);
      }
      if (old == -1 || old == x) {
        if constexpr (kGlobal) __hip_atomic_fetch_add(vals + h, wt, LPA_RLX_AGENT);
        else atomicAdd(vals + h, wt);
        return;
      }
      h = (h + 1) & mask;
    }
  }
  __device__ __forceinline__ int32_t key(u64 i) const {
    if constexpr (kGlobal) return __hip_atomic_load(keys + i, LPA_RLX_AGENT);
    else return keys[i];
  }
  __device__ __forceinline__ ull val(u64 i) const {
    if constexpr (kGlobal) return __hip_atomic_load(vals + i, LPA_RLX_AGENT);
    else return vals[i];
  }
};

// between the phases of a row's tally (clear, insert, read)
template <bool kBlock, bool kGlobal>
__device__ __forceinline__ void phase_sync() {
  if constexpr (kBlock) {
    __syncthreads();
  } else {
    if constexpr (kGlobal) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

// thread t of T: this thread's share of row u's candidates (own weight, best other community)
template <bool kBlock, bool kGlobal>
__device__ __forceinline__ void tally_row(const Move& m, int64_t u, int32_t a, int64_t b, int64_t len, Tab<kGlobal> tab,
                                          int t, int T, int64_t* kown, int64_t* bsc, int32_t* bx) {
  const u64 slots = tab.mask + 1;
  for (u64 i = t; i < slots; i += T) tab.clear(i);
  phase_sync<kBlock, kGlobal>();
  for (int64_t j = t; j < len; j += T) tab.add(m.c[m.col[b + j]], (ull)m.w[b + j]);
  phase_sync<kBlock, kGlobal>();
  const int64_t ku = m.k[u];
  for (u64 i = t; i < slots; i += T) {
    const int32_t x = tab.key(i);
    if (x < 0) continue;
    const int64_t K = (int64_t)tab.val(i);
    if (x == a) {
      *kown = K;
    } else {
      const int64_t sc = m.A * K - ku * m.D[x];
      if (better(sc, x, *bsc, *bx)) {
        *bsc = sc;
        *bx = x;
      }
    }
  }
}

__device__ __forceinline__ void wave_best(int64_t* kown, int64_t* bsc, int32_t* bx) {
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t osc = __shfl_xor(*bsc, o, 64), ok = __shfl_xor(*kown, o, 64);
    const int32_t ox = __shfl_xor(*bx, o, 64);
    if (better(osc, ox, *bsc, *bx)) {
      *bsc = osc;
      *bx = ox;
    }
    *kown = ok > *kown ? ok : *kown;
  }
}

__device__ __forceinline__ void publish(const Move& m, int64_t u, int32_t a, int64_t kown, int64_t bsc, int32_t bx) {
  const int32_t p = decide(m, u, a, kown, bsc, bx);
  m.prop[u] = p;
  if (p >= 0) {
    atomicAdd(m.acc + C_PROP, 1ull);
    if (p < a) atomicAdd(m.acc + C_DOWN, 1ull);
  }
}

// a wave per listed row; kSlots = the most LDS slots a wave's table has
template <int kSlots>
__global__ __launch_bounds__(256) void k_lv_move_wave(const int32_t* __restrict__ rows, int64_t nrows, Move m) {
  __shared__ int32_t tk[4][kSlots];
  __shared__ ull tv[4][kSlots];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < nrows; r += (int64_t)gridDim.x * 4) {
    const int64_t u = rows[r], b = m.off[u], len = m.off[u + 1] - b;
    const int32_t a = m.c[u];
    int64_t kown = 0, bsc = kNoScore;
    int32_t bx = kNoCand;
    if (spills(m.f, 1, len)) {
      const Tab<true> tab{m.sp_keys + m.spoff[u], m.sp_vals + m.spoff[u], spill_slots(len) - 1};
      tally_row<false, true>(m, u, a, b, len, tab, lane, 64, &kown, &bsc, &bx);
    } else {
      const Tab<false> tab{tk[wv], tv[wv], (u64)m.f.wave_slots - 1};
      tally_row<false, false>(m, u, a, b, len, tab, lane, 64, &kown, &bsc, &bx);
    }
    wave_best(&kown, &bsc, &bx);
    if (lane == 0) publish(m, u, a, kown, bsc, bx);
    phase_sync<false, false>();   // the table is the next row's
  }
}

// a block per listed row
template <int kSlots>
__global__ __launch_bounds__(kBlockThreads) void k_lv_move_block(const int32_t* __restrict__ rows, int64_t nrows, Move m) {
  __shared__ int32_t tk[kSlots];
  __shared__ ull tv[kSlots];
  __shared__ int64_t rk[kBlockThreads / 64], rs[kBlockThreads / 64];
  __shared__ int32_t rx[kBlockThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const int64_t u = rows[r], b = m.off[u], len = m.off[u + 1] - b;
    const int32_t a = m.c[u];
    int64_t kown = 0, bsc = kNoScore;
    int32_t bx = kNoCand;
    if (spills(m.f, 2, len)) {
      const Tab<true> tab{m.sp_keys + m.spoff[u], m.sp_vals + m.spoff[u], spill_slots(len) - 1};
      tally_row<true, true>(m, u, a, b, len, tab, (int)threadIdx.x, kBlockThreads, &kown, &bsc, &bx);
    } else {
      const Tab<false> tab{tk, tv, (u64)m.f.block_slots - 1};
      tally_row<true, false>(m, u, a, b, len, tab, (int)threadIdx.x, kBlockThreads, &kown, &bsc, &bx);
    }
    wave_best(&kown, &bsc, &bx);
    if (lane == 0) {
      rk[wv] = kown;
      rs[wv] = bsc;
      rx[wv] = bx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 1; i < kBlockThreads / 64; ++i) {
        if (better(rs[i], rx[i], bsc, bx)) {
          bsc = rs[i];
          bx = rx[i];
        }
        kown = rk[i] > kown ? rk[i] : kown;
      }
      publish(m, u, a, kown, bsc, bx);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// apply and test
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_iota(int32_t* __restrict__ c, int64_t n) {
  GRID_STRIDE(u, n) c[u] = (int32_t)u;
}

__global__ __launch_bounds__(256) void k_lv_fill(int32_t* __restrict__ p, int64_t n, int32_t v) {
  GRID_STRIDE(u, n) p[u] = v;
}

// the trial labels (every proposal, or only those to a smaller id) and their D and size
__global__ __launch_bounds__(256) void k_lv_apply(const int32_t* __restrict__ c, const int32_t* __restrict__ prop,
                                                  const int64_t* __restrict__ k, int64_t n, int only_down,
                                                  int32_t* __restrict__ cx, ull* __restrict__ D,
                                                  int32_t* __restrict__ size) {
  GRID_STRIDE(u, n) {
    const int32_t a = c[u], p = prop[u];
    const int32_t x = p >= 0 && (!only_down || p < a) ? p : a;
    cx[u] = x;
    atomicAdd(D + x, (ull)k[u]);
    atomicAdd(size + x, 1);
  }
}

// I, the arcs' part: one streaming pass
__global__ __launch_bounds__(256) void k_lv_intra(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                  const int64_t* __restrict__ w, int64_t nnz,
                                                  const int32_t* __restrict__ cx, ull* __restrict__ acc) {
  ull in = 0;
  GRID_STRIDE(j, nnz) {
    const int32_t r = __builtin_nontemporal_load(row + j), q = __builtin_nontemporal_load(col + j);
    const int64_t x = __builtin_nontemporal_load(w + j);
    in += cx[r] == cx[q] ? (ull)x : 0ull;
  }
  block_add2(in, 0ull, acc + C_INTRA, acc + C_SQ);
}

// I, the self weights' part, and the sum of D^2
__global__ __launch_bounds__(256) void k_lv_sq(const ull* __restrict__ D, const int64_t* __restrict__ s, int64_t n,
                                               ull* __restrict__ acc) {
  ull in = 0, sq = 0;
  GRID_STRIDE(u, n) {
    in += (ull)s[u];
    sq += D[u] * D[u];
  }
  block_add2(in, sq, acc + C_INTRA, acc + C_SQ);
}

// ---------------------------------------------------------------------------
// aggregation, flatten, summary
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_alive(const int32_t* __restrict__ size, int64_t n, uint8_t* __restrict__ flag) {
  GRID_STRIDE(u, n) flag[u] = size[u] > 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_lv_member(int32_t* __restrict__ member, int64_t V, const int32_t* __restrict__ c,
                                                   const u32* __restrict__ id) {
  GRID_STRIDE(v, V) member[v] = (int32_t)id[c[member[v]]];
}

__global__ __launch_bounds__(256) void k_lv_low(const int32_t* __restrict__ member, int64_t V, int32_t* __restrict__ low) {
  GRID_STRIDE(v, V) atomicMin(low + member[v], (int32_t)v);
}

__global__ __launch_bounds__(256) void k_lv_comm(const int32_t* __restrict__ member, const int32_t* __restrict__ low,
                                                 int64_t V, int32_t* __restrict__ comm, ull* __restrict__ size) {
  GRID_STRIDE(v, V) {
    const int32_t x = low[member[v]];
    comm[v] = x;
    if (size) atomicAdd(size + x, 1ull);
  }
}

// acc[0] communities, [1] singletons, [2] max of (size << 32 | 0xFFFFFFFF - id): the largest
// community, the smallest id among equals
__global__ __launch_bounds__(256) void k_lv_summary(const int32_t* __restrict__ comm, const ull* __restrict__ size,
                                                    int64_t V, ull* __restrict__ acc) {
  __shared__ ull ws[4];
  ull n = 0, n1 = 0, best = 0;
  GRID_STRIDE(v, V) {
    if (comm[v] == (int32_t)v) {
      const ull sz = size[v];
      n += 1;
      n1 += sz == 1ull ? 1ull : 0ull;
      best = dev::umax64(best, (sz << 32) | (ull)(0xFFFFFFFFu - (u32)v));
    }
  }
  for (int off = 32; off > 0; off >>= 1) best = dev::umax64(best, __shfl_xor(best, off, 64));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    best = dev::umax64(dev::umax64(ws[0], ws[1]), dev::umax64(ws[2], ws[3]));
    if (best) atomicMax(acc + 2, best);
  }
  __syncthreads();
  block_add2(n, n1, acc, acc + 1);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct Level {   // one level's weighted CSR, its row lists and its spill table
  int64_t n = 0, nnz = 0;
  int64_t *off = nullptr, *w = nullptr, *s = nullptr, *k = nullptr;
  int32_t *row = nullptr, *col = nullptr;
  int32_t* lists = nullptr;     // [2 n] the wave-form rows, ascending; at + n the block-form rows
  int64_t* spoff = nullptr;     // [n + 1]
  int32_t* sp_keys = nullptr;
  ull* sp_vals = nullptr;
  u32 n_wave = 0, n_block = 0;
  void release(Tmp& t) {
    void* all[] = {off, w, s, k, row, col, lists, spoff, sp_keys, sp_vals};
    for (void* p : all)
      if (p) t.drop(p);
    *this = Level{};
  }
};

// (keys, wt)[M] over n vertices -> the level (keys and wt are read only)
int build_level(Tmp& tmp, const u64* keys, const int64_t* wt, int64_t M, int64_t n, const Forms& f, Level* L) {
  hipStream_t s = tmp.s;
  L->n = n;
  uint8_t* flag = nullptr;
  u32* pos = nullptr;
  LPA_TRY(tmp.get(&L->s, n));
  LPA_TRY(tmp.get(&flag, M));
  LPA_TRY(tmp.get(&pos, M + 1));
  LPA_HIP(hipMemsetAsync(L->s, 0, sizeof(int64_t) * (size_t)n, s));
  hipLaunchKernelGGL(k_lv_peel, dim3(grid_for(M)), dim3(256), 0, s, keys, wt, M, (ull*)L->s, flag);
  LPA_HIP(hipGetLastError());
  LPA_TRY(exclusive_scan_u8_u32(flag, pos, M, s));
  u32 h = 0;
  LPA_HIP(hipMemcpyAsync(&h, pos + M, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  const int64_t M1 = (int64_t)h;
  u64 *kk = nullptr, *ww = nullptr;   // [2 M1] each: the arcs and the sort's other buffer
  LPA_TRY(tmp.get(&kk, 2 * M1));
  LPA_TRY(tmp.get(&ww, 2 * M1));
  hipLaunchKernelGGL(k_lv_compact, dim3(grid_for(M)), dim3(256), 0, s, keys, wt, flag, pos, M, kk, ww);
  LPA_HIP(hipGetLastError());
  const HalfShifts sh(bits_for((uint64_t)n));
  LPA_TRY(radix_sort_u64_kv(kk, ww, kk + M1, ww + M1, M1, sh.both(), 2 * sh.ns, s));
  hipLaunchKernelGGL(k_lv_heads, dim3(grid_for(M1)), dim3(256), 0, s, kk, M1, flag);
  LPA_HIP(hipGetLastError());
  LPA_TRY(exclusive_scan_u8_u32(flag, pos, M1, s));
  LPA_HIP(hipMemcpyAsync(&h, pos + M1, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  const int64_t E = (int64_t)h;
  L->nnz = E;
  LPA_TRY(tmp.get(&L->off, n + 1));
  LPA_TRY(tmp.get(&L->k, n));
  LPA_TRY(tmp.get(&L->row, E));
  LPA_TRY(tmp.get(&L->col, E));
  LPA_TRY(tmp.get(&L->w, E));
  LPA_HIP(hipMemsetAsync(L->w, 0, sizeof(int64_t) * (size_t)(E > 0 ? E : 1), s));
  LPA_HIP(hipMemcpyAsync(L->k, L->s, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_lv_reduce, dim3(grid_for(M1)), dim3(256), 0, s, kk, ww, flag, pos, M1, L->row, L->col,
                     (ull*)L->w, (ull*)L->k);
  hipLaunchKernelGGL(k_lv_bounds, dim3(grid_for(n + 1)), dim3(256), 0, s, kk, pos, M1, n, L->off);
  LPA_HIP(hipGetLastError());
  tmp.drop(kk);
  tmp.drop(ww);
  tmp.drop(flag);
  tmp.drop(pos);
  // ---- the row lists and the spill regions ----
  uint8_t *fw = nullptr, *fb = nullptr;
  u32 *pw = nullptr, *pb = nullptr;
  int64_t* need = nullptr;
  LPA_TRY(tmp.get(&fw, n));
  LPA_TRY(tmp.get(&fb, n));
  LPA_TRY(tmp.get(&pw, n + 1));
  LPA_TRY(tmp.get(&pb, n + 1));
  LPA_TRY(tmp.get(&need, n));
  LPA_TRY(tmp.get(&L->lists, 2 * n));
  LPA_TRY(tmp.get(&L->spoff, n + 1));
  hipLaunchKernelGGL(k_lv_forms, dim3(grid_for(n)), dim3(256), 0, s, L->off, n, f, fw, fb, need);
  LPA_HIP(hipGetLastError());
  LPA_TRY(exclusive_scan_u8_u32(fw, pw, n, s));
  LPA_TRY(exclusive_scan_u8_u32(fb, pb, n, s));
  LPA_TRY(exclusive_scan_i64(need, L->spoff, n, s));
  LPA_TRY(fill_form_lists(fw, fb, pw, pb, n, L->lists, s));
  int64_t total = 0;
  LPA_HIP(hipMemcpyAsync(&L->n_wave, pw + n, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(&L->n_block, pb + n, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(&total, L->spoff + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  LPA_TRY(tmp.get(&L->sp_keys, total));
  LPA_TRY(tmp.get(&L->sp_vals, total));
  tmp.drop(fw);
  tmp.drop(fb);
  tmp.drop(pw);
  tmp.drop(pb);
  tmp.drop(need);
  return LPA_OK;
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream and lv_short / lv_wave / lv_table of the handle,
// nothing of the LPA state; every array is a stream-ordered temporary.
int louvain(lpa_graph* g, int32_t max_levels, int32_t max_rounds, int32_t* comm_out, int32_t out_is_device,
            int64_t* size_out, lpa_louvain_level* levels_out, int32_t levels_cap, lpa_louvain_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  lpa_louvain_summary sum = {};
  sum.largest_id = -1;
  if (summary) *summary = sum;
  if (V == 0) return LPA_OK;
  if (2 * m >= (int64_t)UINT32_MAX) {   // past the arc limit whatever is kept, and past the sort's range
    set_error("lpa_louvain: %lld edges exceed the limit of %lld arcs (arcs^2 must fit int64)", (long long)m,
              (long long)kMaxArcs);
    return LPA_EINVAL;
  }
  Tmp tmp(s);
  Forms f;
  f.lv_short = g->lv_short;
  f.lv_wave = g->lv_wave;
  f.wave_slots = (u32)(g->lv_table < kLvWaveSlots ? g->lv_table : kLvWaveSlots);
  f.block_slots = (u32)g->lv_table;
  ull* acc = nullptr;
  int32_t *member = nullptr, *comm = comm_out;
  LPA_TRY(tmp.get(&acc, C_LEN));
  LPA_TRY(tmp.get(&member, V));
  if (!out_is_device) LPA_TRY(tmp.get(&comm, V));
  ull* pinned = nullptr;
  LPA_TRY(tmp.pin(&pinned, C_LEN));
  const volatile ull* hc = pinned;
  const auto read_acc = [&]() -> int {
    LPA_HIP(hipMemcpyAsync(pinned, acc, sizeof(ull) * C_LEN, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipStreamSynchronize(s));
    return LPA_OK;
  };
  hipLaunchKernelGGL(k_lv_iota, dim3(grid_for(V)), dim3(256), 0, s, member, V);
  LPA_HIP(hipMemsetAsync(acc, 0, sizeof(ull) * C_LEN, s));
  // ---- level 0 ----
  Level L;
  int64_t A = 0;
  if (m > 0) {
    u64* keys = nullptr;
    int64_t* wt = nullptr;
    LPA_TRY(tmp.get(&keys, 2 * m));
    LPA_TRY(tmp.get(&wt, 2 * m));
    hipLaunchKernelGGL(k_lv_keys0, dim3(grid_for(m)), dim3(256), 0, s, g->e_src, g->e_dst, m, (u32)V, keys, wt, acc);
    LPA_HIP(hipGetLastError());
    LPA_TRY(read_acc());
    A = 2 * (int64_t)hc[C_KEPT];
    if (A > kMaxArcs) {
      set_error("lpa_louvain: %lld arcs exceed the limit of %lld (arcs^2 must fit int64)", (long long)A,
                (long long)kMaxArcs);
      return LPA_EINVAL;
    }
    if (A > 0) LPA_TRY(build_level(tmp, keys, wt, 2 * m, V, f, &L));
    tmp.drop(keys);
    tmp.drop(wt);
  }
  int64_t levels = 0, N = 0, intra = 0, rounds_all = 0, damped_all = 0, moves_all = 0;
  while (A > 0) {
    const int64_t n = L.n;
    // ---- the level's state: c = identity, and its D, size, N by the round's own kernels ----
    int32_t *c = nullptr, *cx = nullptr, *prop = nullptr;
    char* ds[2] = {nullptr, nullptr};   // (D [n] ull, size [n] int32): the current and the trial
    const size_t ds_bytes = (sizeof(ull) + sizeof(int32_t)) * (size_t)n;
    LPA_TRY(tmp.get(&c, n));
    LPA_TRY(tmp.get(&cx, n));
    LPA_TRY(tmp.get(&prop, n));
    LPA_TRY(tmp.get(&ds[0], (int64_t)ds_bytes));
    LPA_TRY(tmp.get(&ds[1], (int64_t)ds_bytes));
    const auto D_of = [&](char* p) { return reinterpret_cast<ull*>(p); };
    const auto size_of = [&](char* p) { return reinterpret_cast<int32_t*>(p + sizeof(ull) * (size_t)n); };
    // trial labels from (c, prop) into cx with their D / size in ds[1], then I and sum D^2 into acc
    const auto trial = [&](int only_down) -> int {
      LPA_HIP(hipMemsetAsync(ds[1], 0, ds_bytes, s));
      LPA_HIP(hipMemsetAsync(acc + C_INTRA, 0, sizeof(ull) * 2, s));
      hipLaunchKernelGGL(k_lv_apply, dim3(grid_for(n)), dim3(256), 0, s, c, prop, L.k, n, only_down, cx, D_of(ds[1]),
                         size_of(ds[1]));
      if (L.nnz > 0)
        hipLaunchKernelGGL(k_lv_intra, dim3(grid_for(L.nnz)), dim3(256), 0, s, L.row, L.col, L.w, L.nnz, cx, acc);
      hipLaunchKernelGGL(k_lv_sq, dim3(grid_for(n)), dim3(256), 0, s, D_of(ds[1]), L.s, n, acc);
      LPA_HIP(hipGetLastError());
      return read_acc();
    };
    const auto accept = [&]() {
      int32_t* t = c;
      c = cx;
      cx = t;
      char* d = ds[0];
      ds[0] = ds[1];
      ds[1] = d;
      intra = (int64_t)hc[C_INTRA];
      N = A * intra - (int64_t)hc[C_SQ];
    };
    hipLaunchKernelGGL(k_lv_iota, dim3(grid_for(n)), dim3(256), 0, s, c, n);
    LPA_HIP(hipMemsetAsync(prop, 0xFF, sizeof(int32_t) * (size_t)n, s));
    LPA_TRY(trial(0));
    accept();
    int64_t rounds = 0, damped = 0, moves = 0;
    while (rounds < (int64_t)max_rounds) {
      LPA_HIP(hipMemsetAsync(acc, 0, sizeof(ull) * 2, s));
      const Move mv{L.off, L.col, L.w, L.k, c, reinterpret_cast<const int64_t*>(D_of(ds[0])), size_of(ds[0]), prop, acc,
                    A, n, f, L.spoff, L.sp_keys, L.sp_vals};
      hipLaunchKernelGGL(k_lv_move_short, dim3(grid_rows(n, 256 / kShortLanes, 65536)), dim3(256), 0, s, mv);
      if (L.n_wave)
        hipLaunchKernelGGL(k_lv_move_wave<kLvWaveSlots>, dim3(grid_rows(L.n_wave, 4, 16384)), dim3(256), 0, s, L.lists,
                           (int64_t)L.n_wave, mv);
      if (L.n_block)
        hipLaunchKernelGGL(k_lv_move_block<kLvBlockSlots>, dim3(grid_rows(L.n_block, 1, 4096)), dim3(kBlockThreads), 0,
                           s, L.lists + n, (int64_t)L.n_block, mv);
      LPA_HIP(hipGetLastError());
      LPA_TRY(trial(0));
      const int64_t n_prop = (int64_t)hc[C_PROP], n_down = (int64_t)hc[C_DOWN];
      if (n_prop == 0) break;
      ++rounds;
      if (A * (int64_t)hc[C_INTRA] - (int64_t)hc[C_SQ] > N) {
        accept();
        moves += n_prop;
        continue;
      }
      if (n_down == 0) break;
      LPA_TRY(trial(1));
      if (!(A * (int64_t)hc[C_INTRA] - (int64_t)hc[C_SQ] > N)) break;
      accept();
      moves += n_down;
      ++damped;
    }
    int64_t n_next = n;
    if (moves > 0) {
      // ---- aggregate: the surviving ids, ascending, are the next level's vertices ----
      uint8_t* alive = nullptr;
      u32* id = nullptr;
      LPA_TRY(tmp.get(&alive, n));
      LPA_TRY(tmp.get(&id, n + 1));
      hipLaunchKernelGGL(k_lv_alive, dim3(grid_for(n)), dim3(256), 0, s, size_of(ds[0]), n, alive);
      LPA_HIP(hipGetLastError());
      LPA_TRY(exclusive_scan_u8_u32(alive, id, n, s));
      u32 h = 0;
      LPA_HIP(hipMemcpyAsync(&h, id + n, sizeof(u32), hipMemcpyDeviceToHost, s));
      hipLaunchKernelGGL(k_lv_member, dim3(grid_for(V)), dim3(256), 0, s, member, V, c, id);
      LPA_HIP(hipGetLastError());
      LPA_HIP(hipStreamSynchronize(s));
      n_next = (int64_t)h;
      if (levels < (int64_t)levels_cap && levels_out)
        levels_out[levels] = lpa_louvain_level{n, n_next, rounds, damped, moves, N};
      ++levels;
      rounds_all += rounds;
      damped_all += damped;
      moves_all += moves;
      if (levels < (int64_t)max_levels) {
        const int64_t M = L.nnz + n;
        u64* keys = nullptr;
        int64_t* wt = nullptr;
        LPA_TRY(tmp.get(&keys, M));
        LPA_TRY(tmp.get(&wt, M));
        hipLaunchKernelGGL(k_lv_agg_keys, dim3(grid_for(M)), dim3(256), 0, s, L.row, L.col, L.w, L.nnz, L.s, n, c, id,
                           keys, wt);
        LPA_HIP(hipGetLastError());
        L.release(tmp);
        LPA_TRY(build_level(tmp, keys, wt, M, n_next, f, &L));
        tmp.drop(keys);
        tmp.drop(wt);
      }
      tmp.drop(alive);
      tmp.drop(id);
    }
    tmp.drop(c);
    tmp.drop(cx);
    tmp.drop(prop);
    tmp.drop(ds[0]);
    tmp.drop(ds[1]);
    if (moves == 0 || levels == (int64_t)max_levels) break;
  }
  // ---- flatten: member[v] indexes the last level's vertices (at most V of them) ----
  int32_t* low = nullptr;
  ull *size = nullptr, *sacc = nullptr;
  ull h[3] = {0, 0, 0};
  LPA_TRY(tmp.get(&low, V));
  hipLaunchKernelGGL(k_lv_fill, dim3(grid_for(V)), dim3(256), 0, s, low, V, (int32_t)0x7FFFFFFF);
  hipLaunchKernelGGL(k_lv_low, dim3(grid_for(V)), dim3(256), 0, s, member, V, low);
  if (size_out || summary) {
    size = reinterpret_cast<ull*>(size_out);
    if (!size_out || !out_is_device) LPA_TRY(tmp.get(&size, V));
    LPA_HIP(hipMemsetAsync(size, 0, sizeof(ull) * (size_t)V, s));
  }
  hipLaunchKernelGGL(k_lv_comm, dim3(grid_for(V)), dim3(256), 0, s, member, low, V, comm, size);
  LPA_HIP(hipGetLastError());
  if (summary) {
    LPA_TRY(tmp.get(&sacc, 3));
    LPA_HIP(hipMemsetAsync(sacc, 0, sizeof(h), s));
    hipLaunchKernelGGL(k_lv_summary, dim3(grid_for(V) < 2048u ? grid_for(V) : 2048u), dim3(256), 0, s, comm, size, V,
                       sacc);
    LPA_HIP(hipGetLastError());
    LPA_HIP(hipMemcpyAsync(h, sacc, sizeof(h), hipMemcpyDeviceToHost, s));
  }
  if (!out_is_device) {
    LPA_HIP(hipMemcpyAsync(comm_out, comm, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    if (size_out) LPA_HIP(hipMemcpyAsync(size_out, size, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  }
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    sum.n_communities = (int64_t)h[0];
    sum.n_singletons = (int64_t)h[1];
    sum.largest_size = (int64_t)(h[2] >> 32);
    sum.largest_id = (int64_t)(0xFFFFFFFFu - (u32)h[2]);
    sum.levels = levels;
    sum.rounds = rounds_all;
    sum.damped_rounds = damped_all;
    sum.moves = moves_all;
    sum.arcs = A;
    sum.intra_arcs = intra;
    sum.numerator = N;
    sum.modularity = A > 0 ? (double)N / ((double)A * (double)A) : 0.0;
    *summary = sum;
  }
  return LPA_OK;
}

}  // namespace lpa
