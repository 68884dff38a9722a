// k-core decomposition of the handle's input multigraph (GraphFrame.coreNumber / kCore):
// core[v] = the largest k such that v lies in a subgraph of the canonical simple undirected
// graph (no self-loops, no direction, duplicates collapsed: lpa_adj.hip's) in which every vertex
// has at least k neighbours; with a cap, min(core[v], max_k).  Integers throughout.
//
//   build    keys (min << 32 | max) of every edge, radix-sorted; the first key of each run with
//            min != max is a simple edge (E of them: lpa_adj.hip, simple_edges).  Both directions of every
//            simple edge as arc keys (from << 32 | to), sorted by the high half: the CSR
//            off[] (the first arc of every vertex, by binary search) / col[] (2 E entries).
//            deg[v] = off[v + 1] - off[v], the live count; the simple degree stays readable
//            from off[]
//   level    k = the smallest live count among the alive vertices (one block-reduced pass over
//            the alive list, which also counts it: empty levels are jumped over).  k >= max_k:
//            every alive vertex gets max_k, done.  The list is compacted whenever at most half
//            of it is alive, so the passes of all levels sum to O(V) + the levels themselves
//   seed     every alive v with deg[v] <= k: core[v] = k, dead, appended to the removal queue
//   expand   sub-level by sub-level over the queue: a queued u takes 1 from deg[w] of its
//            neighbours (relaxed agent-scope fetch-add); the one thread whose add takes deg[w]
//            from k + 1 to k removes w: core[w] = k, dead, appended.  Until the queue drains
//
// Why the interleaving does not matter.  deg[w] only falls, by one per dead neighbour, and the
// adds are atomic: whatever their order, exactly one of them returns k + 1 (a batched add of n,
// below: exactly one spans it, old > k >= old - n), and it does so exactly when w has fewer than
// k + 1 neighbours left among the vertices not yet removed, which is when the peeling removes
// it.  No second claim is possible, so no state-byte CAS is needed.  The peeling's fixpoint is
// unique (the k-core is the union of all subgraphs of minimum degree >= k), hence core[], the
// levels and every summary field but `passes` are functions of (V, edge set, max_k) alone.
//
// Visibility.  dead[] is read with plain loads and may be stale inside a kernel (another CU's L1
// is never refreshed): a byte only goes 0 -> 1, so a stale 0 costs one needless atomic on a
// vertex that is already gone (its count is never looked at again) and a read of 1 is always
// true.  The byte never decides a claim: the fetch-add alone does.  deg[] is only touched by
// agent-scope atomics while it is shared; the min / seed passes read it in a later kernel.
// core[w] is written once, by w's claimer.  Lists written by one kernel are read by the next.
//
// Row forms, by list length L (lpa_graph::kc_short / kc_wave):
//   short   L <= kc_short   8 lanes per queued row
//   wave    L <= kc_wave    a wave per queued row
//   block   above           a block of 1024 per queued row
// A wave-form or block-form row's lanes hold distinct neighbours.  The short form's lanes hold
// eight rows' neighbours, which under a star are all the hub: the lanes of a wave that hold the
// first active lane's w share one fetch-add of their number (kKcAgg such rounds, then one add
// per lane), as k_tc_degrees folds a run.
// A sub-level of at most kc_block vertices (a longer row counting as kKcLongRow) runs in ONE
// block, which goes on sub-level by sub-level (an LDS queue, __syncthreads between) until the
// queue drains, outgrows LDS or holds more than that; a larger one is a launch per row form and
// one host read of the tails.  A path of n vertices is n / 2 sub-levels of two vertices: a
// handful of host round trips instead of n / 2.
#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

namespace {

constexpr int kKcAgg = 2;            // shared fetch-adds tried per trip of the short form
// The in-block peel walks a wave-form or block-form row with the whole block, one row after
// another: a row's latency each, where a launch spreads them over the chip.  Such a row counts as
// this many short ones against kc_block (512 / 64: up to 8 of them stay in the block, about the
// 19 us a host-driven sub-level costs)
constexpr int kKcLongRow = 64;

// slots of the call's counters (u32): the removal queue's tails and, after an in-block peel, its
// heads, per row form; the alive pass's minimum and count; the compacted list's length; the
// largest simple degree and the vertices of simple degree 0
enum { Q_TAIL = 0, Q_HEAD = 3, K_MIN = 6, N_ALIVE = 7, N_LIST = 8, MAX_DEG = 9, N_CORE0 = 10, C_LEN = 12 };

// ---- build (the simple edges: lpa_adj.hip) ----
// the simple edge at position p: its two arcs at 2 p and 2 p + 1
__global__ __launch_bounds__(256) void k_kc_arcs(const u64* __restrict__ keys, const int32_t* __restrict__ first,
                                                 const int64_t* __restrict__ pos, int64_t m, u64* __restrict__ arcs) {
  GRID_STRIDE(i, m) {
    if (first[i]) {
      const u64 k = keys[i];
      arcs[2 * pos[i]] = k;
      arcs[2 * pos[i] + 1] = (k << 32) | (k >> 32);
    }
  }
}

// the live counts; cnt[MAX_DEG], cnt[N_CORE0]; the alive pass's slots at their start values
__global__ __launch_bounds__(256) void k_kc_init(const int64_t* __restrict__ off, int64_t V, int32_t* __restrict__ deg,
                                                 u32* __restrict__ cnt) {
  __shared__ u32 ws[2][4];
  u32 dmax = 0, zero = 0;
  GRID_STRIDE(v, V) {
    const u32 d = (u32)(off[v + 1] - off[v]);
    deg[v] = (int32_t)d;
    dmax = d > dmax ? d : dmax;
    zero += d == 0u ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const u32 x = (u32)__shfl_xor((int)dmax, o, 64);
    dmax = x > dmax ? x : dmax;
    zero += (u32)__shfl_xor((int)zero, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    ws[0][threadIdx.x >> 6] = dmax;
    ws[1][threadIdx.x >> 6] = zero;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      dmax = ws[0][i] > dmax ? ws[0][i] : dmax;
      zero += ws[1][i];
    }
    if (dmax) atomicMax(&cnt[MAX_DEG], dmax);
    if (zero) atomicAdd(&cnt[N_CORE0], zero);
  }
}

__global__ __launch_bounds__(256) void k_kc_degree_out(const int64_t* __restrict__ off, int64_t V,
                                                       int32_t* __restrict__ out) {
  GRID_STRIDE(v, V) out[v] = (int32_t)(off[v + 1] - off[v]);
}

// ---- peel ----
struct Peel {
  const int64_t* off;
  const int32_t* col;
  int32_t* deg;
  int32_t* core;
  uint8_t* dead;
  int32_t* queue;   // form f's rows at queue + f V, cnt[Q_TAIL + f] of them
  int64_t V;
  u32* cnt;
  int32_t k;        // the level
  int32_t fshort, fwave;
  __device__ __forceinline__ int form(int32_t v) const {
    const int64_t L = off[v + 1] - off[v];
    return L <= fshort ? 0 : L <= fwave ? 1 : 2;
  }
  // v leaves at this level.  Every vertex enters the queue once, so a form's list never passes
  // V entries; a slot past the end is not written and shows in the tails (the caller's check)
  // (returns v's form)
  __device__ __forceinline__ int remove(int32_t v) const {
    core[v] = k;
    dead[v] = 1;
    const int f = form(v);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (f == j) {
        const u32 p = atomicAdd(cnt + Q_TAIL + j, 1u);
        if ((int64_t)p < V) queue[(int64_t)j * V + p] = v;
      }
    return f;
  }
  // a dead u's neighbour w loses a neighbour; true for the one thread that removes w
  __device__ __forceinline__ bool take(int32_t w) const {
    if (dead[w]) return false;
    return __hip_atomic_fetch_add(deg + w, -1, LPA_RLX_AGENT) == k + 1;
  }
  // the same for a whole wave (every lane calls it; act: this lane has a w): the lanes that
  // hold the first active lane's w take their number from deg[w] in one add, and the add that
  // spans k + 1 -> k claims, for its leader
  __device__ __forceinline__ bool take_wave(bool act, int32_t w, int lane) const {
    bool mine = false;
    act = act && !dead[w];
#pragma unroll
    for (int it = 0; it < kKcAgg; ++it) {
      const u64 todo = __ballot(act);
      if (todo == 0ull) break;   // uniform
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const int32_t wl = __shfl(w, leader, 64);
      const bool same = act && w == wl;
      const int n = __popcll(__ballot(same));
      if (lane == leader) {
        const int32_t old = __hip_atomic_fetch_add(deg + wl, -n, LPA_RLX_AGENT);
        mine = old > k && old - n <= k;
      }
      if (same) act = false;
    }
    if (act) mine = __hip_atomic_fetch_add(deg + w, -1, LPA_RLX_AGENT) == k + 1;
    return mine;
  }
};

// the alive pass over list[0, n) (list == nullptr: the vertices 0 .. n - 1): the smallest live
// count among the alive and their number
__global__ __launch_bounds__(256) void k_kc_min(const int32_t* __restrict__ list, int64_t n,
                                                const int32_t* __restrict__ deg, const uint8_t* __restrict__ dead,
                                                u32* __restrict__ cnt) {
  __shared__ u32 ws[2][4];
  u32 lo = 0xFFFFFFFFu, alive = 0;
  GRID_STRIDE(i, n) {
    const int32_t v = list ? list[i] : (int32_t)i;
    if (!dead[v]) {
      const u32 d = (u32)deg[v];
      lo = d < lo ? d : lo;
      alive += 1;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const u32 x = (u32)__shfl_xor((int)lo, o, 64);
    lo = x < lo ? x : lo;
    alive += (u32)__shfl_xor((int)alive, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    ws[0][threadIdx.x >> 6] = lo;
    ws[1][threadIdx.x >> 6] = alive;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      lo = ws[0][i] < lo ? ws[0][i] : lo;
      alive += ws[1][i];
    }
    if (alive) {
      atomicMin(&cnt[K_MIN], lo);
      atomicAdd(&cnt[N_ALIVE], alive);
    }
  }
}

// the alive entries of list[0, n) to out[0, cnt[N_LIST]) (in no particular order)
__global__ __launch_bounds__(256) void k_kc_compact(const int32_t* __restrict__ list, int64_t n,
                                                    const uint8_t* __restrict__ dead, int32_t* __restrict__ out,
                                                    int64_t cap, u32* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const u64 lt = (1ull << lane) - 1ull;
  BLOCK_STRIDE(b, n) {
    const int64_t i = b + threadIdx.x;
    int32_t v = 0;
    bool act = i < n;
    if (act) {
      v = list ? list[i] : (int32_t)i;
      act = !dead[v];
    }
    const u64 mk = __ballot(act);
    if (mk == 0ull) continue;   // uniform over the wave
    u32 base = 0;
    if (lane == __ffsll((unsigned long long)mk) - 1) base = atomicAdd(&cnt[N_LIST], (u32)__popcll(mk));
    base = (u32)__shfl((int)base, __ffsll((unsigned long long)mk) - 1, 64);
    const int64_t p = (int64_t)base + __popcll(mk & lt);
    if (act && p < cap) out[p] = v;
  }
}

// the level's seeds; the alive pass's slots back at their start values for the next level
__global__ __launch_bounds__(256) void k_kc_seed(const int32_t* __restrict__ list, int64_t n, Peel p) {
  GRID_STRIDE(i, n) {
    const int32_t v = list ? list[i] : (int32_t)i;
    if (!p.dead[v] && p.deg[v] <= p.k) p.remove(v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    p.cnt[K_MIN] = 0xFFFFFFFFu;
    p.cnt[N_ALIVE] = 0u;
  }
}

// the cap: every vertex still alive gets max_k
__global__ __launch_bounds__(256) void k_kc_fill(const int32_t* __restrict__ list, int64_t n,
                                                 const uint8_t* __restrict__ dead, int32_t* __restrict__ core,
                                                 int32_t max_k) {
  GRID_STRIDE(i, n) {
    const int32_t v = list ? list[i] : (int32_t)i;
    if (!dead[v]) core[v] = max_k;
  }
}

// 8 lanes per queued row; the trips are uniform over the wave (take_wave)
__global__ __launch_bounds__(256) void k_kc_rows_short(const int32_t* __restrict__ rows, int64_t nrows, Peel p) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1), lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < nrows; base += (int64_t)gridDim.x * kRows) {
    const int64_t r = base + threadIdx.x / G;
    int64_t b = 0, L = 0;
    if (r < nrows) {
      const int32_t u = rows[r];
      b = p.off[u];
      L = p.off[u + 1] - b;
    }
    for (int64_t i = sub; __ballot(i < L) != 0ull; i += G) {
      const bool act = i < L;
      const int32_t w = act ? p.col[b + i] : 0;
      if (p.take_wave(act, w, lane)) p.remove(w);
    }
  }
}

__global__ __launch_bounds__(256) void k_kc_rows_wave(const int32_t* __restrict__ rows, int64_t nrows, Peel p) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (int64_t)gridDim.x * 4) {
    const int32_t u = rows[r];
    const int64_t b = p.off[u], L = p.off[u + 1] - b;
    for (int64_t i = lane; i < L; i += 64) {
      const int32_t w = p.col[b + i];
      if (p.take(w)) p.remove(w);
    }
  }
}

__global__ __launch_bounds__(kBlockThreads) void k_kc_rows_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                 Peel p) {
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const int32_t u = rows[r];
    const int64_t b = p.off[u], L = p.off[u + 1] - b;
    for (int64_t i = threadIdx.x; i < L; i += kBlockThreads) {
      const int32_t w = p.col[b + i];
      if (p.take(w)) p.remove(w);
    }
  }
}

// Sub-levels of one level in one block, from the queue's entries [h_f, tail_f) (at most
// kKcPeelCap in all, the caller's check).  A sub-level's vertices sit in q[cur]; a short row is
// one thread's, a longer one is set aside and walked by the whole block.  Ends when a sub-level
// removes nothing, more than q[] holds, or more than the block should take (`limit`, a longer
// row weighing kKcLongRow short ones: the caller's own test of the first sub-level): the heads
// it leaves (cnt[Q_HEAD + f]) tell the caller what is still to expand.
__global__ __launch_bounds__(kBlockThreads) void k_kc_peel_block(Peel p, u32 h0, u32 h1, u32 h2, u32 limit) {
  __shared__ int32_t q[2][kKcPeelCap];
  __shared__ int32_t big[kKcPeelCap];
  __shared__ u32 nq[2], nbig, nlong, hd[3];
  const int tid = threadIdx.x, lane = threadIdx.x & 63;
  {
    const u32 h[3] = {h0, h1, h2};
    u32 base = 0;
    for (int f = 0; f < 3; ++f) {
      const u32 t = __hip_atomic_load(p.cnt + Q_TAIL + f, LPA_RLX_AGENT);
      for (u32 i = h[f] + tid; i < t; i += kBlockThreads)
        if (base + (i - h[f]) < (u32)kKcPeelCap) q[0][base + (i - h[f])] = p.queue[(int64_t)f * p.V + i];
      base += t - h[f];
      if (tid == 0) hd[f] = t;
    }
    if (tid == 0) nq[0] = base < (u32)kKcPeelCap ? base : (u32)kKcPeelCap;
  }
  int cur = 0;
  while (true) {
    __syncthreads();   // q[cur], nq[cur] and hd are settled
    const u32 n = nq[cur];
    if (n == 0) break;
    if (tid == 0) {
      nq[cur ^ 1] = 0;
      nbig = 0;
      nlong = 0;
    }
    __syncthreads();
    int32_t* next = q[cur ^ 1];
    u32* nnext = &nq[cur ^ 1];
    for (u32 k0 = 0; k0 < n; k0 += kBlockThreads) {   // the same trips in every thread
      int64_t b = 0, L = 0;
      if (k0 + tid < n) {
        const int32_t u = q[cur][k0 + tid];
        if (p.form(u) == 0) {
          b = p.off[u];
          L = p.off[u + 1] - b;
        } else {
          big[atomicAdd(&nbig, 1u)] = u;
        }
      }
      for (int64_t i = 0; __ballot(i < L) != 0ull; ++i) {
        const bool act = i < L;
        const int32_t w = act ? p.col[b + i] : 0;
        if (p.take_wave(act, w, lane)) {
          if (p.remove(w) != 0) atomicAdd(&nlong, 1u);
          const u32 j = atomicAdd(nnext, 1u);
          if (j < (u32)kKcPeelCap) next[j] = w;
        }
      }
    }
    __syncthreads();
    const u32 nb = nbig;
    for (u32 r = 0; r < nb; ++r) {
      const int32_t u = big[r];
      const int64_t b = p.off[u], L = p.off[u + 1] - b;
      for (int64_t i = tid; i < L; i += kBlockThreads) {
        const int32_t w = p.col[b + i];
        if (p.take(w)) {
          if (p.remove(w) != 0) atomicAdd(&nlong, 1u);
          const u32 j = atomicAdd(nnext, 1u);
          if (j < (u32)kKcPeelCap) next[j] = w;
        }
      }
    }
    __syncthreads();   // every append of the sub-level has returned
    // outgrown, or too much for one block: hd stays at this sub-level's end
    if (nq[cur ^ 1] > (u32)kKcPeelCap || nq[cur ^ 1] + (u32)(kKcLongRow - 1) * nlong > limit) break;
    if (tid == 0)
      for (int f = 0; f < 3; ++f) hd[f] = __hip_atomic_load(p.cnt + Q_TAIL + f, LPA_RLX_AGENT);
    cur ^= 1;
  }
  if (tid == 0)
    for (int f = 0; f < 3; ++f) p.cnt[Q_HEAD + f] = hd[f];
}

// the queued rows [head[f], head[f] + n[f]) of every form f
void launch_rows(const Peel& p, const u32* head, const u32* n, hipStream_t s) {
  if (n[0])
    hipLaunchKernelGGL(k_kc_rows_short, dim3(grid_rows(n[0], 256 / kShortLanes, 65536)), dim3(256), 0, s,
                       p.queue + head[0], (int64_t)n[0], p);
  if (n[1])
    hipLaunchKernelGGL(k_kc_rows_wave, dim3(grid_rows(n[1], 4, 16384)), dim3(256), 0, s, p.queue + p.V + head[1],
                       (int64_t)n[1], p);
  if (n[2])
    hipLaunchKernelGGL(k_kc_rows_block, dim3(grid_rows(n[2], 1, 4096)), dim3(kBlockThreads), 0, s,
                       p.queue + 2 * p.V + head[2], (int64_t)n[2], p);
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream and the kc_* knobs of the handle, nothing of the LPA
// state; every array is a stream-ordered temporary.
int core_numbers(lpa_graph* g, int32_t max_k, int32_t* core_out, int32_t* simple_degree_out, int32_t out_is_device,
                 lpa_core_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  if (summary) *summary = lpa_core_summary{0, 0, 0, 0, 0, 0, 0};
  if (V == 0) return LPA_OK;
  Tmp tmp(s);
  // ---- build ----
  SimpleEdges se;   // keys [2 m]: the edge keys and the sorts' other buffer
  LPA_TRY(simple_edges(g, tmp, &se));
  const int64_t E = se.E;
  int64_t* off = nullptr;
  int32_t* col = nullptr;
  LPA_TRY(tmp.get(&off, V + 1));
  LPA_TRY(tmp.get(&col, 2 * E));
  if (E > 0) {
    const HalfShifts sh(bits_for((uint64_t)(V - 1)));
    u64* arcs = nullptr;
    LPA_TRY(tmp.get(&arcs, 2 * E));
    hipLaunchKernelGGL(k_kc_arcs, dim3(grid_for(m)), dim3(256), 0, s, se.keys, se.first, se.pos, m, arcs);
    LPA_HIP(hipGetLastError());
    // the edge keys are spent: keys[0, 2 E) is the sort's other buffer (E <= m)
    LPA_TRY(radix_sort_u64(arcs, se.keys, 2 * E, sh.hi(), sh.ns, s));
    LPA_TRY(key_bounds(arcs, 2 * E, V, true, off, s));
    LPA_TRY(key_col(arcs, 2 * E, col, s));
  } else {
    LPA_HIP(hipMemsetAsync(off, 0, sizeof(int64_t) * (size_t)(V + 1), s));
  }
  // ---- state ----
  int32_t *deg = nullptr, *queue = nullptr, *lists = nullptr, *core = core_out;
  uint8_t* dead = nullptr;
  u32* cnt = nullptr;
  LPA_TRY(tmp.get(&deg, V));
  LPA_TRY(tmp.get(&dead, V));
  LPA_TRY(tmp.get(&cnt, C_LEN));
  if (!out_is_device) LPA_TRY(tmp.get(&core, V));
  u32* pinned = nullptr;
  LPA_TRY(tmp.pin(&pinned, C_LEN));
  LPA_HIP(hipMemsetAsync(dead, 0, (size_t)V, s));
  LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(u32) * C_LEN, s));
  LPA_HIP(hipMemsetAsync(cnt + K_MIN, 0xFF, sizeof(u32), s));
  hipLaunchKernelGGL(k_kc_init, dim3(grid_bh(V)), dim3(256), 0, s, off, V, deg, cnt);
  LPA_HIP(hipGetLastError());
  const volatile u32* hc = pinned;
  const auto read_counts = [&]() -> int {
    LPA_HIP(hipMemcpyAsync(pinned, cnt, sizeof(u32) * C_LEN, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipStreamSynchronize(s));
    return LPA_OK;
  };
  // ---- peel ----
  int64_t passes = 0, levels = 0, removed = 0, alive = V, last_size = 0;
  int32_t last_k = 0;
  bool capped = max_k == 0;
  if (max_k > 0) {
    LPA_TRY(tmp.get(&queue, 3 * V));
    LPA_TRY(tmp.get(&lists, 2 * V));   // the alive list and the buffer its compaction writes
    Peel p{off, col, deg, core, dead, queue, V, cnt, 0, g->kc_short, g->kc_wave};
    const int64_t in_block = g->kc_block < kKcPeelCap ? g->kc_block : kKcPeelCap;
    const int32_t* list = nullptr;   // nullptr: every vertex
    int64_t list_len = V;
    int which = 0;
    u32 head[3] = {0, 0, 0}, tail[3] = {0, 0, 0};
    while (true) {
      hipLaunchKernelGGL(k_kc_min, dim3(grid_bh(list_len)), dim3(256), 0, s, list, list_len, deg, dead, cnt);
      LPA_HIP(hipGetLastError());
      LPA_TRY(read_counts());
      ++passes;
      alive = (int64_t)hc[N_ALIVE];
      if (alive == 0) break;
      if ((int64_t)hc[K_MIN] >= (int64_t)max_k) {
        capped = true;
        hipLaunchKernelGGL(k_kc_fill, dim3(grid_for(list_len)), dim3(256), 0, s, list, list_len, dead, core, max_k);
        LPA_HIP(hipGetLastError());
        break;
      }
      p.k = (int32_t)hc[K_MIN];
      if (2 * alive <= list_len) {
        int32_t* out = lists + (int64_t)which * V;
        LPA_HIP(hipMemsetAsync(cnt + N_LIST, 0, sizeof(u32), s));
        hipLaunchKernelGGL(k_kc_compact, dim3(grid_bh(list_len)), dim3(256), 0, s, list, list_len, dead, out, alive,
                           cnt);
        LPA_HIP(hipGetLastError());
        list = out;
        list_len = alive;
        which ^= 1;
      }
      hipLaunchKernelGGL(k_kc_seed, dim3(grid_for(list_len)), dim3(256), 0, s, list, list_len, p);
      LPA_HIP(hipGetLastError());
      LPA_TRY(read_counts());
      ++passes;
      for (int f = 0; f < 3; ++f) tail[f] = hc[Q_TAIL + f];
      // ---- expand until the queue drains ----
      while (true) {
        const u32 n[3] = {tail[0] - head[0], tail[1] - head[1], tail[2] - head[2]};
        const int64_t pending = (int64_t)n[0] + n[1] + n[2];
        if (pending == 0) break;
        if (pending + (int64_t)(kKcLongRow - 1) * ((int64_t)n[1] + n[2]) <= in_block) {
          hipLaunchKernelGGL(k_kc_peel_block, dim3(1), dim3(kBlockThreads), 0, s, p, head[0], head[1], head[2],
                             (u32)in_block);
          LPA_HIP(hipGetLastError());
          LPA_TRY(read_counts());
          for (int f = 0; f < 3; ++f) head[f] = hc[Q_HEAD + f];
        } else {
          launch_rows(p, head, n, s);
          LPA_HIP(hipGetLastError());
          LPA_TRY(read_counts());
          for (int f = 0; f < 3; ++f) head[f] = tail[f];
        }
        ++passes;
        for (int f = 0; f < 3; ++f) tail[f] = hc[Q_TAIL + f];
        if ((int64_t)tail[0] + tail[1] + tail[2] > V) break;   // the check below reports it
      }
      const int64_t gone = (int64_t)tail[0] + tail[1] + tail[2];
      last_size = gone - removed;
      removed = gone;
      last_k = p.k;
      ++levels;
      if (removed >= V) {   // nobody is left: the next alive pass would only say so
        alive = 0;
        break;
      }
    }
  } else {
    LPA_HIP(hipMemsetAsync(core, 0, sizeof(int32_t) * (size_t)V, s));
  }
  if (removed + (capped ? alive : 0) != V) {
    LPA_HIP(hipStreamSynchronize(s));
    set_error("core_numbers: the removal queue holds %lld entries for %lld peeled vertices", (long long)removed,
              (long long)(V - (capped ? alive : 0)));
    return LPA_EOVERFLOW;
  }
  // ---- the outputs ----
  if (simple_degree_out) {
    int32_t* sd = simple_degree_out;
    if (!out_is_device) LPA_TRY(tmp.get(&sd, V));
    hipLaunchKernelGGL(k_kc_degree_out, dim3(grid_for(V)), dim3(256), 0, s, off, V, sd);
    LPA_HIP(hipGetLastError());
    if (!out_is_device)
      LPA_HIP(hipMemcpyAsync(simple_degree_out, sd, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  }
  if (!out_is_device) LPA_HIP(hipMemcpyAsync(core_out, core, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  LPA_TRY(read_counts());
  if (summary) {
    summary->degeneracy = capped ? (int64_t)max_k : (int64_t)last_k;
    summary->main_core_size = capped ? alive : last_size;
    summary->levels = levels + (capped ? 1 : 0);
    summary->simple_edges = E;
    summary->max_degree = (int64_t)hc[MAX_DEG];
    summary->n_core0 = (int64_t)hc[N_CORE0];
    summary->passes = passes;
  }
  return LPA_OK;
}

}  // namespace lpa
