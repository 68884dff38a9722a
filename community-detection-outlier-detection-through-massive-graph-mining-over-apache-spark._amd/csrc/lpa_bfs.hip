// Breadth-first search between two vertex sets of the handle's directed input graph
// (GraphFrame.bfs, GraphFrames lib.BFS): F = the vertices of from_mask, T = those of to_mask,
// the kept edges those of edge_keep.  L = the fewest kept non-loop edges on a directed path
// src -> dst from F to T; the result is the DAG of EVERY path of L edges: lev[v] = the place of
// v on such a path (-1 off them), on_edge[e] = input edge e lies on one.  The host enumerates
// the paths (their number is the size of the output).  Integers throughout.
//
// One bit per vertex: the bitmaps seen, front, next and tbits hold ceil(V / 64) 64-bit words, a
// wave64 ballot's width, word t = the vertices 64 t .. 64 t + 63 (2 MB at V = 2^24).
//
//   build    the E distinct non-loop arcs of the KEPT edges (lpa_adj.hip: arcs_count with the
//            keep mask, arcs_lists): the out-lists oo / ocol, for the push and the backward
//            sweep, and the in-lists io / icol, for the pull.  Offsets int64, ids int32
//   bits     next = the ballots of from_mask, tbits = those of to_mask; seen = 0, lev = -1
//   level    settle, read seven counts on the host, stop, else expand
//   settle   new = next & ~seen; seen |= new; front = new; next = 0, a wave per word; the lane
//            of a set bit stores lev[v] = level.  Also counts, block-reduced: the frontier's
//            vertices (and how many of each push form), its out-arcs, the in-arcs of the
//            vertices still unseen, the words in which new & tbits is not 0
//   stop     at the first level whose settle reports a word with a target: L = level; at an
//            empty frontier or at level == max_len: no path
//   push     (small frontier) the frontier compacted into one list per row form; every listed
//            u walks its out-list: a target whose seen bit is clear gets its bit ORed into its
//            next word, a relaxed agent-scope 64-bit atomic OR, skipped when a read of the word
//            shows the bit already there
//   pull     (large frontier) every unseen v scans its in-list and stops at the first u with
//            the front bit.  Short rows: a lane per vertex, a wave per word; the ballot of the
//            hits is the next word of those 64 vertices, stored once, no atomics.  Wave and
//            block rows (static lists, built once a call) run after it and OR their one bit
//            into the word the short form stored: one atomic per long row that was hit
//   sweep    lev[v] = -1 where lev[v] == L and v is not in T; then for l = L - 1 .. 0 every v
//            with lev[v] == l scans its out-list for a w with lev[w] == l + 1 and takes -1 when
//            there is none.  A pull over out-lists, no atomics; what is left >= 0 is on a path
//   mark     per input edge: on_edge[e] = kept, in range, no loop, lev[src] >= 0 and
//            lev[dst] == lev[src] + 1.  Plain byte stores, the count block-reduced
//
// The sweep keeps no bitmap of its own (the "on" set): a vertex that is off every path loses its
// level at once, so "w is on, at level l + 1" is the one test lev[w] == l + 1, and the mark
// reads lev alone.  That is a subset of the loads a separate bitmap would need.
//
// Row forms, by list length (kSpShort / kSpWave, the shortest paths' constants):
//   short   <= kSpShort   push and sweep: 8 lanes per row; pull: a lane per row (the ballot)
//   wave    <= kSpWave    a wave per listed row
//   block   above         a block of 1024 per listed row
// The pull's and the sweep's lists are static (by in-degree, by out-degree); the push's are the
// frontier's, rebuilt on every push level.
//
// Invariants.  seen, front, tbits and the offsets are written by settle, bits and the build
// only, never by an expansion, so an expansion reads them as of the kernel boundary before it.
// next is 0 outside an expansion and its settle.  front is a subset of seen; the bit of v is
// set in seen exactly when lev[v] >= 0 (until the sweep).  Bits past V are never set.
//
// Why the interleaving does not matter.  After level k, next & ~seen has the bit of v exactly
// when an arc u -> v leaves a frontier vertex u and v is unseen, whatever computed it: OR is
// commutative, associative and idempotent, so the order of the atomics, the order of a
// compacted list (its positions come from an atomic cursor), a pull that stops at its first
// hit, a skipped atomic (the bit was there) and the push / pull choice all give the same word.
// By induction over the levels seen, front and lev are functions of (V, kept arc set, F)
// alone, and the stop is a function of those and (T, max_len).  The sweep's level l reads only
// levels l + 1 (final since the pass before) and l (each vertex its own): a fixpoint per level,
// whatever the order.  Only push_levels / pull_levels tell the schedule; their sum is L when a
// path is found, else the levels expanded.
#include <chrono>
#include <cstdio>
#include <cstring>

#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

namespace {

constexpr int kBfsBeta = 24;        // back to the push when the frontier falls below V / kBfsBeta

// slots of the per-level counters
enum { C_FRONT = 0, C_SHORT = 1, C_WAVE = 2, C_BLOCK = 3, C_OUT_ARCS = 4, C_IN_ARCS = 5, C_HIT = 6, C_READ = 7,
       C_CURSOR = 7, C_LEN = 10 };
// slots of the result counters
enum { R_VERTS = 0, R_EDGES = 1, R_LEN = 2 };

__device__ __forceinline__ ull bfs_wave_add(ull x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ bool bfs_bit(const ull* __restrict__ bits, int64_t v) {
  return (bits[v >> 6] >> (v & 63)) & 1ull;
}
// lev in the sweep: a level's pass stores -1 to vertices of that level while other waves read
// them (as "not l + 1" either way): relaxed agent-scope accesses, no ordering needed
__device__ __forceinline__ int32_t bfs_lev(const int32_t* lev, int64_t v) {
  return __hip_atomic_load(lev + v, LPA_RLX_AGENT);
}
__device__ __forceinline__ void bfs_drop(int32_t* lev, int64_t v) {
  __hip_atomic_store(lev + v, -1, LPA_RLX_AGENT);
}

// ---- bits: the masks as bitmaps, a wave per word (lanes past V vote 0) ----
__global__ __launch_bounds__(256) void k_bfs_bits(const uint8_t* __restrict__ from, const uint8_t* __restrict__ to,
                                                  int64_t V, ull* __restrict__ next, ull* __restrict__ tbits) {
  const int lane = threadIdx.x & 63;
  const int64_t tiles = (V + 63) >> 6;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const int64_t v = t * 64 + lane;
    const ull fw = __ballot(v < V && from[v] != 0), tw = __ballot(v < V && to[v] != 0);
    if (lane == 0) {
      next[t] = fw;
      tbits[t] = tw;
    }
  }
}

// One level's settle, a wave per word: every lane reads the word, lane 0 writes it back
__global__ __launch_bounds__(256) void k_bfs_settle(ull* __restrict__ seen, ull* __restrict__ front,
                                                    ull* __restrict__ next, const ull* __restrict__ tbits,
                                                    const int64_t* __restrict__ oo, const int64_t* __restrict__ io,
                                                    int64_t V, int32_t level, int32_t* __restrict__ lev,
                                                    ull* __restrict__ cnt) {
  __shared__ ull ws[4][C_READ];
  ull c[C_READ] = {0, 0, 0, 0, 0, 0, 0};
  const int lane = threadIdx.x & 63;
  const int64_t tiles = (V + 63) >> 6;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const int64_t v = t * 64 + lane;
    const ull sn = seen[t], nx = next[t];
    const ull nw = nx & ~sn, s2 = sn | nw;
    if (lane == 0) {
      if (nw) seen[t] = s2;
      front[t] = nw;
      if (nx) next[t] = 0;
      if (nw & tbits[t]) c[C_HIT] += 1;
    }
    if (v < V) {
      if ((nw >> lane) & 1ull) {
        lev[v] = level;
        const int64_t L = oo[v + 1] - oo[v];
        c[C_FRONT] += 1;
        c[C_SHORT] += L > 0 && L <= kSpShort ? 1 : 0;
        c[C_WAVE] += L > kSpShort && L <= kSpWave ? 1 : 0;
        c[C_BLOCK] += L > kSpWave ? 1 : 0;
        c[C_OUT_ARCS] += (ull)L;
      } else if (!((s2 >> lane) & 1ull)) {
        c[C_IN_ARCS] += (ull)(io[v + 1] - io[v]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < C_READ; ++k) {
    const ull x = bfs_wave_add(c[k]);
    if (lane == 0) ws[threadIdx.x >> 6][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < C_READ) {
    const ull x = ws[0][threadIdx.x] + ws[1][threadIdx.x] + ws[2][threadIdx.x] + ws[3][threadIdx.x];
    if (x) atomicAdd(&cnt[threadIdx.x], x);
  }
}

// the frontier compacted by push form: short rows in lists, wave rows in lists + V, block
// rows in lists + 2 V (a row without out-arcs is in none); one cursor add per wave and form
__global__ __launch_bounds__(256) void k_bfs_lists(const ull* __restrict__ front, const int64_t* __restrict__ oo,
                                                   int64_t V, int32_t* __restrict__ lists, ull* __restrict__ cursor) {
  const int lane = threadIdx.x & 63;
  const ull below = (1ull << lane) - 1;
  const int64_t tiles = (V + 63) >> 6;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const ull fw = front[t];
    if (fw == 0) continue;   // the same in every lane
    const int64_t v = t * 64 + lane;
    int form = -1;
    if ((fw >> lane) & 1ull) {   // a set bit is a vertex: v < V
      const int64_t L = oo[v + 1] - oo[v];
      form = L == 0 ? -1 : L <= kSpShort ? 0 : L <= kSpWave ? 1 : 2;
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const ull mask = __ballot(form == f);
      if (mask == 0) continue;
      ull base = 0;
      if (lane == 0) base = atomicAdd(&cursor[f], (ull)__popcll(mask));
      base = __shfl(base, 0, 64);
      if (form == f) lists[(int64_t)f * V + (int64_t)base + __popcll(mask & below)] = (int32_t)v;
    }
  }
}

// ---- push: listed frontier rows walk their out-lists ----
__device__ __forceinline__ void bfs_visit(int32_t p, const ull* __restrict__ seen, ull* next) {
  const int64_t w = p >> 6;
  const ull bit = 1ull << (p & 63);
  if (seen[w] & bit) return;
  if (__hip_atomic_load(next + w, LPA_RLX_AGENT) & bit) return;
  __hip_atomic_fetch_or(next + w, bit, LPA_RLX_AGENT);
}

__global__ __launch_bounds__(256) void k_bfs_push_short(const int32_t* __restrict__ rows, int64_t nrows,
                                                        const int64_t* __restrict__ oo,
                                                        const int32_t* __restrict__ ocol,
                                                        const ull* __restrict__ seen, ull* next) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t k = (int64_t)blockIdx.x * kRows + threadIdx.x / G; k < nrows; k += (int64_t)gridDim.x * kRows) {
    const int64_t u = rows[k];
    const int64_t b = oo[u], L = oo[u + 1] - b;
    for (int64_t i = sub; i < L; i += G) bfs_visit(ocol[b + i], seen, next);
  }
}

__global__ __launch_bounds__(256) void k_bfs_push_wave(const int32_t* __restrict__ rows, int64_t nrows,
                                                       const int64_t* __restrict__ oo,
                                                       const int32_t* __restrict__ ocol,
                                                       const ull* __restrict__ seen, ull* next) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t u = rows[k];
    const int64_t b = oo[u], L = oo[u + 1] - b;
    for (int64_t i = lane; i < L; i += 64) bfs_visit(ocol[b + i], seen, next);
  }
}

__global__ __launch_bounds__(kBlockThreads) void k_bfs_push_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                  const int64_t* __restrict__ oo,
                                                                  const int32_t* __restrict__ ocol,
                                                                  const ull* __restrict__ seen, ull* next) {
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t u = rows[k];
    const int64_t b = oo[u], L = oo[u + 1] - b;
    for (int64_t i = threadIdx.x; i < L; i += kBlockThreads) bfs_visit(ocol[b + i], seen, next);
  }
}

// ---- pull: unseen rows scan their in-lists up to the first frontier vertex ----
// a wave per word, a lane per vertex; a longer row is not this form's (its bit stays 0 here)
__global__ __launch_bounds__(256) void k_bfs_pull_short(const int64_t* __restrict__ io,
                                                        const int32_t* __restrict__ icol, int64_t V,
                                                        const ull* __restrict__ seen, const ull* __restrict__ front,
                                                        ull* __restrict__ next) {
  const int lane = threadIdx.x & 63;
  const int64_t tiles = (V + 63) >> 6;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const int64_t v = t * 64 + lane;
    bool hit = false;
    if (v < V && !((seen[t] >> lane) & 1ull)) {
      const int64_t b = io[v], L = io[v + 1] - b;
      if (L <= kSpShort)
        for (int64_t i = 0; i < L; ++i)
          if (bfs_bit(front, icol[b + i])) {
            hit = true;
            break;
          }
    }
    const ull word = __ballot(hit);
    if (lane == 0 && word) next[t] = word;   // next is 0 before an expansion
  }
}

// this wave's share of a row of L entries at col + b, 256 entries a step from `first`,
// `stride` entries on: does one of them have its bit in `bits`?  Stops after the step that
// finds one (the answer is the same in every lane)
__device__ __forceinline__ bool bfs_scan_bits(const int32_t* __restrict__ col, const ull* __restrict__ bits, int64_t b,
                                              int64_t L, int64_t first, int64_t stride, int lane) {
  for (int64_t i0 = first; i0 < L; i0 += stride) {
    bool hit = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = i0 + j * 64 + lane;
      if (i < L) hit |= bfs_bit(bits, col[b + i]);
    }
    if (__ballot(hit)) return true;
  }
  return false;
}

// a wave per listed row; runs after the short form, which stored the row's word
__global__ __launch_bounds__(256) void k_bfs_pull_wave(const int32_t* __restrict__ rows, int64_t nrows,
                                                       const int64_t* __restrict__ io,
                                                       const int32_t* __restrict__ icol, const ull* __restrict__ seen,
                                                       const ull* __restrict__ front, ull* next) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t v = rows[k];
    if (bfs_bit(seen, v)) continue;
    const int64_t b = io[v];
    const bool hit = bfs_scan_bits(icol, front, b, io[v + 1] - b, 0, 256, lane);
    if (hit && lane == 0) __hip_atomic_fetch_or(next + (v >> 6), 1ull << (v & 63), LPA_RLX_AGENT);
  }
}

// a block per listed row (k and the seen bit are the same in every thread: barriers inside);
// every wave stops on its own
__global__ __launch_bounds__(kBlockThreads) void k_bfs_pull_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                  const int64_t* __restrict__ io,
                                                                  const int32_t* __restrict__ icol,
                                                                  const ull* __restrict__ seen,
                                                                  const ull* __restrict__ front, ull* next) {
  constexpr int kWaves = kBlockThreads / 64;
  __shared__ int ws[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t v = rows[k];
    if (bfs_bit(seen, v)) continue;
    const int64_t b = io[v];
    const bool hit = bfs_scan_bits(icol, front, b, io[v + 1] - b, (int64_t)wave * 256, (int64_t)kWaves * 256, lane);
    if (lane == 0) ws[wave] = hit ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
      int any = 0;
      for (int i = 0; i < kWaves; ++i) any |= ws[i];
      if (any) __hip_atomic_fetch_or(next + (v >> 6), 1ull << (v & 63), LPA_RLX_AGENT);
    }
    __syncthreads();   // before the next row rewrites ws
  }
}

// ---- the backward sweep ----
// level L keeps its targets only
__global__ __launch_bounds__(256) void k_bfs_tail(int32_t* __restrict__ lev, const ull* __restrict__ tbits, int64_t V,
                                                  int32_t L) {
  GRID_STRIDE(v, V) {
    if (lev[v] == L && !bfs_bit(tbits, v)) lev[v] = -1;
  }
}

// every row in id order, kShortLanes lanes each; a longer row is not this form's.  A row of
// level l without an arc to level l + 1 (a row without arcs too) loses its level
__global__ __launch_bounds__(256) void k_bfs_back_short(const int64_t* __restrict__ oo,
                                                        const int32_t* __restrict__ ocol, int64_t V, int32_t l,
                                                        int32_t* lev) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < V; base += (int64_t)gridDim.x * kRows) {
    const int64_t v = base + threadIdx.x / G;
    bool mine = false;
    int hit = 0;
    if (v < V && bfs_lev(lev, v) == l) {
      const int64_t b = oo[v], L = oo[v + 1] - b;
      mine = L <= kSpShort;
      if (mine)
        for (int64_t i = sub; i < L; i += G)
          if (bfs_lev(lev, ocol[b + i]) == l + 1) {
            hit = 1;
            break;
          }
    }
    // the G lanes of a row are neighbours: every one of them ends with the row's answer
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) hit |= __shfl_xor(hit, off, 64);
    if (mine && sub == 0 && !hit) bfs_drop(lev, v);
  }
}

// as bfs_scan_bits, for "lev == want"
__device__ __forceinline__ bool bfs_scan_lev(const int32_t* __restrict__ col, const int32_t* lev, int64_t b, int64_t L,
                                             int64_t first, int64_t stride, int32_t want, int lane) {
  for (int64_t i0 = first; i0 < L; i0 += stride) {
    bool hit = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = i0 + j * 64 + lane;
      if (i < L) hit |= bfs_lev(lev, col[b + i]) == want;
    }
    if (__ballot(hit)) return true;
  }
  return false;
}

__global__ __launch_bounds__(256) void k_bfs_back_wave(const int32_t* __restrict__ rows, int64_t nrows,
                                                       const int64_t* __restrict__ oo,
                                                       const int32_t* __restrict__ ocol, int32_t l, int32_t* lev) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t v = rows[k];
    if (bfs_lev(lev, v) != l) continue;
    const int64_t b = oo[v];
    const bool hit = bfs_scan_lev(ocol, lev, b, oo[v + 1] - b, 0, 256, l + 1, lane);
    if (!hit && lane == 0) bfs_drop(lev, v);
  }
}

// a block per listed row (k and the row's level are the same in every thread: barriers inside;
// only thread 0 writes the row's level, after the first barrier)
__global__ __launch_bounds__(kBlockThreads) void k_bfs_back_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                  const int64_t* __restrict__ oo,
                                                                  const int32_t* __restrict__ ocol, int32_t l,
                                                                  int32_t* lev) {
  constexpr int kWaves = kBlockThreads / 64;
  __shared__ int ws[kWaves];
  __shared__ int row_level;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t v = rows[k];
    if (threadIdx.x == 0) row_level = bfs_lev(lev, v);
    __syncthreads();
    const bool mine = row_level == l;   // one read for the block: the same in every thread
    if (mine) {
      const int64_t b = oo[v];
      const bool hit = bfs_scan_lev(ocol, lev, b, oo[v + 1] - b, (int64_t)wave * 256, (int64_t)kWaves * 256, l + 1,
                                    lane);
      if (lane == 0) ws[wave] = hit ? 1 : 0;
    }
    __syncthreads();
    if (mine && threadIdx.x == 0) {
      int any = 0;
      for (int i = 0; i < kWaves; ++i) any |= ws[i];
      if (!any) bfs_drop(lev, v);
    }
    __syncthreads();   // before the next row rewrites ws and row_level
  }
}

// ---- mark ----
// res[R_EDGES] += the edges marked
__global__ __launch_bounds__(256) void k_bfs_mark(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                  const uint8_t* __restrict__ keep, int64_t m, u32 V,
                                                  const int32_t* __restrict__ lev, uint8_t* __restrict__ on_edge,
                                                  ull* __restrict__ res) {
  __shared__ ull ws[4];
  ull n = 0;
  GRID_STRIDE(e, m) {
    const u32 a = (u32)src[e], b = (u32)dst[e];
    bool on = a < V && b < V && a != b && (keep == nullptr || keep[e] != 0);
    if (on) {
      const int32_t la = lev[a];
      on = la >= 0 && lev[b] == la + 1;
    }
    on_edge[e] = on ? 1 : 0;
    n += on ? 1 : 0;
  }
  n = bfs_wave_add(n);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    n = ws[0] + ws[1] + ws[2] + ws[3];
    if (n) atomicAdd(&res[R_EDGES], n);
  }
}

// res[R_VERTS] += the vertices that kept a level
__global__ __launch_bounds__(256) void k_bfs_count(const int32_t* __restrict__ lev, int64_t V, ull* __restrict__ res) {
  __shared__ ull ws[4];
  ull n = 0;
  GRID_STRIDE(v, V) n += lev[v] >= 0 ? 1 : 0;
  n = bfs_wave_add(n);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    n = ws[0] + ws[1] + ws[2] + ws[3];
    if (n) atomicAdd(&res[R_VERTS], n);
  }
}

// |F|, |T| and |F n T| of the two host masks, eight bytes a step (most words are 0)
void bfs_count_sets(const uint8_t* from, const uint8_t* to, int64_t n, int64_t* n_from, int64_t* n_to,
                    int64_t* n_both) {
  constexpr uint64_t k7 = 0x7F7F7F7F7F7F7F7Full, k8 = 0x8080808080808080ull;
  int64_t a = 0, b = 0, c = 0, i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t x, y;
    memcpy(&x, from + i, 8);
    memcpy(&y, to + i, 8);
    if ((x | y) == 0) continue;
    // bit 7 of every nonzero byte: the low seven bits carry into it, the byte's own bit 7 is ORed in
    const uint64_t p = (((x & k7) + k7) | x) & k8, q = (((y & k7) + k7) | y) & k8;
    a += __builtin_popcountll(p);
    b += __builtin_popcountll(q);
    c += __builtin_popcountll(p & q);
  }
  for (; i < n; ++i) {
    const bool f = from[i] != 0, t = to[i] != 0;
    a += f;
    b += t;
    c += f && t;
  }
  *n_from = a;
  *n_to = b;
  *n_both = c;
}

double bfs_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream and bfs_alpha / bfs_pull / bfs_times of the handle,
// nothing of the LPA state; every array is a stream-ordered temporary.  max_len >= 0, the
// masks and the outputs are there when V > 0 (m > 0), checked by the caller.  ms: the stage
// clocks (sets, build, forward, backward, mark)
static int bfs_run(lpa_graph* g, const uint8_t* from_mask, const uint8_t* to_mask, const uint8_t* edge_keep,
                   int32_t max_len, int32_t* level_out, uint8_t* on_edge_out, lpa_bfs_summary* summary, double* ms) {
  const auto t_sets = std::chrono::steady_clock::now();
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  lpa_bfs_summary sm = {0, 0, 0, -1, 0, 0, 0, 0, 0};
  if (summary) *summary = sm;
  if (V == 0) return LPA_OK;
  // ---- the sets, on the host: the cases without a search ----
  int64_t nF = 0, nT = 0, nFT = 0;
  bfs_count_sets(from_mask, to_mask, V, &nF, &nT, &nFT);
  sm.sources = nF;
  sm.targets = nT;
  const bool both = nF > 0 && nT > 0;
  if (both) sm.reached = nF;   // level 0
  // the outputs of a call that marks nothing: length 0 (the common vertices at level 0) or -1
  auto plain_outputs = [&]() {
    memset(level_out, 0xFF, sizeof(int32_t) * (size_t)V);
    if (m > 0) memset(on_edge_out, 0, (size_t)m);
    if (nFT > 0)
      for (int64_t v = 0; v < V; ++v)
        if (from_mask[v] != 0 && to_mask[v] != 0) level_out[v] = 0;
  };
  if (nFT > 0) {
    sm.length = 0;
    sm.path_vertices = nFT;
  }
  const bool search = both && nFT == 0 && max_len > 0;
  if (!search) plain_outputs();
  if (!search && !summary) return LPA_OK;
  ms[0] = bfs_ms_since(t_sets);
  const auto t0 = std::chrono::steady_clock::now();
  Tmp tmp(s);
  // ---- build ----
  uint8_t* keep = nullptr;
  if (edge_keep && m > 0) {
    LPA_TRY(tmp.get(&keep, m));
    LPA_HIP(hipMemcpyAsync(keep, edge_keep, (size_t)m, hipMemcpyHostToDevice, s));
  }
  ArcLists arcs;
  LPA_TRY(arcs_count(g, tmp, nullptr, &arcs, keep));
  sm.arcs = arcs.E;
  if (!search) {
    *summary = sm;
    return LPA_OK;
  }
  LPA_TRY(arcs_lists(g, tmp, &arcs));
  const int64_t *oo = arcs.oo, *io = arcs.io;
  const int32_t *ocol = arcs.ocol, *icol = arcs.icol;
  // the static lists: the pull's by in-degree, the sweep's by out-degree
  int32_t *plists = nullptr, *blists = nullptr;
  u32 hp[2] = {0, 0}, hb[2] = {0, 0};   // their wave rows and block rows (read after the synchronisation below)
  LPA_TRY(form_lists(tmp, io, V, kSpShort, kSpWave, &plists, hp));
  LPA_TRY(form_lists(tmp, oo, V, kSpShort, kSpWave, &blists, hb));
  // ---- state ----
  const int64_t tiles = (V + 63) >> 6;
  ull *seen = nullptr, *front = nullptr, *next = nullptr, *tbits = nullptr, *cnt = nullptr, *res = nullptr;
  int32_t *lev = nullptr, *flists = nullptr;
  uint8_t *dfrom = nullptr, *dto = nullptr, *don = nullptr;
  LPA_TRY(tmp.get(&seen, tiles));
  LPA_TRY(tmp.get(&front, tiles));
  LPA_TRY(tmp.get(&next, tiles));
  LPA_TRY(tmp.get(&tbits, tiles));
  LPA_TRY(tmp.get(&cnt, C_LEN));
  LPA_TRY(tmp.get(&res, R_LEN));
  LPA_TRY(tmp.get(&lev, V));
  LPA_TRY(tmp.get(&flists, 3 * V));
  LPA_TRY(tmp.get(&dfrom, V));
  LPA_TRY(tmp.get(&dto, V));
  LPA_TRY(tmp.get(&don, m));
  ull* pinned = nullptr;
  LPA_TRY(tmp.pin(&pinned, C_READ));
  const unsigned g_tiles = grid_rows(tiles, 4, 8192);
  const unsigned g_short = grid_rows(V, 256 / kShortLanes, 65536);
  LPA_HIP(hipMemcpyAsync(dfrom, from_mask, (size_t)V, hipMemcpyHostToDevice, s));
  LPA_HIP(hipMemcpyAsync(dto, to_mask, (size_t)V, hipMemcpyHostToDevice, s));
  LPA_HIP(hipMemsetAsync(lev, 0xFF, sizeof(int32_t) * (size_t)V, s));
  LPA_HIP(hipMemsetAsync(seen, 0, sizeof(ull) * (size_t)tiles, s));
  hipLaunchKernelGGL(k_bfs_bits, dim3(g_tiles), dim3(256), 0, s, dfrom, dto, V, next, tbits);
  LPA_HIP(hipGetLastError());
  LPA_HIP(hipStreamSynchronize(s));
  ms[1] = bfs_ms_since(t0);
  const auto t1 = std::chrono::steady_clock::now();
  // ---- forward ----
  const volatile ull* hc = pinned;
  int64_t reached = 0, found = -1, n_push = 0, n_pull = 0;
  bool pull = g->bfs_pull != 0;
  for (int32_t level = 0;; ++level) {
    LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(ull) * C_LEN, s));
    hipLaunchKernelGGL(k_bfs_settle, dim3(g_tiles), dim3(256), 0, s, seen, front, next, tbits, oo, io, V, level, lev,
                       cnt);
    LPA_HIP(hipGetLastError());
    LPA_HIP(hipMemcpyAsync(pinned, cnt, sizeof(ull) * C_READ, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipStreamSynchronize(s));
    const int64_t nf = (int64_t)hc[C_FRONT], out_arcs = (int64_t)hc[C_OUT_ARCS], in_arcs = (int64_t)hc[C_IN_ARCS];
    const int64_t rows[3] = {(int64_t)hc[C_SHORT], (int64_t)hc[C_WAVE], (int64_t)hc[C_BLOCK]};
    reached += nf;
    if (nf == 0) break;
    if (hc[C_HIT] != 0) {
      found = level;
      break;
    }
    if (level == max_len) break;
    // Beamer's switch: pull when the frontier's out-arcs exceed the in-arcs of the unseen
    // vertices / alpha; push again below V / kBfsBeta vertices
    if (g->bfs_pull) pull = true;
    else if (g->bfs_alpha == 0) pull = false;
    else if (!pull) pull = out_arcs > in_arcs / (int64_t)g->bfs_alpha;
    else pull = nf >= V / kBfsBeta;
    if (pull) {
      ++n_pull;
      hipLaunchKernelGGL(k_bfs_pull_short, dim3(g_tiles), dim3(256), 0, s, io, icol, V, seen, front, next);
      if (hp[0])
        hipLaunchKernelGGL(k_bfs_pull_wave, dim3(grid_rows(hp[0], 4, 16384)), dim3(256), 0, s, plists, (int64_t)hp[0],
                           io, icol, seen, front, next);
      if (hp[1])
        hipLaunchKernelGGL(k_bfs_pull_block, dim3(grid_rows(hp[1], 1, 4096)), dim3(kBlockThreads), 0, s, plists + V,
                           (int64_t)hp[1], io, icol, seen, front, next);
    } else {
      ++n_push;
      if (rows[0] + rows[1] + rows[2] > 0)
        hipLaunchKernelGGL(k_bfs_lists, dim3(g_tiles), dim3(256), 0, s, front, oo, V, flists, cnt + C_CURSOR);
      if (rows[0])
        hipLaunchKernelGGL(k_bfs_push_short, dim3(grid_rows(rows[0], 256 / kShortLanes, 65536)), dim3(256), 0, s,
                           flists, rows[0], oo, ocol, seen, next);
      if (rows[1])
        hipLaunchKernelGGL(k_bfs_push_wave, dim3(grid_rows(rows[1], 4, 16384)), dim3(256), 0, s, flists + V, rows[1],
                           oo, ocol, seen, next);
      if (rows[2])
        hipLaunchKernelGGL(k_bfs_push_block, dim3(grid_rows(rows[2], 1, 4096)), dim3(kBlockThreads), 0, s,
                           flists + 2 * V, rows[2], oo, ocol, seen, next);
    }
    LPA_HIP(hipGetLastError());
  }
  ms[2] = bfs_ms_since(t1);
  sm.reached = reached;
  sm.push_levels = n_push;
  sm.pull_levels = n_pull;
  if (found > 0) {   // found == 0 cannot be: F and T are disjoint here
    const auto t2 = std::chrono::steady_clock::now();
    // ---- backward sweep ----
    hipLaunchKernelGGL(k_bfs_tail, dim3(grid_for(V)), dim3(256), 0, s, lev, tbits, V, (int32_t)found);
    for (int32_t l = (int32_t)found - 1; l >= 0; --l) {
      hipLaunchKernelGGL(k_bfs_back_short, dim3(g_short), dim3(256), 0, s, oo, ocol, V, l, lev);
      if (hb[0])
        hipLaunchKernelGGL(k_bfs_back_wave, dim3(grid_rows(hb[0], 4, 16384)), dim3(256), 0, s, blists, (int64_t)hb[0],
                           oo, ocol, l, lev);
      if (hb[1])
        hipLaunchKernelGGL(k_bfs_back_block, dim3(grid_rows(hb[1], 1, 4096)), dim3(kBlockThreads), 0, s, blists + V,
                           (int64_t)hb[1], oo, ocol, l, lev);
    }
    LPA_HIP(hipGetLastError());
    if (g->bfs_times) LPA_HIP(hipStreamSynchronize(s));
    ms[3] = bfs_ms_since(t2);
    const auto t3 = std::chrono::steady_clock::now();
    // ---- mark ----
    LPA_HIP(hipMemsetAsync(res, 0, sizeof(ull) * R_LEN, s));
    hipLaunchKernelGGL(k_bfs_count, dim3(grid_bh(V)), dim3(256), 0, s, lev, V, res);
    if (m > 0)
      hipLaunchKernelGGL(k_bfs_mark, dim3(grid_bh(m)), dim3(256), 0, s, g->e_src, g->e_dst, keep, m, (u32)V, lev, don,
                         res);
    LPA_HIP(hipGetLastError());
    LPA_HIP(hipMemcpyAsync(pinned, res, sizeof(ull) * R_LEN, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipMemcpyAsync(level_out, lev, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    if (m > 0) LPA_HIP(hipMemcpyAsync(on_edge_out, don, (size_t)m, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipStreamSynchronize(s));
    sm.length = found;
    sm.path_vertices = (int64_t)hc[R_VERTS];
    sm.path_edges = (int64_t)hc[R_EDGES];
    ms[4] = bfs_ms_since(t3);
  } else {
    plain_outputs();
  }
  if (summary) *summary = sm;
  return LPA_OK;
}

// LPA_BFS_TIMES=1: one line per call that searched, host clocks in ms: sets (the masks counted
// on the host), build, forward, backward, mark, and other = the rest of the call (the
// temporaries and the pinned words given back)
int bfs(lpa_graph* g, const uint8_t* from_mask, const uint8_t* to_mask, const uint8_t* edge_keep, int32_t max_len,
        int32_t* level_out, uint8_t* on_edge_out, lpa_bfs_summary* summary) {
  const auto t = std::chrono::steady_clock::now();
  double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int rc = bfs_run(g, from_mask, to_mask, edge_keep, max_len, level_out, on_edge_out, summary, ms);
  if (g->bfs_times && rc == LPA_OK && ms[2] > 0.0)
    fprintf(stderr, "lpa_bfs: sets_ms=%.3f build_ms=%.3f forward_ms=%.3f backward_ms=%.3f mark_ms=%.3f other_ms=%.3f\n",
            ms[0], ms[1], ms[2], ms[3], ms[4], bfs_ms_since(t) - ms[0] - ms[1] - ms[2] - ms[3] - ms[4]);
  return rc;
}

}  // namespace lpa
