// Landmark shortest paths of the handle's directed input graph (GraphFrame.shortestPaths,
// GraphX lib.ShortestPaths): dist[l][v] = the edges on a shortest directed path from v to
// landmark l along src -> dst, -1 where there is none.  Duplicates and self-loops change
// nothing; an edge with an end outside [0, V) is no edge.  Integers throughout.
//
// A multi-source breadth-first search from the landmarks over the REVERSED arcs, up to 64
// landmarks to a pass (Then et al., VLDB 2014): the state of a vertex is one 64-bit word,
// bit b = landmark b of the batch, a wave64 ballot's width.  A level ORs words along arcs;
// the distance is the level at which a bit first appeared.
//
//   build    the E distinct non-loop arcs (lpa_adj.hip: arcs_count, arcs_lists): the
//            out-lists oo / ocol, for the pull, and the in-lists io / icol, for the push.
//            Offsets int64, ids int32
//   batch    seen = front = next = 0, the batch's distance rows -1; next[landmark b] |= bit b
//   level    settle, read four counts on the host, stop at an empty frontier, else expand
//   settle   new = next & ~seen; seen |= new; front = new; next = 0; every set bit b of
//            new[v]: dist[b][v] = level.  A wave takes 64 consecutive vertices and, for
//            every bit of the wave's OR of new, its lanes store to 64 consecutive addresses
//            of that row under a mask (the 64 x 64 bit transpose, coalesced).  Also counts,
//            block-reduced: the frontier's vertices (and how many of each push form), its
//            in-arcs, the out-arcs of the vertices that still miss a landmark, the bits set
//   push     (small frontier) the frontier compacted into one list per row form; every
//            listed u walks its in-list: next[p] |= front[u] & ~seen[p], a relaxed
//            agent-scope 64-bit atomic OR, skipped when the word is 0
//   pull     (large frontier) every v that misses a landmark ORs front[u] over its
//            out-list, stops once the word covers all it misses, and stores
//            next[v] = acc & ~seen[v]: no atomics
//
// Row forms, by list length L (kSpShort / kSpWave; in-lists for the push, out-lists for
// the pull):
//   short   L <= kSpShort   8 lanes per row (the pull: every row in id order, longer rows
//           skipped; the push: the listed rows)
//   wave    L <= kSpWave    a wave per listed row
//   block   above           a block of 1024 per listed row (a hub of 10^5 arcs: 16 waves)
// The pull's lists are static (by out-degree, built once a call); the push's are the
// frontier's, rebuilt on every push level.
//
// Invariants.  seen, front and the offsets are written by settle and the build only, never
// by an expansion, so an expansion reads them as of the kernel boundary before it.  next is
// 0 outside an expansion and its settle.  front is a subset of seen and of the batch's bits;
// bit b of seen[v] is set exactly when dist[b][v] >= 0.
//
// Why the interleaving does not matter.  After level k, next & ~seen at v is the OR of
// front[u] & ~seen[v] over the arcs v -> u, whatever computed it: OR is commutative,
// associative and idempotent, so the order of the atomics, the order of a compacted list
// (its positions come from an atomic cursor) and the push / pull choice all give the same
// word; a pull that stops early has by then covered every bit v misses, and bits v has
// already are masked off.  By induction over the levels seen, front and dist are functions
// of (V, arc set, landmarks) alone.  Only push_levels / pull_levels tell the schedule; their
// sum is, over the batches, the batch's largest distance + 1.
#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

namespace {

constexpr int kSpBeta = 24;         // back to the push when the frontier falls below V / kSpBeta

// slots of the per-level counters
enum { C_FRONT = 0, C_SHORT = 1, C_WAVE = 2, C_BLOCK = 3, C_IN_ARCS = 4, C_OUT_ARCS = 5, C_BITS = 6, C_READ = 7,
       C_CURSOR = 7, C_LEN = 10 };

__device__ __forceinline__ ull sp_wave_or(ull x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x |= __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ ull sp_wave_add(ull x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ void sp_or(ull* p, ull w) {
  __hip_atomic_fetch_or(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- a batch ----
// lm: the batch's nb landmarks (each in [0, V), checked by the caller)
__global__ __launch_bounds__(64) void k_sp_seed(const int32_t* __restrict__ lm, int nb, ull* __restrict__ next) {
  const int b = threadIdx.x;
  if (b < nb) sp_or(next + lm[b], 1ull << b);
}

// One level's settle over every vertex, a wave per 64 consecutive ones (V need not be a
// multiple of 64: the lanes past V hold new = 0).  dist: the batch's first row.
__global__ __launch_bounds__(256) void k_sp_settle(ull* __restrict__ seen, ull* __restrict__ front,
                                                   ull* __restrict__ next, const int64_t* __restrict__ oo,
                                                   const int64_t* __restrict__ io, int64_t V, ull active, int32_t level,
                                                   int32_t* __restrict__ dist, ull* __restrict__ cnt) {
  __shared__ ull ws[4][C_READ];
  ull c[C_READ] = {0, 0, 0, 0, 0, 0, 0};
  const int lane = threadIdx.x & 63;
  const int64_t tiles = (V + 63) >> 6;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const int64_t v = t * 64 + lane;
    ull nw = 0;
    if (v < V) {
      const ull sn = seen[v], nx = next[v];
      nw = nx & ~sn;
      const ull s2 = sn | nw;
      if (nw) seen[v] = s2;
      front[v] = nw;
      if (nx) next[v] = 0;
      if (nw) {
        const int64_t L = io[v + 1] - io[v];
        c[C_FRONT] += 1;
        c[C_SHORT] += L > 0 && L <= kSpShort ? 1 : 0;
        c[C_WAVE] += L > kSpShort && L <= kSpWave ? 1 : 0;
        c[C_BLOCK] += L > kSpWave ? 1 : 0;
        c[C_IN_ARCS] += (ull)L;
        c[C_BITS] += (ull)__popcll(nw);
      }
      if (~s2 & active) c[C_OUT_ARCS] += (ull)(oo[v + 1] - oo[v]);
    }
    // the rows that gained a vertex in this tile, one after another (the same in every lane)
    ull rows = sp_wave_or(nw);
    while (rows) {
      const int b = __ffsll(rows) - 1;
      rows &= rows - 1;
      if ((nw >> b) & 1) dist[(int64_t)b * V + v] = level;
    }
  }
#pragma unroll
  for (int k = 0; k < C_READ; ++k) {
    const ull x = sp_wave_add(c[k]);
    if (lane == 0) ws[threadIdx.x >> 6][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < C_READ) {
    const ull x = ws[0][threadIdx.x] + ws[1][threadIdx.x] + ws[2][threadIdx.x] + ws[3][threadIdx.x];
    if (x) atomicAdd(&cnt[threadIdx.x], x);
  }
}

// the frontier compacted by push form: short rows in lists, wave rows in lists + V, block
// rows in lists + 2 V (a row without in-arcs is in none); one cursor add per wave and form
__global__ __launch_bounds__(256) void k_sp_lists(const ull* __restrict__ front, const int64_t* __restrict__ io,
                                                  int64_t V, int32_t* __restrict__ lists, ull* __restrict__ cursor) {
  const int lane = threadIdx.x & 63;
  const ull below = (1ull << lane) - 1;
  const int64_t tiles = (V + 63) >> 6;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const int64_t v = t * 64 + lane;
    int form = -1;
    if (v < V && front[v] != 0) {
      const int64_t L = io[v + 1] - io[v];
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

// ---- push: listed frontier rows walk their in-lists ----
__global__ __launch_bounds__(256) void k_sp_push_short(const int32_t* __restrict__ rows, int64_t nrows,
                                                       const int64_t* __restrict__ io, const int32_t* __restrict__ icol,
                                                       const ull* __restrict__ front, const ull* __restrict__ seen,
                                                       ull* __restrict__ next) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t k = (int64_t)blockIdx.x * kRows + threadIdx.x / G; k < nrows; k += (int64_t)gridDim.x * kRows) {
    const int64_t u = rows[k];
    const ull f = front[u];
    const int64_t b = io[u], L = io[u + 1] - b;
    for (int64_t i = sub; i < L; i += G) {
      const int32_t p = icol[b + i];
      const ull w = f & ~seen[p];
      if (w) sp_or(next + p, w);
    }
  }
}

__global__ __launch_bounds__(256) void k_sp_push_wave(const int32_t* __restrict__ rows, int64_t nrows,
                                                      const int64_t* __restrict__ io, const int32_t* __restrict__ icol,
                                                      const ull* __restrict__ front, const ull* __restrict__ seen,
                                                      ull* __restrict__ next) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t u = rows[k];
    const ull f = front[u];
    const int64_t b = io[u], L = io[u + 1] - b;
    for (int64_t i = lane; i < L; i += 64) {
      const int32_t p = icol[b + i];
      const ull w = f & ~seen[p];
      if (w) sp_or(next + p, w);
    }
  }
}

__global__ __launch_bounds__(kBlockThreads) void k_sp_push_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                 const int64_t* __restrict__ io,
                                                                 const int32_t* __restrict__ icol,
                                                                 const ull* __restrict__ front,
                                                                 const ull* __restrict__ seen, ull* __restrict__ next) {
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t u = rows[k];
    const ull f = front[u];
    const int64_t b = io[u], L = io[u + 1] - b;
    for (int64_t i = threadIdx.x; i < L; i += kBlockThreads) {
      const int32_t p = icol[b + i];
      const ull w = f & ~seen[p];
      if (w) sp_or(next + p, w);
    }
  }
}

// ---- pull: rows that miss a landmark scan their out-lists ----
// every row in id order, kShortLanes lanes each; a longer row is not this form's.  A lane
// stops when its own word covers what the row misses
__global__ __launch_bounds__(256) void k_sp_pull_short(const int64_t* __restrict__ oo, const int32_t* __restrict__ ocol,
                                                       int64_t V, ull active, const ull* __restrict__ seen,
                                                       const ull* __restrict__ front, ull* __restrict__ next) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < V; base += (int64_t)gridDim.x * kRows) {
    const int64_t v = base + threadIdx.x / G;
    bool mine = false;
    ull acc = 0, miss = 0;
    if (v < V) {
      miss = ~seen[v] & active;
      const int64_t b = oo[v], L = oo[v + 1] - b;
      mine = miss != 0 && L > 0 && L <= kSpShort;
      if (mine)
        for (int64_t i = sub; i < L; i += G) {
          acc |= front[ocol[b + i]];
          if ((acc & miss) == miss) break;
        }
    }
    // the G lanes of a row are neighbours: every one of them ends with the row's word
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) acc |= __shfl_xor(acc, off, 64);
    if (mine && sub == 0) next[v] = acc & miss;
  }
}

// this wave's share of a row of L entries at col + b, 256 entries a step from `first`,
// `stride` entries on; stops after the step at which the wave's word covers `miss`
__device__ __forceinline__ ull sp_scan(const int32_t* __restrict__ col, const ull* __restrict__ front, int64_t b,
                                       int64_t L, int64_t first, int64_t stride, ull miss, int lane) {
  ull acc = 0;
  for (int64_t i0 = first; i0 < L; i0 += stride) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = i0 + j * 64 + lane;
      if (i < L) acc |= front[col[b + i]];
    }
    acc = sp_wave_or(acc);
    if ((acc & miss) == miss) break;   // the same in every lane
  }
  return acc;
}

// a wave per listed row
__global__ __launch_bounds__(256) void k_sp_pull_wave(const int32_t* __restrict__ rows, int64_t nrows,
                                                      const int64_t* __restrict__ oo, const int32_t* __restrict__ ocol,
                                                      ull active, const ull* __restrict__ seen,
                                                      const ull* __restrict__ front, ull* __restrict__ next) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t v = rows[k];
    const ull miss = ~seen[v] & active;
    if (miss == 0) continue;
    const int64_t b = oo[v];
    const ull acc = sp_scan(ocol, front, b, oo[v + 1] - b, 0, 256, miss, lane);
    if (lane == 0) next[v] = acc & miss;
  }
}

// a block per listed row (k and miss are the same in every thread: barriers inside); every
// wave stops on its own
__global__ __launch_bounds__(kBlockThreads) void k_sp_pull_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                 const int64_t* __restrict__ oo,
                                                                 const int32_t* __restrict__ ocol, ull active,
                                                                 const ull* __restrict__ seen,
                                                                 const ull* __restrict__ front, ull* __restrict__ next) {
  constexpr int kWaves = kBlockThreads / 64;
  __shared__ ull ws[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t v = rows[k];
    const ull miss = ~seen[v] & active;
    if (miss == 0) continue;
    const int64_t b = oo[v];
    const ull acc = sp_scan(ocol, front, b, oo[v + 1] - b, (int64_t)wave * 256, (int64_t)kWaves * 256, miss, lane);
    if (lane == 0) ws[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      ull t = 0;
      for (int i = 0; i < kWaves; ++i) t |= ws[i];
      next[v] = t & miss;
    }
    __syncthreads();   // before the next row rewrites ws
  }
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream and sp_alpha / sp_pull of the handle, nothing of the
// LPA state; every array is a stream-ordered temporary.  The landmarks are in [0, V).
int shortest_paths(lpa_graph* g, const int32_t* landmarks, int32_t n_landmarks, int32_t* dist_out,
                   int32_t out_is_device, lpa_sp_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V;
  const int64_t batches = ((int64_t)n_landmarks + 63) / 64;
  if (summary) *summary = lpa_sp_summary{0, 0, -1, batches, 0, 0};
  if (V == 0 || (n_landmarks == 0 && !summary)) return LPA_OK;
  Tmp tmp(s);
  // ---- build ----
  ArcLists arcs;
  LPA_TRY(arcs_count(g, tmp, nullptr, &arcs));
  if (summary) summary->arcs = arcs.E;
  if (n_landmarks == 0) return LPA_OK;
  LPA_TRY(arcs_lists(g, tmp, &arcs));
  const int64_t *oo = arcs.oo, *io = arcs.io;
  const int32_t *ocol = arcs.ocol, *icol = arcs.icol;
  // the pull's static lists, by out-degree
  int32_t* plists = nullptr;
  u32 hp[2] = {0, 0};   // the pull's wave rows and block rows (read after the synchronisation below)
  LPA_TRY(form_lists(tmp, oo, V, kSpShort, kSpWave, &plists, hp));
  // ---- state ----
  ull *seen = nullptr, *front = nullptr, *next = nullptr, *cnt = nullptr;
  int32_t *flists = nullptr, *lm = nullptr, *dbuf = nullptr;
  LPA_TRY(tmp.get(&seen, V));
  LPA_TRY(tmp.get(&front, V));
  LPA_TRY(tmp.get(&next, V));
  LPA_TRY(tmp.get(&cnt, C_LEN));
  LPA_TRY(tmp.get(&flists, 3 * V));
  LPA_TRY(tmp.get(&lm, n_landmarks));
  if (!out_is_device) LPA_TRY(tmp.get(&dbuf, (n_landmarks < 64 ? (int64_t)n_landmarks : 64) * V));
  ull* pinned = nullptr;
  LPA_TRY(tmp.pin(&pinned, C_READ));
  LPA_HIP(hipMemcpyAsync(lm, landmarks, sizeof(int32_t) * (size_t)n_landmarks, hipMemcpyHostToDevice, s));
  LPA_HIP(hipStreamSynchronize(s));
  const volatile ull* hc = pinned;
  const int64_t tiles = (V + 63) >> 6;
  const unsigned g_tiles = grid_rows(tiles, 4, 8192);
  const unsigned g_short = grid_rows(V, 256 / kShortLanes, 65536);
  int64_t reached = 0, max_d = -1, n_push = 0, n_pull = 0;
  for (int64_t bt = 0; bt < batches; ++bt) {
    const int nb = (int)((int64_t)n_landmarks - 64 * bt < 64 ? (int64_t)n_landmarks - 64 * bt : 64);
    const ull active = nb == 64 ? ~0ull : (1ull << nb) - 1;
    int32_t* dist = out_is_device ? dist_out + 64 * bt * V : dbuf;
    LPA_HIP(hipMemsetAsync(dist, 0xFF, sizeof(int32_t) * (size_t)nb * (size_t)V, s));
    LPA_HIP(hipMemsetAsync(seen, 0, sizeof(ull) * (size_t)V, s));
    LPA_HIP(hipMemsetAsync(next, 0, sizeof(ull) * (size_t)V, s));
    hipLaunchKernelGGL(k_sp_seed, dim3(1), dim3(64), 0, s, lm + 64 * bt, nb, next);
    LPA_HIP(hipGetLastError());
    bool pull = g->sp_pull != 0;
    for (int32_t level = 0;; ++level) {
      LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(ull) * C_LEN, s));
      hipLaunchKernelGGL(k_sp_settle, dim3(g_tiles), dim3(256), 0, s, seen, front, next, oo, io, V, active, level, dist,
                         cnt);
      LPA_HIP(hipGetLastError());
      LPA_HIP(hipMemcpyAsync(pinned, cnt, sizeof(ull) * C_READ, hipMemcpyDeviceToHost, s));
      LPA_HIP(hipStreamSynchronize(s));
      const int64_t nf = (int64_t)hc[C_FRONT], in_arcs = (int64_t)hc[C_IN_ARCS], out_arcs = (int64_t)hc[C_OUT_ARCS];
      const int64_t rows[3] = {(int64_t)hc[C_SHORT], (int64_t)hc[C_WAVE], (int64_t)hc[C_BLOCK]};
      reached += (int64_t)hc[C_BITS];
      if (nf == 0) break;
      max_d = level > max_d ? level : max_d;
      // Beamer's switch: pull when the frontier's in-arcs exceed the out-arcs of the
      // vertices that still miss a landmark / alpha; push again below V / kSpBeta vertices
      if (g->sp_pull) pull = true;
      else if (g->sp_alpha == 0) pull = false;
      else if (!pull) pull = in_arcs > out_arcs / (int64_t)g->sp_alpha;
      else pull = nf >= V / kSpBeta;
      if (pull) {
        ++n_pull;
        hipLaunchKernelGGL(k_sp_pull_short, dim3(g_short), dim3(256), 0, s, oo, ocol, V, active, seen, front, next);
        if (hp[0])
          hipLaunchKernelGGL(k_sp_pull_wave, dim3(grid_rows(hp[0], 4, 16384)), dim3(256), 0, s, plists, (int64_t)hp[0],
                             oo, ocol, active, seen, front, next);
        if (hp[1])
          hipLaunchKernelGGL(k_sp_pull_block, dim3(grid_rows(hp[1], 1, 4096)), dim3(kBlockThreads), 0, s, plists + V,
                             (int64_t)hp[1], oo, ocol, active, seen, front, next);
      } else {
        ++n_push;
        if (rows[0] + rows[1] + rows[2] > 0)
          hipLaunchKernelGGL(k_sp_lists, dim3(g_tiles), dim3(256), 0, s, front, io, V, flists, cnt + C_CURSOR);
        if (rows[0])
          hipLaunchKernelGGL(k_sp_push_short, dim3(grid_rows(rows[0], 256 / kShortLanes, 65536)), dim3(256), 0, s,
                             flists, rows[0], io, icol, front, seen, next);
        if (rows[1])
          hipLaunchKernelGGL(k_sp_push_wave, dim3(grid_rows(rows[1], 4, 16384)), dim3(256), 0, s, flists + V, rows[1],
                             io, icol, front, seen, next);
        if (rows[2])
          hipLaunchKernelGGL(k_sp_push_block, dim3(grid_rows(rows[2], 1, 4096)), dim3(kBlockThreads), 0, s,
                             flists + 2 * V, rows[2], io, icol, front, seen, next);
      }
      LPA_HIP(hipGetLastError());
    }
    if (!out_is_device)
      LPA_HIP(hipMemcpyAsync(dist_out + 64 * bt * V, dbuf, sizeof(int32_t) * (size_t)nb * (size_t)V,
                             hipMemcpyDeviceToHost, s));
  }
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->reached = reached;
    summary->max_distance = max_d;
    summary->push_levels = n_push;
    summary->pull_levels = n_pull;
  }
  return LPA_OK;
}

}  // namespace lpa
