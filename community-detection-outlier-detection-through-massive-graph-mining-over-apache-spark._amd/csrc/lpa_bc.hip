// Betweenness centrality (GraphFrame.betweennessCentrality): Brandes' algorithm over the
// distinct non-loop arcs of the input graph (directed) or over both orientations of them
// (undirected), from a set of sources, B sources to a pass in lockstep by level.
//
//   raw[v]     = sum over the sources s != v of delta_s(v)
//   delta_s(v) = sum over the arcs v -> w with level_s(w) == level_s(v) + 1
//                of sigma_s(v) / sigma_s(w) * (1 + delta_s(w))
// level_s the breadth-first distance from s, sigma_s the number of shortest s-paths
// (binary64, as networkx: above 2^53 the counts are rounded).  The caller scales raw.
//
//   build    the E arcs (lpa_adj.hip: arcs_count, arcs_lists): out-lists oo / ocol and in-lists
//            io / icol; undirected: both orientations of every edge go through the same sort,
//            the two lists coincide and the in-lists are dropped
//   layout   level (int32), sigma and delta (binary64) interleaved per vertex, x[v * B + slot]:
//            one gathered arc serves the B sources of the pass from one contiguous piece
//            (B = 16: a 128-byte line of doubles).  seen[v] / next[v]: one mask word per vertex,
//            bit b = slot b.  The pass's level-ordered list: entries (mask << 32 | vertex), a
//            vertex once for every level at which some slot settles it; per level three
//            contiguous runs, by the row form of the vertex's OUT-list
//   forward  level d: settle (a sweep of the mask words: seen |= next, the counts of the new
//            vertices by out-form and by in-form, the bits set), the host reads the counts and
//            stops at none; fill (a second sweep of the mask words: the new vertices appended to
//            the level's runs and to this level's in-form lists, next = 0); sigma (d > 0): the
//            new vertices pull over their IN-lists, sigma[w][b] = sum of sigma[u][b] over the
//            in-arcs with level[u][b] == d - 1, and write level = d, delta = 0; push: the level's
//            entries walk their out-lists, next[w] |= mask & ~seen[w], an integer atomic OR
//   backward d = depth - 1 ... 0: the level's entries pull over their OUT-lists with the
//            recurrence above, for the slots of the entry's mask.  Work: the level's own
//            entries and their arcs
//   finish   raw[v] = raw[v] + delta[v][b] for the pass's slots in source order, b's own source
//            and the vertices it did not reach skipped
//
// Row forms, by list length L (kBcShort / kBcWave), P lanes ("phases") per slot:
//   short   L <= kBcShort   P = 1: B lanes per row
//   wave    L <= kBcWave    P = 4: 4 B lanes per row
//   block   above           P = 64: a block of 64 B threads per row
// P does not depend on B: that is what makes a sum's shape the same at every batch width.
//
// No floating-point atomics.  A slot's sum over a row: phase p adds the entries p, p + P, ... in
// four interleaved accumulators, (a0 + a1) + (a2 + a3); the wave form adds its four phases as
// (p0 + p2) + (p1 + p3) (two xor-shuffles: both sides form the same commutative sum); the block
// form adds, in order, the sixteen such sums of its phases four by four, from LDS.  An arc that
// does not belong to the sum adds 0.0, which changes no bit of a non-negative sum.  The shape
// depends on L and the form alone, not on the slot, on B or on the pass's other sources; the
// position of a vertex in a level's list (an atomic cursor's) moves no operand.  So raw is a
// function of (V, arc set, sources in order, form boundaries): bit-identical across runs,
// handles, input edge orders and batch widths.
//
// sigma_v / sigma_w * (1 + delta_w) is written as the definition writes it: no contraction.
#include <vector>

#include "lpa_device.h"
#include "lpa_algo.h"

#pragma clang fp contract(off)

namespace lpa {

namespace {

// slots of the per-level counters
enum { C_OUT = 0, C_IN = 3, C_BITS = 6, C_READ = 7, C_CUR_OUT = 8, C_CUR_IN = 11, C_LEN = 14 };

constexpr int kWavePhases = 4, kBlockPhases = 64;

__device__ __forceinline__ int bc_form(int64_t L) { return L <= kBcShort ? 0 : L <= kBcWave ? 1 : 2; }

__device__ __forceinline__ ull bc_wave_add(ull x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

struct Pass {   // the interleaved state and what a row is asked for
  int32_t* level;
  double* sigma;
  double* delta;
  int32_t want;   // the level of the arcs' other ends that belong to the sum (d - 1 forward, d + 1 backward)
  int32_t d;      // forward: the level the rows settle at
};

// ---- a pass's start ----
// src: the pass's nb sources (distinct, in [0, V))
template <int B>
__global__ __launch_bounds__(64) void k_bc_seed(const int32_t* __restrict__ src, int nb, Pass ps,
                                                u32* __restrict__ next) {
  const int b = threadIdx.x;
  if (b < nb) {
    const int64_t i = (int64_t)src[b] * B + b;
    ps.level[i] = 0;
    ps.sigma[i] = 1.0;
    ps.delta[i] = 0.0;
    __hip_atomic_fetch_or(next + src[b], 1u << b, LPA_RLX_AGENT);
  }
}

// ---- a level's settle and fill: sweeps of the mask words ----
__global__ __launch_bounds__(256) void k_bc_settle(u32* __restrict__ seen, const u32* __restrict__ next,
                                                   const int64_t* __restrict__ oo, const int64_t* __restrict__ io,
                                                   int64_t V, ull* __restrict__ cnt) {
  __shared__ ull ws[4][C_READ];
  ull c[C_READ] = {0, 0, 0, 0, 0, 0, 0};
  GRID_STRIDE(v, V) {
    const u32 nx = next[v];
    if (nx) {
      seen[v] |= nx;
      c[C_OUT + bc_form(oo[v + 1] - oo[v])] += 1;
      c[C_IN + bc_form(io[v + 1] - io[v])] += 1;
      c[C_BITS] += (ull)__popc(nx);
    }
  }
#pragma unroll
  for (int k = 0; k < C_READ; ++k) {
    const ull x = bc_wave_add(c[k]);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < C_READ) {
    const ull x = ws[0][threadIdx.x] + ws[1][threadIdx.x] + ws[2][threadIdx.x] + ws[3][threadIdx.x];
    if (x) atomicAdd(&cnt[threadIdx.x], x);
  }
}

// the new vertices (next != 0) as entries: at olist + obase[form of the out-list] and at
// ilist + ibase[form of the in-list], positions from one cursor add per wave and form
struct Bases {
  int64_t o[3], i[3];
};
__global__ __launch_bounds__(256) void k_bc_fill(u32* __restrict__ next, const int64_t* __restrict__ oo,
                                                 const int64_t* __restrict__ io, int64_t V, Bases bs,
                                                 u64* __restrict__ olist, u64* __restrict__ ilist,
                                                 ull* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const ull below = (1ull << lane) - 1;
  BLOCK_STRIDE(base, V) {
    const int64_t v = base + threadIdx.x;
    int fo = -1, fi = -1;
    u64 e = 0;
    if (v < V) {
      const u32 nx = next[v];
      if (nx) {
        next[v] = 0;
        fo = bc_form(oo[v + 1] - oo[v]);
        fi = bc_form(io[v + 1] - io[v]);
        e = ((u64)nx << 32) | (u64)(u32)v;
      }
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const ull mo = __ballot(fo == f);
      if (mo) {
        ull p = 0;
        if (lane == 0) p = atomicAdd(&cnt[C_CUR_OUT + f], (ull)__popcll(mo));
        p = __shfl(p, 0, 64);
        if (fo == f) olist[bs.o[f] + (int64_t)p + __popcll(mo & below)] = e;
      }
      const ull mi = __ballot(fi == f);
      if (mi) {
        ull p = 0;
        if (lane == 0) p = atomicAdd(&cnt[C_CUR_IN + f], (ull)__popcll(mi));
        p = __shfl(p, 0, 64);
        if (fi == f) ilist[bs.i[f] + (int64_t)p + __popcll(mi & below)] = e;
      }
    }
  }
}

// ---- push: the level's entries walk their out-lists (integers only) ----
template <int G>   // lanes per row
__global__ __launch_bounds__(G < 256 ? 256 : G) void k_bc_push(const u64* __restrict__ ent, int64_t nrows,
                                                               const int64_t* __restrict__ oo,
                                                               const int32_t* __restrict__ ocol,
                                                               const u32* __restrict__ seen, u32* __restrict__ next) {
  constexpr int kThreads = G < 256 ? 256 : G, kRows = kThreads / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t k = (int64_t)blockIdx.x * kRows + threadIdx.x / G; k < nrows; k += (int64_t)gridDim.x * kRows) {
    const u64 e = ent[k];
    const int64_t u = (int64_t)(u32)e;
    const u32 f = (u32)(e >> 32);
    const int64_t b = oo[u], L = oo[u + 1] - b;
    for (int64_t i = sub; i < L; i += G) {
      const int32_t p = ocol[b + i];
      const u32 w = f & ~seen[p];
      if (w) __hip_atomic_fetch_or(next + p, w, LPA_RLX_AGENT);
    }
  }
}

// ---- the two pulls ----
// what the arc to x adds to slot b's sum of a row whose own sigma is sv
template <int B, bool kBack>
__device__ __forceinline__ double bc_term(const Pass& ps, int64_t x, int b, double sv) {
  const int64_t i = x * B + b;
  if (ps.level[i] != ps.want) return 0.0;
  if (kBack) return sv / ps.sigma[i] * (1.0 + ps.delta[i]);
  return ps.sigma[i];
}

// phase `first` of `stride` phases: the entries first, first + stride, ... of a row of L at
// col + b0, in four interleaved accumulators
template <int B, bool kBack>
__device__ __forceinline__ double bc_strided(const Pass& ps, const int32_t* __restrict__ col, int64_t b0, int64_t L,
                                             int first, int stride, int b, double sv) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t i = first;
  for (; i + 3 * (int64_t)stride < L; i += 4 * (int64_t)stride) {
    const int32_t u0 = col[b0 + i], u1 = col[b0 + i + stride], u2 = col[b0 + i + 2 * (int64_t)stride],
                  u3 = col[b0 + i + 3 * (int64_t)stride];
    a0 += bc_term<B, kBack>(ps, u0, b, sv);
    a1 += bc_term<B, kBack>(ps, u1, b, sv);
    a2 += bc_term<B, kBack>(ps, u2, b, sv);
    a3 += bc_term<B, kBack>(ps, u3, b, sv);
  }
  for (; i < L; i += stride) a0 += bc_term<B, kBack>(ps, col[b0 + i], b, sv);
  return (a0 + a1) + (a2 + a3);
}

// slot b of row v from its sum
template <int B, bool kBack>
__device__ __forceinline__ void bc_store(const Pass& ps, int64_t v, int b, double s) {
  const int64_t i = v * B + b;
  if (kBack) {
    ps.delta[i] = s;
  } else {
    ps.level[i] = ps.d;
    ps.sigma[i] = s;
    ps.delta[i] = 0.0;
  }
}

// P phases per slot, P B <= 64 lanes per row, 256 / (P B) rows to a block.  Every thread runs
// every trip (the shuffles); a row's lanes are neighbours inside one wave
template <int B, int P, bool kBack>
__global__ __launch_bounds__(256) void k_bc_rows(const u64* __restrict__ ent, int64_t nrows,
                                                 const int64_t* __restrict__ off, const int32_t* __restrict__ col,
                                                 Pass ps) {
  constexpr int T = P * B, kRows = 256 / T;
  static_assert(T <= 64, "a row's lanes share a wave");
  const int sub = threadIdx.x % T, b = sub % B, ph = sub / B;
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < nrows; base += (int64_t)gridDim.x * kRows) {
    const int64_t k = base + threadIdx.x / T;
    bool mine = false;
    int64_t v = 0;
    double acc = 0.0;
    if (k < nrows) {
      const u64 e = ent[k];
      v = (int64_t)(u32)e;
      mine = ((u32)(e >> 32) >> b) & 1u;
      if (mine) {
        const int64_t b0 = off[v];
        const double sv = kBack ? ps.sigma[v * B + b] : 0.0;
        acc = bc_strided<B, kBack>(ps, col, b0, off[v + 1] - b0, ph, P, b, sv);
      }
    }
#pragma unroll
    for (int o = T / 2; o >= B; o >>= 1) acc += __shfl_xor(acc, o, 64);   // P = 4: (p0 + p2) + (p1 + p3)
    if (mine && ph == 0) bc_store<B, kBack>(ps, v, b, acc);
  }
}

// a block of 64 B threads per row (k is the same in every thread: barriers inside)
template <int B, bool kBack>
__global__ __launch_bounds__(kBlockPhases * B) void k_bc_block(const u64* __restrict__ ent, int64_t nrows,
                                                               const int64_t* __restrict__ off,
                                                               const int32_t* __restrict__ col, Pass ps) {
  constexpr int P = kBlockPhases;
  __shared__ double ws[P][B];
  const int b = threadIdx.x % B, ph = threadIdx.x / B;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const u64 e = ent[k];
    const int64_t v = (int64_t)(u32)e;
    const bool mine = ((u32)(e >> 32) >> b) & 1u;
    double acc = 0.0;
    if (mine) {
      const int64_t b0 = off[v];
      const double sv = kBack ? ps.sigma[v * B + b] : 0.0;
      acc = bc_strided<B, kBack>(ps, col, b0, off[v + 1] - b0, ph, P, b, sv);
    }
    ws[ph][b] = acc;
    __syncthreads();
    if (mine && ph == 0) {
      double t = 0.0;
      for (int q = 0; q < P; q += 4) t += (ws[q][b] + ws[q + 2][b]) + (ws[q + 1][b] + ws[q + 3][b]);
      bc_store<B, kBack>(ps, v, b, t);
    }
    __syncthreads();   // before the next row rewrites ws
  }
}

// ---- a pass's finish ----
template <int B>
__global__ __launch_bounds__(256) void k_bc_accumulate(const int32_t* __restrict__ src, int nb, Pass ps, int64_t V,
                                                       double* __restrict__ raw) {
  GRID_STRIDE(v, V) {
    double r = raw[v];
    for (int b = 0; b < nb; ++b)
      if (v != (int64_t)src[b] && ps.level[v * B + b] >= 0) r = r + ps.delta[v * B + b];
    raw[v] = r;
  }
}

// the three forms of one pull over the runs ent + base[f] of n[f] entries
template <int B, bool kBack>
int bc_pull(hipStream_t s, const u64* ent, const int64_t* base, const int64_t* n, const int64_t* off,
            const int32_t* col, const Pass& ps) {
  if (n[0])
    hipLaunchKernelGGL((k_bc_rows<B, 1, kBack>), dim3(grid_rows(n[0], 256 / B, 65536)), dim3(256), 0, s, ent + base[0],
                       n[0], off, col, ps);
  if (n[1])
    hipLaunchKernelGGL((k_bc_rows<B, kWavePhases, kBack>), dim3(grid_rows(n[1], 256 / (kWavePhases * B), 65536)),
                       dim3(256), 0, s, ent + base[1], n[1], off, col, ps);
  if (n[2])
    hipLaunchKernelGGL((k_bc_block<B, kBack>), dim3(grid_rows(n[2], 1, 4096)), dim3(kBlockPhases * B), 0, s,
                       ent + base[2], n[2], off, col, ps);
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

struct Lists {
  int64_t V = 0;
  const int64_t *oo = nullptr, *io = nullptr;
  const int32_t *ocol = nullptr, *icol = nullptr;
};
struct Totals {
  int64_t reached = 0, max_depth = -1, levels = 0;
};

struct LevelRuns {
  int64_t base[3], n[3];
};

// Every pass at width B; src: the sources on the device.  LPA_ENOMEM before any work when the
// width's state cannot be allocated (the caller then tries a narrower one)
template <int B>
int bc_passes(lpa_graph* g, const Lists& ls, const int32_t* src, int32_t n_sources, double* raw, Totals* tot) {
  hipStream_t s = g->stream;
  const int64_t V = ls.V;
  Tmp tmp(s);
  Pass ps{nullptr, nullptr, nullptr, 0, 0};
  u32 *seen = nullptr, *next = nullptr;
  u64 *olist = nullptr, *ilist = nullptr;
  ull* cnt = nullptr;
  LPA_TRY(tmp.get(&ps.level, V * B));
  LPA_TRY(tmp.get(&ps.sigma, V * B));
  LPA_TRY(tmp.get(&ps.delta, V * B));
  LPA_TRY(tmp.get(&olist, V * B));   // a (vertex, slot) pair settles once: at most V B entries a pass
  LPA_TRY(tmp.get(&ilist, V));       // a level's new vertices
  LPA_TRY(tmp.get(&seen, V));
  LPA_TRY(tmp.get(&next, V));
  LPA_TRY(tmp.get(&cnt, C_LEN));
  ull* pinned = nullptr;
  LPA_TRY(tmp.pin(&pinned, C_READ));
  const volatile ull* hc = pinned;
  const unsigned g_sweep = grid_bh(V);
  std::vector<LevelRuns> runs;
  LPA_HIP(hipMemsetAsync(next, 0, sizeof(u32) * (size_t)V, s));
  for (int32_t first = 0; first < n_sources; first += B) {
    const int nb = n_sources - first < B ? n_sources - first : B;
    LPA_HIP(hipMemsetAsync(ps.level, 0xFF, sizeof(int32_t) * (size_t)(V * B), s));
    LPA_HIP(hipMemsetAsync(seen, 0, sizeof(u32) * (size_t)V, s));
    hipLaunchKernelGGL(k_bc_seed<B>, dim3(1), dim3(64), 0, s, src + first, nb, ps, next);
    LPA_HIP(hipGetLastError());
    runs.clear();
    int64_t filled = 0;   // entries of the pass so far
    // ---- forward ----
    for (int32_t d = 0;; ++d) {
      LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(ull) * C_LEN, s));
      hipLaunchKernelGGL(k_bc_settle, dim3(g_sweep), dim3(256), 0, s, seen, next, ls.oo, ls.io, V, cnt);
      LPA_HIP(hipGetLastError());
      LPA_HIP(hipMemcpyAsync(pinned, cnt, sizeof(ull) * C_READ, hipMemcpyDeviceToHost, s));
      LPA_HIP(hipStreamSynchronize(s));
      LevelRuns r;
      int64_t ni[3], ibase[3], nf = 0, at = 0;
      for (int f = 0; f < 3; ++f) {
        r.n[f] = (int64_t)hc[C_OUT + f];
        r.base[f] = filled + nf;
        nf += r.n[f];
        ni[f] = (int64_t)hc[C_IN + f];
        ibase[f] = at;
        at += ni[f];
      }
      if (nf == 0) break;   // no slot discovered a vertex (next is all zero again)
      tot->reached += (int64_t)hc[C_BITS];
      if (filled + nf > V * B || at > V) {
        set_error("lpa_betweenness: a level's %lld new vertices overrun the pass's list", (long long)nf);
        return LPA_EOVERFLOW;
      }
      const Bases bs{{r.base[0], r.base[1], r.base[2]}, {ibase[0], ibase[1], ibase[2]}};
      hipLaunchKernelGGL(k_bc_fill, dim3(g_sweep), dim3(256), 0, s, next, ls.oo, ls.io, V, bs, olist, ilist, cnt);
      LPA_HIP(hipGetLastError());
      runs.push_back(r);
      filled += nf;
      if (d > 0) {
        ps.want = d - 1;
        ps.d = d;
        LPA_TRY((bc_pull<B, false>(s, ilist, ibase, ni, ls.io, ls.icol, ps)));
      }
      if (r.n[0])
        hipLaunchKernelGGL(k_bc_push<kShortLanes>, dim3(grid_rows(r.n[0], 256 / kShortLanes, 65536)), dim3(256), 0, s,
                           olist + r.base[0], r.n[0], ls.oo, ls.ocol, seen, next);
      if (r.n[1])
        hipLaunchKernelGGL(k_bc_push<64>, dim3(grid_rows(r.n[1], 4, 16384)), dim3(256), 0, s, olist + r.base[1],
                           r.n[1], ls.oo, ls.ocol, seen, next);
      if (r.n[2])
        hipLaunchKernelGGL(k_bc_push<kBlockThreads>, dim3(grid_rows(r.n[2], 1, 4096)), dim3(kBlockThreads), 0, s,
                           olist + r.base[2], r.n[2], ls.oo, ls.ocol, seen, next);
      LPA_HIP(hipGetLastError());
    }
    const int64_t depth = (int64_t)runs.size() - 1;
    tot->levels += depth + 1;
    tot->max_depth = depth > tot->max_depth ? depth : tot->max_depth;
    // ---- backward (the deepest level's delta is the 0.0 its settling wrote) ----
    for (int64_t d = depth - 1; d >= 0; --d) {
      ps.want = (int32_t)d + 1;
      LPA_TRY((bc_pull<B, true>(s, olist, runs[(size_t)d].base, runs[(size_t)d].n, ls.oo, ls.ocol, ps)));
    }
    hipLaunchKernelGGL(k_bc_accumulate<B>, dim3(grid_for(V)), dim3(256), 0, s, src + first, nb, ps, V, raw);
    LPA_HIP(hipGetLastError());
  }
  LPA_HIP(hipStreamSynchronize(s));
  return LPA_OK;
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream and bc_batch of the handle, nothing of the LPA state;
// every array is a stream-ordered temporary.  V > 0.
int betweenness(lpa_graph* g, const int32_t* sources, int32_t n_sources, int32_t directed, int32_t batch,
                double* raw_out, int32_t out_is_device, lpa_bc_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V;
  Tmp tmp(s);
  double* raw = raw_out;
  if (!out_is_device) LPA_TRY(tmp.get(&raw, V));
  LPA_HIP(hipMemsetAsync(raw, 0, sizeof(double) * (size_t)V, s));
  // ---- build ----
  ArcLists arcs;
  LPA_TRY(arcs_count(g, tmp, nullptr, &arcs, nullptr, !directed));
  if (summary) summary->arcs = arcs.E;
  Totals tot;
  int B = batch ? batch : g->bc_batch;
  int64_t batches = 0;
  if (n_sources > 0) {
    LPA_TRY(arcs_lists(g, tmp, &arcs));
    if (arcs.keys) {
      tmp.drop(arcs.keys);
      tmp.drop(arcs.flag);
      tmp.drop(arcs.pos);
    }
    Lists ls{V, arcs.oo, arcs.io, arcs.ocol, arcs.icol};
    if (!directed) {   // both orientations: the in-lists are the out-lists
      tmp.drop(arcs.icol);
      tmp.drop(arcs.io);
      ls.io = ls.oo;
      ls.icol = ls.ocol;
    }
    int32_t* src = nullptr;
    LPA_TRY(tmp.get(&src, n_sources));
    LPA_HIP(hipMemcpyAsync(src, sources, sizeof(int32_t) * (size_t)n_sources, hipMemcpyHostToDevice, s));
    for (;;) {
      int rc = LPA_EINVAL;
      switch (B) {
        case 1: rc = bc_passes<1>(g, ls, src, n_sources, raw, &tot); break;
        case 4: rc = bc_passes<4>(g, ls, src, n_sources, raw, &tot); break;
        case 8: rc = bc_passes<8>(g, ls, src, n_sources, raw, &tot); break;
        case 16: rc = bc_passes<16>(g, ls, src, n_sources, raw, &tot); break;
        default: set_error("lpa_betweenness: no kernels for a batch width of %d", B); break;
      }
      if (rc == LPA_ENOMEM && B > 1) {   // the state of this width does not fit: a narrower pass
        B = B == 4 ? 1 : B / 2;
        continue;
      }
      LPA_TRY(rc);
      break;
    }
    batches = ((int64_t)n_sources + B - 1) / B;
  }
  if (!out_is_device) LPA_HIP(hipMemcpyAsync(raw_out, raw, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->sources = n_sources;
    summary->batches = batches;
    summary->batch_width = B;
    summary->reached = tot.reached;
    summary->max_depth = tot.max_depth;
    summary->levels = tot.levels;
  }
  return LPA_OK;
}

}  // namespace lpa
