// Static PageRank of the handle's directed input multigraph (GraphFrame.pageRank(maxIter),
// GraphX PageRank.runWithOptions): every kept edge u -> v carries w[u] = 1 / outdeg[u],
// duplicates are edges of their own, a self-loop is one edge.  IEEE binary64 throughout.
//
//   keys     (dst << 32 | src) of every edge (an id outside [0, V): the edge gets the key
//            (V << 32 | V) and sorts behind every vertex in either half)
//   sort     radix sort, least significant digit first, over both halves.  After the
//            passes over the low half the keys are in source order: op[u] = the first key
//            with source >= u (a binary search per vertex), outdeg[u] = op[u + 1] - op[u]
//            -- the histogram of src without 2.7e8 scattered atomics (11.7 ms of a 42 ms
//            build at R-MAT-24).  After the high half every in-list is ascending by source
//            with duplicates adjacent: the layout is a function of the edge multiset
//   slots    between the two stages: slot[u] = the rank of u in (outdeg descending, id)
//            order, and the low half of every key becomes its source's slot.  c[] is indexed
//            by slot, so the sources gathered most share the first megabytes of c[] (what
//            an XCD's L2 keeps) and the sinks, never gathered, the tail: R-MAT-24 supersteps
//            4.37 -> 2.83 ms
//   rows     rp[v] = the first key with destination >= v (the same search; rp[V] = E, the
//            kept edges), col[i] = the low half of key i, indeg[v] = rp[v + 1] - rp[v]
//   iterate  a pull, max_iter times: s[v] = sum of c[col[i]] over the in-list of v,
//            r[v] = base(v) + (1 - a) s[v], c'[slot[v]] = r[v] w[v]; c double-buffered
//   finish   S = sum r (per-block partials of a fixed grid, then one block), r *= V / S
//            (with a source: r /= S); summary in two block-reduced passes
// keys .. rows with w, the form lists and the counters are pr_build(), which the parallel
// personalized call (lpa_ppr.hip) shares; iterate and finish are this file's own.
//
// Row forms, by in-degree L (boundaries: lpa_graph::pr_short / pr_wave):
//   short   L <= pr_short   8 lanes per row, 32 rows per block, rows in id order (rp, w, r
//           stream coalesced; a longer row is skipped here and listed).  L = 0 is always
//           a short row: it has nothing to gather
//   wave    L <= pr_wave    a wave per listed row (the lists: a flag byte per vertex and
//           form, scanned; ascending by id)
//   block   above           a block of 1024 per listed row (a hub of 10^6 in-edges: 16 waves
//           with four gathers in flight per lane)
//
// No floating-point atomics.  A row's sum has a shape fixed by L and the form: every lane
// adds its strided share in order (the wider forms in four interleaved accumulators,
// combined as (a0 + a1) + (a2 + a3)), then an xor-shuffle tree (both sides of an exchange
// form the same commutative sum), then, in the block form, the 16 wave sums in order.  S
// is reduced the same way over a grid that depends on V alone.  The ranks are therefore
// bit-identical across runs, handles and input edge orders.  The only atomics are integer
// ones of the summary (sinks, longest in-list, largest rank's bits and id): they commute.
//
// a + (1 - a) s and r w are written as the spec writes them, a product then a sum: no
// contraction into fused multiply-adds in this file.
#include <string.h>

#include "lpa_device.h"
#include "lpa_algo.h"

#pragma clang fp contract(off)

namespace lpa {

namespace {

__global__ __launch_bounds__(256) void k_pr_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                 int64_t m, u32 V, u64* __restrict__ keys) {
  GRID_STRIDE(i, m) {
    const u32 a = (u32)__builtin_nontemporal_load(src + i), b = (u32)__builtin_nontemporal_load(dst + i);
    keys[i] = a < V && b < V ? ((u64)b << 32) | a : ((u64)V << 32) | V;
  }
}

// Slots of c[]: the vertices in (out-degree descending, id ascending) order, so that the
// sources most often gathered share a few contiguous megabytes (L2-sized) and the sinks,
// which no edge ever gathers, lie behind everyone else.  ok[u] = (~outdeg[u] << 32 | u),
// in id order: a stable sort of the high half alone orders it.
__global__ __launch_bounds__(256) void k_pr_order_keys(const int64_t* __restrict__ op, int64_t V,
                                                       u64* __restrict__ ok) {
  GRID_STRIDE(u, V) ok[u] = ((u64)(0xFFFFFFFFu - (u32)(op[u + 1] - op[u])) << 32) | (u64)u;
}

__global__ __launch_bounds__(256) void k_pr_slots(const u64* __restrict__ ok, int64_t V, int32_t* __restrict__ slot) {
  GRID_STRIDE(i, V) slot[(u32)ok[i]] = (int32_t)i;
}

// keys in source order (the first sort stage): the low half becomes the source's slot
// (consecutive keys share or neighbour their source: slot[] streams); a dropped edge keeps V
__global__ __launch_bounds__(256) void k_pr_remap(u64* __restrict__ keys, int64_t m, u32 V,
                                                  const int32_t* __restrict__ slot) {
  GRID_STRIDE(i, m) {
    const u64 k = keys[i];
    const u32 a = (u32)k;
    if (a < V) keys[i] = (k & 0xFFFFFFFF00000000ull) | (u32)slot[a];
  }
}

// w of every vertex and its form flags (fw: a wave row, fb: a block row); cnt[0] the
// longest in-list, cnt[1] the sinks (two atomics per wave, at its end)
__global__ __launch_bounds__(256) void k_pr_rows(const int64_t* __restrict__ op, const int64_t* __restrict__ rp,
                                                 int64_t V, int64_t short_max, int64_t wave_max,
                                                 double* __restrict__ w, uint8_t* __restrict__ fw,
                                                 uint8_t* __restrict__ fb, u32* __restrict__ cnt) {
  u32 lmax = 0, sinks = 0;
  GRID_STRIDE(v, V) {
    const int64_t o = op[v + 1] - op[v], L = rp[v + 1] - rp[v];
    w[v] = o == 0 ? 0.0 : 1.0 / (double)o;
    fw[v] = L > short_max && L <= wave_max ? 1 : 0;   // short_max >= 0: L = 0 is in neither list
    fb[v] = L > short_max && L > wave_max ? 1 : 0;
    sinks += o == 0 ? 1u : 0u;
    lmax = (u32)L > lmax ? (u32)L : lmax;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const u32 o = (u32)__shfl_xor((int)lmax, off, 64);
    lmax = o > lmax ? o : lmax;
    sinks += (u32)__shfl_xor((int)sinks, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (lmax) atomicMax(&cnt[0], lmax);
    if (sinks) atomicAdd(&cnt[1], sinks);
  }
}

// r0 and c0 of every vertex
__global__ __launch_bounds__(256) void k_pr_start(int64_t V, int32_t source, const double* __restrict__ w,
                                                  const int32_t* __restrict__ slot, double* __restrict__ r,
                                                  double* __restrict__ c) {
  GRID_STRIDE(v, V) {
    const double rv = source < 0 || v == (int64_t)source ? 1.0 : 0.0;
    r[v] = rv;
    c[slot[v]] = rv * w[v];
  }
}

struct Update {   // what a row needs beside its sum
  double a, oma;        // resetProbability and 1 - a
  int32_t source;       // -1: none
  const double* w;      // [V] by vertex
  const int32_t* slot;  // [V] the vertex's slot in c[]
};

// a sink's c is never gathered: not written (its slot of either buffer is never read)
__device__ __forceinline__ void pr_finish(int64_t v, double s, const Update& up, double* __restrict__ r,
                                          double* __restrict__ cn) {
  const double base = up.source < 0 || v == (int64_t)up.source ? up.a : 0.0;
  const double rv = base + up.oma * s;
  const double wv = up.w[v];
  r[v] = rv;
  if (wv != 0.0) cn[up.slot[v]] = rv * wv;
}

// every row in id order, kShortLanes lanes each; a row longer than short_max is not this
// form's (L = 0 always is)
__global__ __launch_bounds__(256) void k_pr_short(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                  int64_t V, int64_t short_max, Update up, const double* __restrict__ c,
                                                  double* __restrict__ r, double* __restrict__ cn) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < V; base += (int64_t)gridDim.x * kRows) {
    const int64_t v = base + threadIdx.x / G;
    bool mine = false;
    double acc = 0.0;
    if (v < V) {
      const int64_t b = rp[v], L = rp[v + 1] - b;
      mine = L == 0 || L <= short_max;
      if (mine)
        for (int64_t i = sub; i < L; i += G) acc += c[col[b + i]];
    }
    // the G lanes of a row are neighbours: every one of them ends with the row's sum
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (mine && sub == 0) pr_finish(v, acc, up, r, cn);
  }
}

// this lane's share of a row of L entries at col + b, lanes `stride` apart: four
// interleaved accumulators (four gathers in flight), combined in a fixed order
__device__ __forceinline__ double pr_strided(const int32_t* __restrict__ col, const double* __restrict__ c, int64_t b,
                                             int64_t L, int first, int stride) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t i = first;
  for (; i + 3 * (int64_t)stride < L; i += 4 * (int64_t)stride) {
    const int32_t u0 = col[b + i], u1 = col[b + i + stride], u2 = col[b + i + 2 * (int64_t)stride],
                  u3 = col[b + i + 3 * (int64_t)stride];
    a0 += c[u0];
    a1 += c[u1];
    a2 += c[u2];
    a3 += c[u3];
  }
  for (; i < L; i += stride) a0 += c[col[b + i]];
  return (a0 + a1) + (a2 + a3);
}

__device__ __forceinline__ double pr_wave_sum(double acc) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  return acc;
}

// a wave per listed row
__global__ __launch_bounds__(256) void k_pr_wave(const int32_t* __restrict__ rows, int64_t nrows,
                                                 const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                 Update up, const double* __restrict__ c, double* __restrict__ r,
                                                 double* __restrict__ cn) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t v = rows[k];
    const int64_t b = rp[v];
    const double s = pr_wave_sum(pr_strided(col, c, b, rp[v + 1] - b, lane, 64));
    if (lane == 0) pr_finish(v, s, up, r, cn);
  }
}

// a block per listed row (k is the same in every thread: barriers inside)
__global__ __launch_bounds__(kBlockThreads) void k_pr_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                            const int64_t* __restrict__ rp,
                                                            const int32_t* __restrict__ col, Update up,
                                                            const double* __restrict__ c, double* __restrict__ r,
                                                            double* __restrict__ cn) {
  constexpr int kWaves = kBlockThreads / 64;
  __shared__ double ws[kWaves];
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t v = rows[k];
    const int64_t b = rp[v];
    const double s = pr_wave_sum(pr_strided(col, c, b, rp[v + 1] - b, threadIdx.x, kBlockThreads));
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = ws[0];
      for (int i = 1; i < kWaves; ++i) t += ws[i];
      pr_finish(v, t, up, r, cn);
    }
    __syncthreads();   // before the next row rewrites ws
  }
}

// the block's sum of x over the threads, in thread 0 (fixed shape: wave tree, then the
// four wave sums in order)
__device__ __forceinline__ double pr_block_sum(double x, double* ws) {
  x = pr_wave_sum(x);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((ws[0] + ws[1]) + (ws[2] + ws[3]));
}

// part[block] = the block's share of sum r (the launch's grid is grid_bh(V): V alone)
__global__ __launch_bounds__(256) void k_pr_partials(const double* __restrict__ r, int64_t V,
                                                     double* __restrict__ part) {
  __shared__ double ws[4];
  double x = 0.0;
  GRID_STRIDE(v, V) x += r[v];
  x = pr_block_sum(x, ws);
  if (threadIdx.x == 0) part[blockIdx.x] = x;
}

// one block: fin[0] = S, fin[1] = V / S
__global__ __launch_bounds__(256) void k_pr_total(const double* __restrict__ part, int n, int64_t V,
                                                  double* __restrict__ fin) {
  __shared__ double ws[4];
  double x = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) x += part[i];
  x = pr_block_sum(x, ws);
  if (threadIdx.x == 0) {
    fin[0] = x;
    fin[1] = (double)V / x;
  }
}

// normalizeRankSum, and acc[0] = the bits of the largest normalised rank (ranks are
// >= 0: their order is the order of their bit patterns)
__global__ __launch_bounds__(256) void k_pr_scale(double* __restrict__ r, int64_t V, const double* __restrict__ fin,
                                                  int personalised, ull* __restrict__ acc) {
  __shared__ ull ws[4];
  const double S = fin[0], f = fin[1];
  ull best = 0;
  GRID_STRIDE(v, V) {
    const double x = personalised ? r[v] / S : r[v] * f;
    r[v] = x;
    best = dev::umax64(best, (ull)__double_as_longlong(x));
  }
  for (int off = 32; off > 0; off >>= 1) best = dev::umax64(best, __shfl_xor(best, off, 64));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    best = dev::umax64(dev::umax64(ws[0], ws[1]), dev::umax64(ws[2], ws[3]));
    if (best) atomicMax(&acc[0], best);
  }
}

// acc[1] (preset to ~0) = the smallest v whose rank has the bits acc[0]
__global__ __launch_bounds__(256) void k_pr_argmax(const double* __restrict__ r, int64_t V, ull* __restrict__ acc) {
  __shared__ ull ws[4];
  const ull best = acc[0];
  ull id = ~0ull;
  GRID_STRIDE(v, V) {
    if ((ull)__double_as_longlong(r[v]) == best && (ull)v < id) id = (ull)v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const ull o = __shfl_xor(id, off, 64);
    id = o < id ? o : id;
  }
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = id;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) id = ws[i] < id ? ws[i] : id;
    if (id != ~0ull) atomicMin(&acc[1], id);
  }
}

__global__ __launch_bounds__(256) void k_pr_degrees(const int64_t* __restrict__ op, const int64_t* __restrict__ rp,
                                                    int64_t V, int64_t* __restrict__ outdeg,
                                                    int64_t* __restrict__ indeg) {
  GRID_STRIDE(v, V) {
    if (outdeg) outdeg[v] = op[v + 1] - op[v];
    if (indeg) indeg[v] = rp[v + 1] - rp[v];
  }
}

}  // namespace

PrCsr::~PrCsr() {
  for (int i = 0; i < n; ++i) tmp_free(ptrs[i], s);
}

// The build half of a PageRank call.  Reads V (> 0), m, e_src / e_dst, the stream and the
// pr_* boundaries of the handle, nothing of the LPA state; the arrays of *b outlive the call,
// everything else is freed in stream order before it returns.
int pr_build(lpa_graph* g, PrCsr* b) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  b->s = s;
  const auto keep = [&](auto** p, int64_t count) {
    LPA_TRY(tmp_alloc((void**)p, sizeof(**p) * (size_t)(count > 0 ? count : 1), s));
    b->ptrs[b->n++] = *p;
    return (int)LPA_OK;
  };
  Tmp tmp(s);
  u32 *cnt = nullptr, *pw = nullptr, *pb = nullptr;
  uint8_t *fw = nullptr, *fb = nullptr;
  LPA_TRY(keep(&b->op, V + 1));
  LPA_TRY(keep(&b->rp, V + 1));
  LPA_TRY(keep(&b->lists, 2 * V));
  LPA_TRY(tmp.get(&cnt, 2));
  LPA_TRY(tmp.get(&fw, V));
  LPA_TRY(tmp.get(&fb, V));
  LPA_TRY(tmp.get(&pw, V + 1));
  LPA_TRY(tmp.get(&pb, V + 1));
  LPA_TRY(keep(&b->w, V));
  LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(u32) * 2, s));
  int64_t *op = b->op, *rp = b->rp;
  u64* keys = nullptr;   // [2 m]: the keys and the sort's other buffer
  u64* ok = nullptr;     // [2 V]: the vertex order's keys and their sort's other buffer
  LPA_TRY(tmp.get(&ok, 2 * V));
  LPA_TRY(keep(&b->slot, V));
  int32_t* slot = b->slot;
  // the halves hold values up to V (a dropped edge); the sort is stable, so the passes
  // over the high half keep the source order inside every row
  const HalfShifts sh(bits_for((uint64_t)V));
  if (m > 0) {
    LPA_TRY(tmp.get(&keys, 2 * m));
    hipLaunchKernelGGL(k_pr_keys, dim3(grid_for(m)), dim3(256), 0, s, g->e_src, g->e_dst, m, (u32)V, keys);
    LPA_HIP(hipGetLastError());
    LPA_TRY(radix_sort_u64(keys, keys + m, m, sh.lo(), sh.ns, s));
    LPA_TRY(key_bounds(keys, m, V, false, op, s));
  } else {
    LPA_HIP(hipMemsetAsync(op, 0, sizeof(int64_t) * (size_t)(V + 1), s));
  }
  const int all_hi[4] = {32, 40, 48, 56};
  hipLaunchKernelGGL(k_pr_order_keys, dim3(grid_for(V)), dim3(256), 0, s, op, V, ok);
  LPA_HIP(hipGetLastError());
  LPA_TRY(radix_sort_u64(ok, ok + V, V, all_hi, 4, s));
  hipLaunchKernelGGL(k_pr_slots, dim3(grid_for(V)), dim3(256), 0, s, ok, V, slot);
  LPA_HIP(hipGetLastError());
  if (m > 0) {
    hipLaunchKernelGGL(k_pr_remap, dim3(grid_for(m)), dim3(256), 0, s, keys, m, (u32)V, slot);
    LPA_HIP(hipGetLastError());
    LPA_TRY(radix_sort_u64(keys, keys + m, m, sh.hi(), sh.ns, s));
    LPA_TRY(key_bounds(keys, m, V, true, rp, s));
  } else {
    LPA_HIP(hipMemsetAsync(rp, 0, sizeof(int64_t) * (size_t)(V + 1), s));
  }
  hipLaunchKernelGGL(k_pr_rows, dim3(grid_bh(V)), dim3(256), 0, s, op, rp, V, (int64_t)g->pr_short,
                     (int64_t)g->pr_wave, b->w, fw, fb, cnt);
  LPA_HIP(hipGetLastError());
  LPA_TRY(exclusive_scan_u8_u32(fw, pw, V, s));
  LPA_TRY(exclusive_scan_u8_u32(fb, pb, V, s));
  LPA_TRY(fill_form_lists(fw, fb, pw, pb, V, b->lists, s));
  u32 hc[2] = {0, 0};   // the longest in-list and the sinks
  LPA_HIP(hipMemcpyAsync(&b->E, rp + V, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(&b->n_wave, pw + V, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(&b->n_block, pb + V, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  b->max_in = hc[0];
  b->sinks = hc[1];
  LPA_TRY(keep(&b->col, b->E));
  if (b->E > 0) LPA_TRY(key_col(keys, b->E, b->col, s));
  return LPA_OK;
}

// Every array is a stream-ordered temporary.
int pagerank(lpa_graph* g, int32_t max_iter, double reset_prob, int32_t source, double* rank_out,
             int64_t* out_degree_out, int64_t* in_degree_out, int32_t out_is_device, lpa_pagerank_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V;
  if (summary) *summary = lpa_pagerank_summary{0.0, 0.0, -1, 0, 0, 0};
  if (V == 0) return LPA_OK;
  PrCsr csr;
  LPA_TRY(pr_build(g, &csr));
  const int64_t *op = csr.op, *rp = csr.rp;
  const int32_t *col = csr.col, *lists = csr.lists, *slot = csr.slot;
  const double* w = csr.w;
  const int64_t E = csr.E;
  const u32 h[2] = {csr.n_wave, csr.n_block}, hc[2] = {csr.max_in, csr.sinks};
  Tmp tmp(s);
  double *r = rank_out, *c[2] = {nullptr, nullptr};
  if (!out_is_device) LPA_TRY(tmp.get(&r, V));
  LPA_TRY(tmp.get(&c[0], V));
  LPA_TRY(tmp.get(&c[1], V));
  hipLaunchKernelGGL(k_pr_start, dim3(grid_for(V)), dim3(256), 0, s, V, source, w, slot, r, c[0]);
  LPA_HIP(hipGetLastError());
  // ---- iterate ----
  const Update up{reset_prob, 1.0 - reset_prob, source, w, slot};
  const unsigned g_short = grid_rows(V, 256 / kShortLanes, 65536);
  for (int32_t it = 0; it < max_iter; ++it) {
    const double* cc = c[it & 1];
    double* cn = c[(it & 1) ^ 1];
    hipLaunchKernelGGL(k_pr_short, dim3(g_short), dim3(256), 0, s, rp, col, V, (int64_t)g->pr_short, up, cc, r, cn);
    if (h[0])
      hipLaunchKernelGGL(k_pr_wave, dim3(grid_rows(h[0], 4, 16384)), dim3(256), 0, s, lists, (int64_t)h[0], rp, col, up,
                         cc, r, cn);
    if (h[1])
      hipLaunchKernelGGL(k_pr_block, dim3(grid_rows(h[1], 1, 4096)), dim3(kBlockThreads), 0, s, lists + V,
                         (int64_t)h[1], rp, col, up, cc, r, cn);
    LPA_HIP(hipGetLastError());
  }
  // ---- finish ----
  double* part = nullptr;
  double* fin = nullptr;
  ull* acc = nullptr;
  const unsigned gp = grid_bh(V);
  LPA_TRY(tmp.get(&part, gp));
  LPA_TRY(tmp.get(&fin, 2));
  LPA_TRY(tmp.get(&acc, 2));
  LPA_HIP(hipMemsetAsync(acc, 0, sizeof(ull), s));
  LPA_HIP(hipMemsetAsync(acc + 1, 0xFF, sizeof(ull), s));
  hipLaunchKernelGGL(k_pr_partials, dim3(gp), dim3(256), 0, s, r, V, part);
  hipLaunchKernelGGL(k_pr_total, dim3(1), dim3(256), 0, s, part, (int)gp, V, fin);
  hipLaunchKernelGGL(k_pr_scale, dim3(gp), dim3(256), 0, s, r, V, fin, source >= 0 ? 1 : 0, acc);
  LPA_HIP(hipGetLastError());
  double hfin[2] = {0.0, 0.0};
  ull hacc[2] = {0, 0};
  if (summary) {
    hipLaunchKernelGGL(k_pr_argmax, dim3(gp), dim3(256), 0, s, r, V, acc);
    LPA_HIP(hipGetLastError());
    LPA_HIP(hipMemcpyAsync(hfin, fin, sizeof(hfin), hipMemcpyDeviceToHost, s));
    LPA_HIP(hipMemcpyAsync(hacc, acc, sizeof(hacc), hipMemcpyDeviceToHost, s));
  }
  if (out_degree_out || in_degree_out) {
    int64_t *dout = out_degree_out, *din = in_degree_out;
    if (!out_is_device) {
      if (dout) LPA_TRY(tmp.get(&dout, V));
      if (din) LPA_TRY(tmp.get(&din, V));
    }
    hipLaunchKernelGGL(k_pr_degrees, dim3(grid_for(V)), dim3(256), 0, s, op, rp, V, dout, din);
    LPA_HIP(hipGetLastError());
    if (!out_is_device) {
      if (dout) LPA_HIP(hipMemcpyAsync(out_degree_out, dout, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
      if (din) LPA_HIP(hipMemcpyAsync(in_degree_out, din, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    }
  }
  if (!out_is_device) LPA_HIP(hipMemcpyAsync(rank_out, r, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->rank_sum = hfin[0];
    memcpy(&summary->max_rank, &hacc[0], sizeof(double));
    summary->max_rank_id = (int64_t)hacc[1];
    summary->edges = E;
    summary->sinks = (int64_t)hc[1];
    summary->max_in_degree = (int64_t)hc[0];
  }
  return LPA_OK;
}

}  // namespace lpa
