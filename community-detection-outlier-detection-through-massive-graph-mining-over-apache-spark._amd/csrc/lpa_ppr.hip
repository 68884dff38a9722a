// Parallel personalized PageRank (GraphFrame.parallelPersonalizedPageRank, GraphX
// PageRank.runParallelPersonalizedPageRank): lpa_pagerank's personalised form from many
// sources in one call.  The in-list CSR is lpa_pr.hip's (pr_build: rp, col by slot, w, the
// form lists), built once; the sources then run B to a pass, B = 4, 8 or 16 (lpa_graph::
// ppr_batch), a sparse matrix times a skinny dense one.  IEEE binary64 throughout.
//
//   layout   c[slot][B] and r[v][B]: a slot's B doubles are contiguous and aligned to 8 B
//            bytes, so the gather of one in-edge is 8 B contiguous bytes for all B sources
//            (B = 16: one 128-byte line) where the single-source gather moves a line for 8
//            useful bytes.  col, rp, the lists and w are read once per pass, not per source
//   lanes    a lane owns two neighbouring columns (one 16-byte load per entry): B / 2
//            "column lanes" side by side read an entry's 8 B bytes in one coalesced piece,
//            and the lanes of a row that remain are "phases" that split the row's entries.
//            A lane carries 4 x 2 doubles of accumulators at every B (not B per lane): the
//            four gathers in flight of lpa_pr.hip fit the register budget at B = 16 too
//   start    c0 = 0 but w[source] at (slot[source], column); r is not kept between the
//            supersteps (c carries the state): only the last superstep writes it
//   iterate  max_iter times: s[v][b] = sum of c[col[i]][b] over the in-list of v,
//            r = base + (1 - a) s, c'[slot[v]][b] = r w[v]; c double-buffered; a sink's c is
//            never written (nor read); a padding column of the last pass starts at 0.0
//            everywhere, has no source (base 0.0) and is not written out
//   finish   per pass: S[b] = sum_v r[v][b] (per-block partials of a grid that depends on
//            V alone, then one block), then one tiled pass divides, transposes r[v][b] into
//            rank_out[(first + b) * V + v] with coalesced writes and counts the positive ranks
//
// Row forms: lpa_pr.hip's, on the same boundaries and lists.  With CL = B / 2 column lanes
//   short   8 lanes per row, rows in id order: 8 / CL phases
//   wave    a wave per listed row: 64 / CL phases
//   block   1024 threads per listed row: 1024 / CL phases
//
// No floating-point atomics.  A column's sum has a shape fixed by the row's length, the form
// and B: a lane adds its phase's strided share of the entries in four interleaved
// accumulators, (a0 + a1) + (a2 + a3); an xor-shuffle tree over the phases of a wave (both
// sides of an exchange form the same commutative sum); in the block form the 16 wave sums
// in order.  Which lane and which half of it a column sits in moves no operand: every
// column of a pass goes through the same shape, so a source's ranks do not depend on its
// position in the call or on its company.  S is reduced over a grid that depends on V alone,
// every column over the same partition of the vertices.  The only atomic is the integer
// count of the positive ranks.
//
// a + (1 - a) s and r w are written as the spec writes them: no contraction in this file.
#include <string.h>

#include <vector>

#include "lpa_device.h"
#include "lpa_algo.h"

#pragma clang fp contract(off)

namespace lpa {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));   // a lane's two columns: one 16-byte access

constexpr int kTile = 64;           // vertices per tile of the transposing finish

struct Pass {   // what a row needs beside its sums
  double a, oma;               // resetProbability and 1 - a
  const int32_t* src;          // [B] the pass's sources by column; -1: a padding column
  const double* w;             // [V] by vertex
  const int32_t* slot;         // [V] the vertex's slot in c[]
  int write_r;                 // the last superstep: r is read by the finish
};

// c0: zero (the launch follows a memset), but w[source] in the source's own column; a sink
// source has w = 0.0 and writes the zero again
template <int B>
__global__ void k_ppr_start(Pass ps, double* __restrict__ c) {
  const int b = threadIdx.x;
  if (b < B && ps.src[b] >= 0) c[(int64_t)ps.slot[ps.src[b]] * B + b] = 1.0 * ps.w[ps.src[b]];
}

// this lane's share of a row of L entries at col + b0, for its two columns at c + 2 cl:
// the entries first, first + stride, ... in four interleaved accumulators
template <int B>
__device__ __forceinline__ d2 ppr_strided(const int32_t* __restrict__ col, const double* __restrict__ c, int64_t b0,
                                          int64_t L, int first, int stride, int cl) {
  const d2* __restrict__ cv = reinterpret_cast<const d2*>(c) + cl;   // entry u: cv[u * (B / 2)]
  constexpr int64_t kRow = B / 2;
  d2 a0 = {0.0, 0.0}, a1 = a0, a2 = a0, a3 = a0;
  int64_t i = first;
  for (; i + 3 * (int64_t)stride < L; i += 4 * (int64_t)stride) {
    const int32_t u0 = col[b0 + i], u1 = col[b0 + i + stride], u2 = col[b0 + i + 2 * (int64_t)stride],
                  u3 = col[b0 + i + 3 * (int64_t)stride];
    a0 += cv[u0 * kRow];
    a1 += cv[u1 * kRow];
    a2 += cv[u2 * kRow];
    a3 += cv[u3 * kRow];
  }
  for (; i < L; i += stride) a0 += cv[col[b0 + i] * kRow];
  return (a0 + a1) + (a2 + a3);
}

__device__ __forceinline__ d2 shfl_xor_d2(d2 x, int off) {
  d2 o;
  o.x = __shfl_xor(x.x, off, 64);
  o.y = __shfl_xor(x.y, off, 64);
  return o;
}

// the sum over the lanes that share this lane's columns among `lanes` neighbours (a power
// of two, <= 64): the offsets lanes / 2 ... B / 2 (none when lanes == B / 2)
template <int B>
__device__ __forceinline__ d2 ppr_phase_sum(d2 acc, int lanes) {
  for (int off = lanes / 2; off >= B / 2; off >>= 1) acc += shfl_xor_d2(acc, off);
  return acc;
}

// the lane's two columns of row v from their sums
template <int B>
__device__ __forceinline__ void ppr_finish(int64_t v, d2 s, int cl, const Pass& ps, double* __restrict__ r,
                                           double* __restrict__ cn) {
  d2 base;
  base.x = v == (int64_t)ps.src[2 * cl] ? ps.a : 0.0;
  base.y = v == (int64_t)ps.src[2 * cl + 1] ? ps.a : 0.0;
  const d2 rv = base + ps.oma * s;
  const double wv = ps.w[v];
  if (ps.write_r) reinterpret_cast<d2*>(r)[v * (B / 2) + cl] = rv;
  if (wv != 0.0) reinterpret_cast<d2*>(cn)[(int64_t)ps.slot[v] * (B / 2) + cl] = rv * wv;
}

// every row in id order, kShortLanes lanes each; a row longer than short_max is not this
// form's (L = 0 always is)
template <int B>
__global__ __launch_bounds__(256) void k_ppr_short(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                   int64_t V, int64_t short_max, Pass ps,
                                                   const double* __restrict__ c, double* __restrict__ r,
                                                   double* __restrict__ cn) {
  constexpr int G = kShortLanes, kRows = 256 / G, CL = B / 2, P = G / CL;
  static_assert(CL <= G, "a row's lanes cover its columns");
  const int sub = threadIdx.x & (G - 1), cl = sub % CL, ph = sub / CL;
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < V; base += (int64_t)gridDim.x * kRows) {
    const int64_t v = base + threadIdx.x / G;
    bool mine = false;
    d2 acc = {0.0, 0.0};
    if (v < V) {
      const int64_t b0 = rp[v], L = rp[v + 1] - b0;
      mine = L == 0 || L <= short_max;
      if (mine) acc = ppr_strided<B>(col, c, b0, L, ph, P, cl);
    }
    acc = ppr_phase_sum<B>(acc, G);   // the G lanes of a row are neighbours
    if (mine && ph == 0) ppr_finish<B>(v, acc, cl, ps, r, cn);
  }
}

// a wave per listed row
template <int B>
__global__ __launch_bounds__(256) void k_ppr_wave(const int32_t* __restrict__ rows, int64_t nrows,
                                                  const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                  Pass ps, const double* __restrict__ c, double* __restrict__ r,
                                                  double* __restrict__ cn) {
  constexpr int CL = B / 2;
  const int lane = threadIdx.x & 63, cl = lane % CL, ph = lane / CL;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t v = rows[k];
    const int64_t b0 = rp[v];
    const d2 s = ppr_phase_sum<B>(ppr_strided<B>(col, c, b0, rp[v + 1] - b0, ph, 64 / CL, cl), 64);
    if (ph == 0) ppr_finish<B>(v, s, cl, ps, r, cn);
  }
}

// a block per listed row (k is the same in every thread: barriers inside)
template <int B>
__global__ __launch_bounds__(kBlockThreads) void k_ppr_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                             const int64_t* __restrict__ rp,
                                                             const int32_t* __restrict__ col, Pass ps,
                                                             const double* __restrict__ c, double* __restrict__ r,
                                                             double* __restrict__ cn) {
  constexpr int kWaves = kBlockThreads / 64, CL = B / 2;
  __shared__ d2 ws[kWaves][CL];
  const int cl = threadIdx.x % CL, ph = threadIdx.x / CL;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t v = rows[k];
    const int64_t b0 = rp[v];
    const d2 s = ppr_phase_sum<B>(ppr_strided<B>(col, c, b0, rp[v + 1] - b0, ph, kBlockThreads / CL, cl), 64);
    if ((threadIdx.x & 63) < CL) ws[threadIdx.x >> 6][cl] = s;
    __syncthreads();
    if (threadIdx.x < CL) {
      d2 t = ws[0][cl];
      for (int i = 1; i < kWaves; ++i) t += ws[i][cl];
      ppr_finish<B>(v, t, cl, ps, r, cn);
    }
    __syncthreads();   // before the next row rewrites ws
  }
}

// The sum of x over the block's threads that share threadIdx.x % B, in the threads below B
// (fixed shape: the wave's tree over the lane bits from B up, then the four wave sums)
template <int B>
__device__ __forceinline__ double ppr_column_sum(double x, double (*ws)[B]) {
  for (int off = 32; off >= B; off >>= 1) x += __shfl_xor(x, off, 64);
  if ((threadIdx.x & 63) < B) ws[threadIdx.x >> 6][threadIdx.x & 63] = x;
  __syncthreads();
  const int b = threadIdx.x & (B - 1);
  return (ws[0][b] + ws[1][b]) + (ws[2][b] + ws[3][b]);
}

// part[block][b] = the block's share of sum_v r[v][b].  r as one array of V B doubles: the
// grid's stride is a multiple of B, so a thread stays in column threadIdx.x % B, and the
// vertices it visits are the same for every column (the launch's grid is grid_bh(V))
template <int B>
__global__ __launch_bounds__(256) void k_ppr_partials(const double* __restrict__ r, int64_t V,
                                                      double* __restrict__ part) {
  __shared__ double ws[4][B];
  double x = 0.0;
  GRID_STRIDE(i, V * B) x += r[i];
  x = ppr_column_sum<B>(x, ws);
  if (threadIdx.x < B) part[(int64_t)blockIdx.x * B + threadIdx.x] = x;
}

// one block: S[b] = the sum of the n partials of column b
template <int B>
__global__ __launch_bounds__(256) void k_ppr_total(const double* __restrict__ part, int n, double* __restrict__ S) {
  __shared__ double ws[4][B];
  double x = 0.0;
  for (int i = threadIdx.x; i < n * B; i += 256) x += part[i];
  x = ppr_column_sum<B>(x, ws);
  if (threadIdx.x < B) S[threadIdx.x] = x;
}

// out[b * V + v] = r[v][b] / S[b] for the pass's nb real columns, a tile of kTile vertices
// at a time through LDS (reads along r's rows, writes along out's); nz += the positive ranks
template <int B>
__global__ __launch_bounds__(256) void k_ppr_scale(const double* __restrict__ r, int64_t V,
                                                   const double* __restrict__ S, int nb, double* __restrict__ out,
                                                   ull* __restrict__ nz) {
  __shared__ double tile[B][kTile + 1];
  const int64_t ntiles = (V + kTile - 1) / kTile;
  u32 pos = 0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t v0 = t * kTile;
    const int64_t nv = V - v0 < kTile ? V - v0 : kTile;
    for (int j = threadIdx.x; j < nv * B; j += 256) tile[j % B][j / B] = r[v0 * B + j];
    __syncthreads();
    for (int j = threadIdx.x; j < nb * kTile; j += 256) {
      const int b = j / kTile, dv = j % kTile;
      if (dv < nv) {
        const double x = tile[b][dv] / S[b];
        out[(int64_t)b * V + v0 + dv] = x;
        pos += x > 0.0 ? 1u : 0u;
      }
    }
    __syncthreads();   // before the next tile is written
  }
  for (int off = 32; off > 0; off >>= 1) pos += (u32)__shfl_xor((int)pos, off, 64);
  if ((threadIdx.x & 63) == 0 && pos) atomicAdd(nz, (ull)pos);
}

// the passes over a built CSR; S_all (device) receives batches * B sums, pass by pass
template <int B>
int ppr_passes(lpa_graph* g, const PrCsr& csr, int32_t max_iter, double reset_prob, const int32_t* sources,
               int32_t n_sources, double* rank_out, int32_t out_is_device, double* S_all, ull* nz) {
  // sources: device, padded with -1 to a multiple of B
  hipStream_t s = g->stream;
  const int64_t V = g->V;
  Tmp tmp(s);
  double *r = nullptr, *c[2] = {nullptr, nullptr}, *stage = nullptr, *part = nullptr;
  const unsigned gp = grid_bh(V);
  LPA_TRY(tmp.get(&r, V * B));
  LPA_TRY(tmp.get(&c[0], V * B));
  LPA_TRY(tmp.get(&c[1], V * B));
  LPA_TRY(tmp.get(&part, (int64_t)gp * B));
  if (!out_is_device) LPA_TRY(tmp.get(&stage, V * B));
  const unsigned g_short = grid_rows(V, 256 / kShortLanes, 65536);
  const unsigned g_scale = grid_rows((V + kTile - 1) / kTile, 1, 16384);
  for (int32_t first = 0; first < n_sources; first += B) {
    const int nb = n_sources - first < B ? n_sources - first : B;
    Pass ps{reset_prob, 1.0 - reset_prob, sources + first, csr.w, csr.slot, 0};
    LPA_HIP(hipMemsetAsync(c[0], 0, sizeof(double) * (size_t)(V * B), s));
    hipLaunchKernelGGL(k_ppr_start<B>, dim3(1), dim3(64), 0, s, ps, c[0]);
    LPA_HIP(hipGetLastError());
    for (int32_t it = 0; it < max_iter; ++it) {
      const double* cc = c[it & 1];
      double* cn = c[(it & 1) ^ 1];
      ps.write_r = it == max_iter - 1 ? 1 : 0;
      hipLaunchKernelGGL(k_ppr_short<B>, dim3(g_short), dim3(256), 0, s, csr.rp, csr.col, V, (int64_t)g->pr_short, ps,
                         cc, r, cn);
      if (csr.n_wave)
        hipLaunchKernelGGL(k_ppr_wave<B>, dim3(grid_rows(csr.n_wave, 4, 16384)), dim3(256), 0, s, csr.lists,
                           (int64_t)csr.n_wave, csr.rp, csr.col, ps, cc, r, cn);
      if (csr.n_block)
        hipLaunchKernelGGL(k_ppr_block<B>, dim3(grid_rows(csr.n_block, 1, 4096)), dim3(kBlockThreads), 0, s,
                           csr.lists + V, (int64_t)csr.n_block, csr.rp, csr.col, ps, cc, r, cn);
      LPA_HIP(hipGetLastError());
    }
    double* S = S_all + (int64_t)(first / B) * B;
    double* out = out_is_device ? rank_out + (int64_t)first * V : stage;
    hipLaunchKernelGGL(k_ppr_partials<B>, dim3(gp), dim3(256), 0, s, r, V, part);
    hipLaunchKernelGGL(k_ppr_total<B>, dim3(1), dim3(256), 0, s, part, (int)gp, S);
    hipLaunchKernelGGL(k_ppr_scale<B>, dim3(g_scale), dim3(256), 0, s, r, V, S, nb, out, nz);
    LPA_HIP(hipGetLastError());
    if (!out_is_device)
      LPA_HIP(hipMemcpyAsync(rank_out + (int64_t)first * V, stage, sizeof(double) * (size_t)(V * nb),
                             hipMemcpyDeviceToHost, s));
  }
  return LPA_OK;
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream, the pr_* boundaries and ppr_batch of the handle,
// nothing of the LPA state; every array is a stream-ordered temporary.
int parallel_pagerank(lpa_graph* g, int32_t max_iter, double reset_prob, const int32_t* sources, int32_t n_sources,
                      double* rank_out, int32_t out_is_device, double* rank_sum_out, lpa_ppr_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V;
  if (summary) memset(summary, 0, sizeof(*summary));
  if (V == 0) return LPA_OK;
  if (n_sources == 0 && !summary) return LPA_OK;
  PrCsr csr;
  LPA_TRY(pr_build(g, &csr));
  if (summary) {
    summary->edges = csr.E;
    summary->sinks = (int64_t)csr.sinks;
    summary->max_in_degree = (int64_t)csr.max_in;
  }
  if (n_sources == 0) return LPA_OK;
  const int B = g->ppr_batch;
  const int64_t batches = ((int64_t)n_sources + B - 1) / B;
  Tmp tmp(s);
  double* S_all = nullptr;
  ull* nz = nullptr;
  int32_t* src = nullptr;   // the sources, padded with -1 to whole passes
  LPA_TRY(tmp.get(&S_all, batches * B));
  LPA_TRY(tmp.get(&src, batches * B));
  LPA_HIP(hipMemsetAsync(src, 0xFF, sizeof(int32_t) * (size_t)(batches * B), s));
  LPA_HIP(hipMemcpyAsync(src, sources, sizeof(int32_t) * (size_t)n_sources, hipMemcpyHostToDevice, s));
  LPA_TRY(tmp.get(&nz, 1));
  LPA_HIP(hipMemsetAsync(nz, 0, sizeof(ull), s));
  switch (B) {
    case 4:
      LPA_TRY(ppr_passes<4>(g, csr, max_iter, reset_prob, src, n_sources, rank_out, out_is_device, S_all, nz));
      break;
    case 8:
      LPA_TRY(ppr_passes<8>(g, csr, max_iter, reset_prob, src, n_sources, rank_out, out_is_device, S_all, nz));
      break;
    case 16:
      LPA_TRY(ppr_passes<16>(g, csr, max_iter, reset_prob, src, n_sources, rank_out, out_is_device, S_all, nz));
      break;
    default:
      set_error("lpa_parallel_pagerank: no kernels for a batch width of %d", B);
      return LPA_EINVAL;
  }
  std::vector<double> hs((size_t)(batches * B));   // the S of every column, padding included
  double* hS = hs.data();
  ull hnz = 0;
  LPA_HIP(hipMemcpyAsync(hS, S_all, sizeof(double) * (size_t)(batches * B), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(&hnz, nz, sizeof(ull), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  if (rank_sum_out) memcpy(rank_sum_out, hS, sizeof(double) * (size_t)n_sources);
  if (summary) {
    double lo = hS[0], hi = hS[0];
    for (int32_t l = 1; l < n_sources; ++l) {
      lo = hS[l] < lo ? hS[l] : lo;
      hi = hS[l] > hi ? hS[l] : hi;
    }
    summary->batches = batches;
    summary->batch_width = B;
    summary->nonzero = (int64_t)hnz;
    summary->rank_sum_min = lo;
    summary->rank_sum_max = hi;
  }
  return LPA_OK;
}

}  // namespace lpa
