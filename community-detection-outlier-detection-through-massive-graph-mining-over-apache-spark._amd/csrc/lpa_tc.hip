// Triangles per vertex of the handle's input multigraph (GraphFrame.triangleCount):
// count[v] = the triangles of the canonical simple undirected graph (no self-loops, no
// direction, duplicates collapsed) that contain v.
//
//   keys     (min << 32 | max) of every edge, radix-sorted; the first key of each run with
//            min != max is a simple edge: marked, scanned (lpa_adj.hip: simple_edges),
//            compacted                                                         (E of them)
//   degrees  d[v] of the simple graph: the min side by runs of the sorted keys (one atomic
//            per run and wave), the max side one atomic per edge
//   orient   every simple edge {a, b} points from the endpoint of lower rank (d, id) to
//            the higher; the oriented keys (from << 32 | to) are sorted again, which
//            gives the CSR rp[] / col[] with every out-list N+(u) ascending by id
//   count    for every oriented edge u -> v, every w in N+(u) n N+(v) closes a triangle:
//            count[u], count[v], count[w] += 1
//   summary  two block-reduced passes (sums and the maximum; then the smallest id at it)
//
// Orientation.  Rank (d, id) is a strict total order, so a triangle has exactly one
// vertex u of lowest rank, and both its other corners v, w are out-neighbours of u; of
// v, w the lower one, say v, has w as an out-neighbour.  The triangle is therefore met
// exactly once: at edge u -> v, match w.  (With degree alone, a regular graph would
// have no order at all; the id decides there.)  An out-neighbour has rank above its
// source, hence degree >= L = |N+(u)|: L vertices of degree >= L need L^2 / 2 <= E, so
// every out-list holds at most sqrt(2 E) entries.  A row with L < 2 is no apex: skipped.
//
// Count kernels, by L (boundaries: lpa_graph::tc_short / tc_wave / tc_lds):
//   group   L <= tc_short   8 lanes per row, 8 rows per wave.  Items = the ordered pairs
//           (v, w) of N+(u), spread over the 8 lanes; item: binary search of w in N+(v)
//           (global memory: the lists are short, the hot ones sit in L2)
//   wave    L <= tc_wave    a wave per row, N+(u) staged in the wave's LDS region
//   block   L <= tc_lds     a block per row, N+(u) staged in (dynamic) LDS
//   global  above           a block per row, N+(u) searched where it lies in col[]
//   The last three are one template: the team takes T out-neighbours v at a time, scans
//   their list lengths, and its lanes stream the concatenated lists N+(v) -- item t finds
//   its list by a search of the T + 1 scanned offsets in LDS, reads x = col[..] and
//   binary-searches x in N+(u).  Lanes stay busy whatever the mix of list lengths.
//
// Everything up to the row lists is tc_build (declared in lpa_internal.h), which lpa_scan.hip
// calls too -- there also with carry: the second sort takes every slot's index in the sorted
// canonical keys along as a payload.  tc_has / tc_pos and the teams' LDS layout are lpa_tc.h.
//
// count[] takes 64-bit integer atomic adds (they commute: every interleaving gives the
// same bits); the apex's share is summed in registers and across the team, one atomic
// per row.  Every offset and count is 64-bit; a vertex id is 32-bit.
#include "lpa_device.h"
#include "lpa_algo.h"
#include "lpa_tc.h"

namespace lpa {

namespace {

__global__ __launch_bounds__(256) void k_tc_compact(const u64* __restrict__ keys, const int32_t* __restrict__ first,
                                                    const int64_t* __restrict__ pos, int64_t m, u64* __restrict__ out) {
  GRID_STRIDE(i, m) {
    if (first[i]) out[pos[i]] = keys[i];
  }
}

__global__ __launch_bounds__(256) void k_tc_iota(u64* __restrict__ v, int64_t n) {
  GRID_STRIDE(i, n) v[i] = (u64)i;
}

// ek: the E simple edges, sorted.  A run of equal min endpoints inside a wave is one
// atomic (a hub of a million edges: 1 / 64 of the same-address adds).
__global__ __launch_bounds__(256) void k_tc_degrees(const u64* __restrict__ ek, int64_t E, int32_t* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  BLOCK_STRIDE(b, E) {
    const int64_t i = b + threadIdx.x;
    const bool act = i < E;
    const u64 k = act ? ek[i] : ~0ull;
    const u32 lo = (u32)(k >> 32);   // 0xFFFFFFFF on an idle lane: no vertex
    if (act) atomicAdd(&d[(u32)k], 1);
    const u32 prev = (u32)__shfl_up((int)lo, 1, 64);
    const bool head = act && (lane == 0 || prev != lo);
    const u64 heads = __ballot(head);
    const int nact = __popcll(__ballot(act));   // the active lanes are lanes [0, nact)
    if (head) {
      const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
      const int end = above ? lane + 1 + (__ffsll((ull)above) - 1) : nact;
      atomicAdd(&d[lo], end - lane);
    }
  }
}

// in place: (a << 32 | b), a < b  ->  (from << 32 | to), rank(from) < rank(to)
__global__ __launch_bounds__(256) void k_tc_orient(u64* __restrict__ ek, int64_t E, const int32_t* __restrict__ d,
                                                   int32_t* __restrict__ od) {
  GRID_STRIDE(i, E) {
    const u64 k = ek[i];
    const u32 a = (u32)(k >> 32), b = (u32)k;
    const bool fwd = d[a] <= d[b];   // equal degrees: a < b decides
    const u32 from = fwd ? a : b, to = fwd ? b : a;
    ek[i] = ((u64)from << 32) | to;
    atomicAdd(&od[from], 1);
  }
}

// Row lists of the four count forms (list k at lists + k * V, in no particular order:
// integer adds commute) and the longest out-list.  cnt[0..3] list lengths, cnt[4] max L.
__global__ __launch_bounds__(256) void k_tc_classify(const int32_t* __restrict__ od, int64_t V, int32_t short_max,
                                                     int32_t wave_max, int32_t lds_max, int32_t* __restrict__ lists,
                                                     u32* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const u64 lt = (1ull << lane) - 1ull;
  int32_t lmax = 0;
  BLOCK_STRIDE(b, V) {
    const int64_t v = b + threadIdx.x;
    const int32_t L = v < V ? od[v] : 0;
    const int f = L < 2 ? -1 : L <= short_max ? 0 : L <= wave_max ? 1 : L <= lds_max ? 2 : 3;
    lmax = L > lmax ? L : lmax;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u64 mk = __ballot(f == k);
      if (mk == 0ull) continue;   // uniform
      u32 base = 0;
      if (lane == 0) base = atomicAdd(&cnt[k], (u32)__popcll(mk));
      base = (u32)__builtin_amdgcn_readfirstlane((int)base);
      if (f == k) lists[(int64_t)k * V + base + __popcll(mk & lt)] = (int32_t)v;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int32_t o = __shfl_xor(lmax, off, 64);
    lmax = o > lmax ? o : lmax;
  }
  if (lane == 0 && lmax > 0) atomicMax(&cnt[4], (u32)lmax);
}

// G lanes per row (256 / G rows per block).  Items: the ordered pairs (v, w) of N+(u).
template <int G>
__global__ __launch_bounds__(256) void k_tc_group(const int32_t* __restrict__ rows, int64_t nrows,
                                                  const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                  ull* __restrict__ count) {
  constexpr int kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < nrows; base += (int64_t)gridDim.x * kRows) {
    const int64_t r = base + threadIdx.x / G;
    const bool act = r < nrows;
    ull cu = 0;
    int32_t u = 0;
    if (act) {
      u = rows[r];
      const int64_t ub = rp[u];
      const int64_t L = rp[u + 1] - ub;
      const int64_t n = L * (L - 1);
      for (int64_t t = sub; t < n; t += G) {
        const int64_t j = t / (L - 1);
        int64_t k = t - j * (L - 1);
        k += k >= j ? 1 : 0;
        const int32_t v = col[ub + j], w = col[ub + k];
        const int64_t vb = rp[v];
        if (tc_has(col + vb, (int32_t)(rp[v + 1] - vb), w)) {
          cu += 1;
          atomicAdd(&count[v], 1ull);
          atomicAdd(&count[w], 1ull);
        }
      }
    }
    // the G lanes of a row are neighbours: the row's sum ends in its lane 0
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) cu += __shfl_xor(cu, off, 64);
    if (act && sub == 0 && cu) atomicAdd(&count[u], cu);
  }
}

// A team of T lanes (a wave, or the block of 256) per row u.  kLds: N+(u) is staged in
// the team's LDS region (L <= cap); otherwise it is searched in col[] (any length).
template <int T, bool kLds>
__global__ __launch_bounds__(256) void k_tc_team(const int32_t* __restrict__ rows, int64_t nrows,
                                                 const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                 ull* __restrict__ count, int32_t cap) {
  static_assert(T == 64 || T == 256, "a wave or the block");
  extern __shared__ ull tc_smem[];
  __shared__ int32_t wsum[4];
  __shared__ ull wcu[4];
  constexpr int kTeams = 256 / T;
  const int team = threadIdx.x / T, tl = threadIdx.x % T, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  ull* region = tc_smem + (int64_t)team * tc_team_words<T>(kLds ? cap : 0);
  int64_t* rpv = reinterpret_cast<int64_t*>(region);
  int32_t* pre = reinterpret_cast<int32_t*>(region + T);
  int32_t* nu = pre + (T + 2);
  // T == 256: r is the same in every thread of the block (barriers inside)
  for (int64_t r = (int64_t)blockIdx.x * kTeams + team; r < nrows; r += (int64_t)gridDim.x * kTeams) {
    const int32_t u = rows[r];
    const int64_t ub = rp[u];
    const int32_t L = (int32_t)(rp[u + 1] - ub);
    const int32_t* __restrict__ gu = col + ub;
    if (kLds) {
      for (int32_t i = tl; i < L; i += T) nu[i] = gu[i];
      tc_team_sync<T>();
    }
    ull cu = 0;
    for (int32_t c0 = 0; c0 < L; c0 += T) {
      // this lane's out-neighbour of the chunk, and the scan of the chunk's list lengths
      int64_t vb = 0;
      int32_t len = 0;
      if (c0 + tl < L) {
        const int32_t v = kLds ? nu[c0 + tl] : gu[c0 + tl];
        vb = rp[v];
        len = (int32_t)(rp[v + 1] - vb);
      }
      int32_t incl = len;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
      }
      if (T == 256) {
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        for (int i = 0; i < w; ++i) incl += wsum[i];
      }
      rpv[tl] = vb;
      pre[tl] = incl - len;
      if (tl == T - 1) pre[T] = incl;
      tc_team_sync<T>();
      const int32_t total = pre[T];
      for (int32_t t = tl; t < total; t += T) {
        // the list of item t: the largest c with pre[c] <= t (empty lists share an offset
        // with their successor and are passed over)
        int32_t c = 0, hi = T;
        while (hi - c > 1) {
          const int32_t mid = (c + hi) >> 1;
          if (pre[mid] <= t) c = mid;
          else hi = mid;
        }
        const int32_t x = col[rpv[c] + (t - pre[c])];
        if (kLds ? tc_has(nu, L, x) : tc_has(gu, L, x)) {
          const int32_t v = kLds ? nu[c0 + c] : gu[c0 + c];
          cu += 1;
          atomicAdd(&count[v], 1ull);
          atomicAdd(&count[x], 1ull);
        }
      }
      tc_team_sync<T>();   // before the next chunk (or row) rewrites rpv / pre / nu
    }
    for (int off = 32; off > 0; off >>= 1) cu += __shfl_xor(cu, off, 64);
    if (T == 256) {
      if (lane == 0) wcu[w] = cu;
      __syncthreads();
      cu = wcu[0] + wcu[1] + wcu[2] + wcu[3];
      __syncthreads();
    }
    if (tl == 0 && cu) atomicAdd(&count[u], cu);
  }
}

__global__ __launch_bounds__(256) void k_tc_widen(const int32_t* __restrict__ a, int64_t n, int64_t* __restrict__ out) {
  GRID_STRIDE(i, n) out[i] = a[i];
}

// acc[0] sum of count, [1] vertices with count > 0, [2] max count, [3] wedges.  The count
// is a full 64-bit value, so the argmax is not packed beside it: k_tc_argmax follows.
__global__ __launch_bounds__(256) void k_tc_summary(const ull* __restrict__ count, const int32_t* __restrict__ d,
                                                    int64_t V, ull* __restrict__ acc) {
  __shared__ ull ws[4][4];
  ull sum = 0, nin = 0, best = 0, wed = 0;
  GRID_STRIDE(v, V) {
    const ull c = count[v], dv = (ull)d[v];
    sum += c;
    nin += c ? 1ull : 0ull;
    best = dev::umax64(best, c);
    wed += dv ? dv * (dv - 1ull) / 2ull : 0ull;
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off, 64);
    nin += __shfl_xor(nin, off, 64);
    wed += __shfl_xor(wed, off, 64);
    best = dev::umax64(best, __shfl_xor(best, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    ws[0][threadIdx.x >> 6] = sum;
    ws[1][threadIdx.x >> 6] = nin;
    ws[2][threadIdx.x >> 6] = best;
    ws[3][threadIdx.x >> 6] = wed;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
    nin = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
    best = dev::umax64(dev::umax64(ws[2][0], ws[2][1]), dev::umax64(ws[2][2], ws[2][3]));
    wed = ws[3][0] + ws[3][1] + ws[3][2] + ws[3][3];
    if (sum) atomicAdd(&acc[0], sum);
    if (nin) atomicAdd(&acc[1], nin);
    if (best) atomicMax(&acc[2], best);
    if (wed) atomicAdd(&acc[3], wed);
  }
}

// acc[4] (preset to ~0) = the smallest v with count[v] == acc[2] (final: the launch before)
__global__ __launch_bounds__(256) void k_tc_argmax(const ull* __restrict__ count, int64_t V, ull* __restrict__ acc) {
  __shared__ ull ws[4];
  const ull best = acc[2];
  ull id = ~0ull;
  GRID_STRIDE(v, V) {
    if (count[v] == best && (ull)v < id) id = (ull)v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const ull o = __shfl_xor(id, off, 64);
    id = o < id ? o : id;
  }
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = id;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) id = ws[i] < id ? ws[i] : id;
    if (id != ~0ull) atomicMin(&acc[4], id);
  }
}

template <int T, bool kLds>
int launch_team(const int32_t* rows, int64_t nrows, const int64_t* rp, const int32_t* col, ull* count, int32_t cap,
                hipStream_t s) {
  if (nrows == 0) return LPA_OK;
  const size_t bytes = sizeof(ull) * (size_t)((256 / T) * tc_team_words<T>(kLds ? cap : 0));
  if (bytes > (size_t)64 * 1024) {   // kTcWaveMax / kTcLdsMax keep every launch below
    set_error("triangle_count: %zu bytes of LDS per block", bytes);
    return LPA_EINVAL;
  }
  hipLaunchKernelGGL((k_tc_team<T, kLds>), dim3(grid_rows(nrows, 256 / T, 16384)), dim3(256), bytes, s, rows, nrows, rp,
                     col, count, cap);
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

}  // namespace

// d: [V], zeroed by the caller; filled with the simple degrees.  E == 0: no array but d.
int tc_build(lpa_graph* g, Tmp& tmp, int32_t* d, bool carry, TcLists* t) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  SimpleEdges se;
  LPA_TRY(simple_edges(g, tmp, &se));
  const int64_t E = t->E = se.E;
  u64* keys = se.keys;   // [2 m]: the sorted edge keys, then [m, m + E) the simple edges
  if (E == 0) return LPA_OK;
  const HalfShifts sh(bits_for((uint64_t)(V - 1)));
  u64* ek = t->ek = keys + m;
  hipLaunchKernelGGL(k_tc_compact, dim3(grid_for(m)), dim3(256), 0, s, keys, se.first, se.pos, m, ek);
  LPA_HIP(hipGetLastError());
  int32_t* od = nullptr;
  u32* cnt = nullptr;
  LPA_TRY(tmp.get(&od, V));
  LPA_TRY(tmp.get(&t->col, E));
  LPA_TRY(tmp.get(&t->rp, V + 1));
  LPA_TRY(tmp.get(&t->lists, 4 * V));
  LPA_TRY(tmp.get(&cnt, 8));
  LPA_HIP(hipMemsetAsync(od, 0, sizeof(int32_t) * (size_t)V, s));
  LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(u32) * 8, s));
  hipLaunchKernelGGL(k_tc_degrees, dim3(grid_for(E)), dim3(256), 0, s, ek, E, d);
  if (carry) {
    // the canonical keys stay (sorted: canonical edge i is ckeys[i]); the payload of slot i is i
    u64* tvals = nullptr;
    LPA_TRY(tmp.get(&t->ckeys, E));
    LPA_TRY(tmp.get(&t->canon, E));
    LPA_TRY(tmp.get(&tvals, E));
    LPA_HIP(hipMemcpyAsync(t->ckeys, ek, sizeof(u64) * (size_t)E, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_tc_iota, dim3(grid_for(E)), dim3(256), 0, s, t->canon, E);
    hipLaunchKernelGGL(k_tc_orient, dim3(grid_for(E)), dim3(256), 0, s, ek, E, d, od);
    LPA_HIP(hipGetLastError());
    LPA_TRY(radix_sort_u64_kv(ek, t->canon, keys, tvals, E, sh.both(), 2 * sh.ns, s));
    tmp.drop(tvals);
  } else {
    hipLaunchKernelGGL(k_tc_orient, dim3(grid_for(E)), dim3(256), 0, s, ek, E, d, od);
    LPA_HIP(hipGetLastError());
    LPA_TRY(radix_sort_u64(ek, keys, E, sh.both(), 2 * sh.ns, s));
  }
  LPA_TRY(key_col(ek, E, t->col, s));
  LPA_TRY(exclusive_scan_i32_i64(od, t->rp, V, s));
  hipLaunchKernelGGL(k_tc_classify, dim3(grid_bh(V)), dim3(256), 0, s, od, V, g->tc_short, g->tc_wave, g->tc_lds,
                     t->lists, cnt);
  LPA_HIP(hipGetLastError());
  u32 h[8] = {0};
  LPA_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < 4; ++k) t->rows[k] = h[k];
  t->lmax = (int32_t)h[4];
  return LPA_OK;
}

// Reads V, m, e_src / e_dst, the stream and the tc_* boundaries of the handle, nothing of
// the LPA state; every array is a stream-ordered temporary.
int triangle_count(lpa_graph* g, int64_t* count_out, int64_t* simple_degree_out, int32_t out_is_device,
                   lpa_triangle_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V;
  if (summary) *summary = lpa_triangle_summary{0, 0, 0, 0, 0, -1};
  if (V == 0) return LPA_OK;
  Tmp tmp(s);
  ull* count = reinterpret_cast<ull*>(count_out);
  int32_t* d = nullptr;
  if (!out_is_device) LPA_TRY(tmp.get(&count, V));
  LPA_TRY(tmp.get(&d, V));
  LPA_HIP(hipMemsetAsync(count, 0, sizeof(ull) * (size_t)V, s));
  LPA_HIP(hipMemsetAsync(d, 0, sizeof(int32_t) * (size_t)V, s));
  TcLists t;
  LPA_TRY(tc_build(g, tmp, d, false, &t));
  const int64_t E = t.E;
  if (E > 0) {
    const int32_t* lists = t.lists;
    const int64_t* rp = t.rp;
    const int32_t* col = t.col;
    const int32_t lmax = t.lmax;
    if (t.rows[0]) {
      hipLaunchKernelGGL(k_tc_group<8>, dim3(grid_rows(t.rows[0], 32, 16384)), dim3(256), 0, s, lists,
                         (int64_t)t.rows[0], rp, col, count);
      LPA_HIP(hipGetLastError());
    }
    LPA_TRY((launch_team<64, true>(lists + V, t.rows[1], rp, col, count, lmax < g->tc_wave ? lmax : g->tc_wave, s)));
    LPA_TRY((launch_team<256, true>(lists + 2 * V, t.rows[2], rp, col, count, lmax < g->tc_lds ? lmax : g->tc_lds, s)));
    LPA_TRY((launch_team<256, false>(lists + 3 * V, t.rows[3], rp, col, count, 0, s)));
  }
  ull h[5] = {0, 0, 0, 0, 0};
  if (summary) {
    ull* acc = nullptr;
    LPA_TRY(tmp.get(&acc, 5));
    LPA_HIP(hipMemsetAsync(acc, 0, sizeof(ull) * 4, s));
    LPA_HIP(hipMemsetAsync(acc + 4, 0xFF, sizeof(ull), s));
    hipLaunchKernelGGL(k_tc_summary, dim3(grid_bh(V)), dim3(256), 0, s, count, d, V, acc);
    hipLaunchKernelGGL(k_tc_argmax, dim3(grid_bh(V)), dim3(256), 0, s, count, V, acc);
    LPA_HIP(hipGetLastError());
    LPA_HIP(hipMemcpyAsync(h, acc, sizeof(h), hipMemcpyDeviceToHost, s));
  }
  if (simple_degree_out) {
    int64_t* dw = simple_degree_out;
    if (!out_is_device) LPA_TRY(tmp.get(&dw, V));
    hipLaunchKernelGGL(k_tc_widen, dim3(grid_for(V)), dim3(256), 0, s, d, V, dw);
    LPA_HIP(hipGetLastError());
    if (!out_is_device)
      LPA_HIP(hipMemcpyAsync(simple_degree_out, dw, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  }
  if (!out_is_device)
    LPA_HIP(hipMemcpyAsync(count_out, count, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->n_triangles = (int64_t)(h[0] / 3ull);
    summary->simple_edges = E;
    summary->wedges = (int64_t)h[3];
    summary->n_in_triangle = (int64_t)h[1];
    summary->max_count = (int64_t)h[2];
    summary->max_count_id = (int64_t)h[4];
  }
  return LPA_OK;
}

}  // namespace lpa
