// The edge-list builds that the algorithm calls share, and the kernels around them.
//
// Directed arcs (arcs_count / arcs_lists: lpa_sp.hip, lpa_scc.hip, lpa_bfs.hip): the distinct non-loop
// arcs of the input graph, as out-lists and in-lists.
//   keys     (src << 32 | dst) of every in-range non-loop edge; anything else gets
//            (V << 32 | V) and sorts behind every vertex, and so does an edge that the
//            caller's keep mask (lpa_bfs.hip; null: every edge is kept) leaves out.  The
//            halves hold values up to V: bits_for(V) bits a half
//   sort     radix sort over both halves; a key that differs from its predecessor is kept
//            (flag byte, u32 scan): E distinct arcs in (src, dst) order, E read on the host
//   out      compaction; oo[u] = the first arc with source >= u (a binary search per
//            vertex), ocol[i] = the low half
//   in       the halves swapped and sorted again by the new high half alone (the sort is
//            stable: sources stay ascending inside a row); io[v], icol[i] alike.
//            Offsets int64, ids int32
//
// Simple edges (simple_edges: lpa_tc.hip, lpa_kcore.hip): the canonical simple undirected
// graph (no self-loops, no direction, duplicates collapsed).
//   keys     (min << 32 | max) of every edge; an id outside [0, V) makes the edge a loop
//            (key 0: dropped).  The halves hold ids: bits_for(V - 1) bits a half
//   sort     radix sort over both halves; the first key of each run with min != max is a
//            simple edge (int32 mark, int64 scan): E of them, read on the host
// The two families keep their own sentinel, pass count and scan type: at V = 2^8, 2^16 and
// 2^24 bits_for(V) takes one more pass a half than bits_for(V - 1).
//
// Edge rows (edge_lists: lpa_motif.hip): every in-range edge row of the MULTIGRAPH, self-loops and
// duplicates kept, as out-lists and in-lists that carry the row's index in the input.
//   keys     (src << 32 | dst), anything else (V << 32 | V); the payload is the edge row
//   sort     radix sort with the payload over both halves.  LSD and stable, the payload in
//            input order: rows of one (src, dst) stay in edge-row order and no digit is spent
//            on the row.  oo[] by binary search (oo[V] = the valid rows), ocol[] the low half,
//            oeid[] the payload
//   in       the halves swapped, sorted again by the new high half alone: (dst, src, row)
//
// Also here, once: the bounds binary search, the low half as col[], the pull-form row lists
// (form_lists) and the component sizes and summary of lpa_cc.hip and lpa_scc.hip.
#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

namespace {

// ---- directed arcs ----
// kLoops: loop[a] = 1 for every in-range self-loop (plain byte stores)
// kKeep: an edge with keep[i] == 0 is no edge (nor a loop)
template <bool kLoops, bool kKeep>
__global__ __launch_bounds__(256) void k_arc_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                  int64_t m, u32 V, u64* __restrict__ keys,
                                                  uint8_t* __restrict__ loop, const uint8_t* __restrict__ keep) {
  GRID_STRIDE(i, m) {
    const u32 a = (u32)__builtin_nontemporal_load(src + i), b = (u32)__builtin_nontemporal_load(dst + i);
    const bool kept = !kKeep || keep[i] != 0;
    keys[i] = kept && a < V && b < V && a != b ? ((u64)a << 32) | b : ((u64)V << 32) | V;
    if (kLoops && kept && a == b && a < V) loop[a] = 1;
  }
}

// keys ascending: flag[i] = key i is an arc and the first of its value
__global__ __launch_bounds__(256) void k_arc_uniq(const u64* __restrict__ keys, int64_t m, u32 V,
                                                  uint8_t* __restrict__ flag) {
  GRID_STRIDE(i, m) {
    const u64 k = keys[i];
    flag[i] = (u32)(k >> 32) < V && (i == 0 || keys[i - 1] != k) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_arc_compact(const u64* __restrict__ keys, const uint8_t* __restrict__ flag,
                                                     const u32* __restrict__ pos, int64_t m, u64* __restrict__ out) {
  GRID_STRIDE(i, m) {
    if (flag[i]) out[pos[i]] = keys[i];
  }
}

// the arcs in (src, dst) order: the out-list columns, and the keys with their halves swapped
__global__ __launch_bounds__(256) void k_arc_split(const u64* __restrict__ okeys, int64_t E, int32_t* __restrict__ ocol,
                                                   u64* __restrict__ tkeys) {
  GRID_STRIDE(i, E) {
    const u64 k = okeys[i];
    ocol[i] = (int32_t)(u32)k;
    tkeys[i] = (k << 32) | (k >> 32);
  }
}

// both orientations of every in-range non-loop edge (lpa_bc.hip, undirected): 2 m keys
__global__ __launch_bounds__(256) void k_arc_keys_both(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                       int64_t m, u32 V, u64* __restrict__ keys) {
  GRID_STRIDE(i, m) {
    const u32 a = (u32)__builtin_nontemporal_load(src + i), b = (u32)__builtin_nontemporal_load(dst + i);
    const bool arc = a < V && b < V && a != b;
    keys[i] = arc ? ((u64)a << 32) | b : ((u64)V << 32) | V;
    keys[m + i] = arc ? ((u64)b << 32) | a : ((u64)V << 32) | V;
  }
}

// ---- simple edges ----
__global__ __launch_bounds__(256) void k_edge_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                   int64_t m, u32 V, u64* __restrict__ keys) {
  GRID_STRIDE(i, m) {
    const u32 a = (u32)__builtin_nontemporal_load(src + i), b = (u32)__builtin_nontemporal_load(dst + i);
    const u32 lo = a < b ? a : b, hi = a < b ? b : a;
    keys[i] = hi < V ? ((u64)lo << 32) | hi : 0ull;
  }
}

__global__ __launch_bounds__(256) void k_edge_mark(const u64* __restrict__ keys, int64_t m,
                                                   int32_t* __restrict__ first) {
  GRID_STRIDE(i, m) {
    const u64 k = keys[i];
    first[i] = ((u32)(k >> 32) != (u32)k && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
  }
}

// ---- edge rows (the multigraph) ----
// keys[i] = (src << 32 | dst) of an in-range edge row, loops and duplicates kept; anything else
// gets (V << 32 | V).  vals[i] = i, the payload the sort carries
__global__ __launch_bounds__(256) void k_edge_row_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                       int64_t m, u32 V, u64* __restrict__ keys,
                                                       u64* __restrict__ vals) {
  GRID_STRIDE(i, m) {
    const u32 a = (u32)__builtin_nontemporal_load(src + i), b = (u32)__builtin_nontemporal_load(dst + i);
    keys[i] = a < V && b < V ? ((u64)a << 32) | b : ((u64)V << 32) | V;
    vals[i] = (u64)i;
  }
}

// the halves of every key swapped in place, the payload copied beside it
__global__ __launch_bounds__(256) void k_edge_row_swap(u64* __restrict__ keys, const u64* __restrict__ vals, int64_t m,
                                                       u64* __restrict__ ivals) {
  GRID_STRIDE(i, m) {
    const u64 k = keys[i];
    keys[i] = (k << 32) | (k >> 32);
    ivals[i] = vals[i];
  }
}

// ---- shared ----
// keys ascending in the half at kShift (0: the low half, 32: the high half).  out[v], v in
// [0, V]: the first position whose half is >= v
template <int kShift>
__global__ __launch_bounds__(256) void k_key_bounds(const u64* __restrict__ keys, int64_t n, int64_t V,
                                                    int64_t* __restrict__ out) {
  GRID_STRIDE(v, V + 1) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)(u32)(keys[mid] >> kShift) < v) lo = mid + 1;
      else hi = mid;
    }
    out[v] = lo;
  }
}

__global__ __launch_bounds__(256) void k_key_col(const u64* __restrict__ keys, int64_t n, int32_t* __restrict__ col) {
  GRID_STRIDE(i, n) col[i] = (int32_t)(u32)keys[i];
}

// a row's form by its list length L (fw: a wave row, fb: a block row; neither: a short row)
__global__ __launch_bounds__(256) void k_forms(const int64_t* __restrict__ off, int64_t V, int64_t short_max,
                                               int64_t wave_max, uint8_t* __restrict__ fw, uint8_t* __restrict__ fb) {
  GRID_STRIDE(v, V) {
    const int64_t L = off[v + 1] - off[v];
    fw[v] = L > short_max && L <= wave_max ? 1 : 0;
    fb[v] = L > short_max && L > wave_max ? 1 : 0;
  }
}

// the flagged rows at their scanned positions: the wave rows in lists, the block rows in lists + V
__global__ __launch_bounds__(256) void k_form_lists(const uint8_t* __restrict__ fw, const uint8_t* __restrict__ fb,
                                                    const u32* __restrict__ pw, const u32* __restrict__ pb, int64_t V,
                                                    int32_t* __restrict__ lists) {
  GRID_STRIDE(v, V) {
    if (fw[v]) lists[pw[v]] = (int32_t)v;
    if (fb[v]) lists[V + pb[v]] = (int32_t)v;
  }
}

// ---- component sizes and summary (comp[c] == c at every value c of comp) ----
// size[c] += 1 for every member; block-aggregated (the giant component is one counter)
__global__ __launch_bounds__(256) void k_comp_sizes(const int32_t* __restrict__ comp, int64_t V,
                                                    ull* __restrict__ size) {
  __shared__ u32 bk[dev::kBhSlots];
  __shared__ ull bv[dev::kBhSlots];
  __shared__ int bsat;
  dev::BlockHist<ull> bh{bk, bv, &bsat};
  bh.init();
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x; b < V; b += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = b + threadIdx.x;
    const bool act = v < V;
    bh.add1(size, act, act ? (u32)comp[v] : 0u, lane);
  }
  bh.flush(size);
}

// acc[0] components, [1] singletons, [2] max of (size << 32 | 0xFFFFFFFF - id): the largest
// component, the smallest id among equals
__global__ __launch_bounds__(256) void k_comp_summary(const int32_t* __restrict__ comp, const ull* __restrict__ size,
                                                      int64_t V, ull* __restrict__ acc) {
  __shared__ ull ws[3][4];
  ull n = 0, n1 = 0, best = 0;
  GRID_STRIDE(v, V) {
    if (comp[v] == (int32_t)v) {
      const ull sz = size[v];
      n += 1;
      n1 += sz == 1ull ? 1ull : 0ull;
      best = dev::umax64(best, (sz << 32) | (ull)(0xFFFFFFFFu - (u32)v));
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    n += __shfl_xor(n, off, 64);
    n1 += __shfl_xor(n1, off, 64);
    best = dev::umax64(best, __shfl_xor(best, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    ws[0][threadIdx.x >> 6] = n;
    ws[1][threadIdx.x >> 6] = n1;
    ws[2][threadIdx.x >> 6] = best;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    n = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
    n1 = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
    best = dev::umax64(dev::umax64(ws[2][0], ws[2][1]), dev::umax64(ws[2][2], ws[2][3]));
    if (n) atomicAdd(&acc[0], n);
    if (n1) atomicAdd(&acc[1], n1);
    if (best) atomicMax(&acc[2], best);
  }
}

}  // namespace

int key_bounds(const u64* keys, int64_t n, int64_t V, bool high_half, int64_t* out, hipStream_t s) {
  if (high_half) hipLaunchKernelGGL(k_key_bounds<32>, dim3(grid_for(V + 1)), dim3(256), 0, s, keys, n, V, out);
  else hipLaunchKernelGGL(k_key_bounds<0>, dim3(grid_for(V + 1)), dim3(256), 0, s, keys, n, V, out);
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

int key_col(const u64* keys, int64_t n, int32_t* col, hipStream_t s) {
  hipLaunchKernelGGL(k_key_col, dim3(grid_for(n)), dim3(256), 0, s, keys, n, col);
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

int arcs_count(lpa_graph* g, Tmp& tmp, uint8_t* loop, ArcLists* a, const uint8_t* keep, bool both) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = both ? 2 * g->m : g->m;   // m: the keys
  a->E = 0;
  a->n = m;
  if (m == 0) return LPA_OK;
  if (m >= (int64_t)1 << 32) {
    set_error("%lld arc keys do not fit the 32-bit positions of the arc build", (long long)m);
    return LPA_EOVERFLOW;
  }
  const HalfShifts sh(bits_for((uint64_t)V));   // the halves hold values up to V (a dropped edge)
  LPA_TRY(tmp.get(&a->keys, 2 * m));
  LPA_TRY(tmp.get(&a->flag, m));
  LPA_TRY(tmp.get(&a->pos, m + 1));
  u64* keys = a->keys;
  auto* k_keys = loop ? (keep ? k_arc_keys<true, true> : k_arc_keys<true, false>)
                      : (keep ? k_arc_keys<false, true> : k_arc_keys<false, false>);
  if (both)   // no loop marks, no keep mask
    hipLaunchKernelGGL(k_arc_keys_both, dim3(grid_for(g->m)), dim3(256), 0, s, g->e_src, g->e_dst, g->m, (u32)V, keys);
  else
    hipLaunchKernelGGL(k_keys, dim3(grid_for(m)), dim3(256), 0, s, g->e_src, g->e_dst, m, (u32)V, keys, loop, keep);
  LPA_HIP(hipGetLastError());
  LPA_TRY(radix_sort_u64(keys, keys + m, m, sh.both(), 2 * sh.ns, s));
  hipLaunchKernelGGL(k_arc_uniq, dim3(grid_for(m)), dim3(256), 0, s, keys, m, (u32)V, a->flag);
  LPA_HIP(hipGetLastError());
  LPA_TRY(exclusive_scan_u8_u32(a->flag, a->pos, m, s));
  u32 hE = 0;
  LPA_HIP(hipMemcpyAsync(&hE, a->pos + m, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  a->E = (int64_t)hE;
  return LPA_OK;
}

int arcs_lists(lpa_graph* g, Tmp& tmp, ArcLists* a) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = a->n, E = a->E;
  LPA_TRY(tmp.get(&a->oo, V + 1));
  LPA_TRY(tmp.get(&a->io, V + 1));
  LPA_TRY(tmp.get(&a->ocol, E));
  LPA_TRY(tmp.get(&a->icol, E));
  if (E > 0) {
    const HalfShifts sh(bits_for((uint64_t)V));
    u64* keys = a->keys;
    u64* okeys = keys + m;   // the arcs in (src, dst) order; then the second sort's other buffer
    hipLaunchKernelGGL(k_arc_compact, dim3(grid_for(m)), dim3(256), 0, s, keys, a->flag, a->pos, m, okeys);
    hipLaunchKernelGGL(k_arc_split, dim3(grid_for(E)), dim3(256), 0, s, okeys, E, a->ocol, keys);
    LPA_TRY(key_bounds(okeys, E, V, true, a->oo, s));
    LPA_TRY(radix_sort_u64(keys, okeys, E, sh.hi(), sh.ns, s));
    LPA_TRY(key_bounds(keys, E, V, true, a->io, s));
    LPA_TRY(key_col(keys, E, a->icol, s));
  } else {
    LPA_HIP(hipMemsetAsync(a->oo, 0, sizeof(int64_t) * (size_t)(V + 1), s));
    LPA_HIP(hipMemsetAsync(a->io, 0, sizeof(int64_t) * (size_t)(V + 1), s));
  }
  return LPA_OK;
}

int edge_lists(lpa_graph* g, Tmp& tmp, bool want_in, EdgeLists* l) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  l->mv = 0;
  LPA_TRY(tmp.get(&l->oo, V + 1));
  if (want_in) LPA_TRY(tmp.get(&l->io, V + 1));
  if (m == 0) {
    LPA_HIP(hipMemsetAsync(l->oo, 0, sizeof(int64_t) * (size_t)(V + 1), s));
    if (want_in) LPA_HIP(hipMemsetAsync(l->io, 0, sizeof(int64_t) * (size_t)(V + 1), s));
    return LPA_OK;
  }
  const HalfShifts sh(bits_for((uint64_t)V));   // the halves hold values up to V (a dropped edge)
  u64 *keys = nullptr, *vals = nullptr, *tk = nullptr, *tv = nullptr;
  LPA_TRY(tmp.get(&keys, m));
  LPA_TRY(tmp.get(&vals, m));
  LPA_TRY(tmp.get(&tk, m));
  LPA_TRY(tmp.get(&tv, m));
  LPA_TRY(tmp.get(&l->ocol, m));
  hipLaunchKernelGGL(k_edge_row_keys, dim3(grid_for(m)), dim3(256), 0, s, g->e_src, g->e_dst, m, (u32)V, keys, vals);
  LPA_HIP(hipGetLastError());
  // stable, the payload in input order: equal (src, dst) keep their edge rows ascending
  LPA_TRY(radix_sort_u64_kv(keys, vals, tk, tv, m, sh.both(), 2 * sh.ns, s));
  LPA_TRY(key_bounds(keys, m, V, true, l->oo, s));   // oo[V] = the valid rows: a dropped edge sorts behind them
  LPA_TRY(key_col(keys, m, l->ocol, s));
  l->oeid = reinterpret_cast<int64_t*>(vals);
  if (want_in) {
    u64* ivals = nullptr;
    LPA_TRY(tmp.get(&ivals, m));
    LPA_TRY(tmp.get(&l->icol, m));
    hipLaunchKernelGGL(k_edge_row_swap, dim3(grid_for(m)), dim3(256), 0, s, keys, vals, m, ivals);
    LPA_HIP(hipGetLastError());
    // by the new high half alone: (src, edge row) stays ascending inside a destination
    LPA_TRY(radix_sort_u64_kv(keys, ivals, tk, tv, m, sh.hi(), sh.ns, s));
    LPA_TRY(key_bounds(keys, m, V, true, l->io, s));
    LPA_TRY(key_col(keys, m, l->icol, s));
    l->ieid = reinterpret_cast<int64_t*>(ivals);
  }
  tmp.drop(tv);
  tmp.drop(tk);
  tmp.drop(keys);
  LPA_HIP(hipMemcpyAsync(&l->mv, l->oo + V, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  return LPA_OK;
}

int fill_form_lists(const uint8_t* fw, const uint8_t* fb, const u32* pw, const u32* pb, int64_t V, int32_t* lists,
                    hipStream_t s) {
  hipLaunchKernelGGL(k_form_lists, dim3(grid_for(V)), dim3(256), 0, s, fw, fb, pw, pb, V, lists);
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

int form_lists(Tmp& tmp, const int64_t* off, int64_t V, int64_t short_max, int64_t wave_max, int32_t** lists,
               u32* n_rows) {
  hipStream_t s = tmp.s;
  uint8_t *fw = nullptr, *fb = nullptr;
  u32 *pw = nullptr, *pb = nullptr;
  LPA_TRY(tmp.get(&fw, V));
  LPA_TRY(tmp.get(&fb, V));
  LPA_TRY(tmp.get(&pw, V + 1));
  LPA_TRY(tmp.get(&pb, V + 1));
  LPA_TRY(tmp.get(lists, 2 * V));
  hipLaunchKernelGGL(k_forms, dim3(grid_for(V)), dim3(256), 0, s, off, V, short_max, wave_max, fw, fb);
  LPA_HIP(hipGetLastError());
  LPA_TRY(exclusive_scan_u8_u32(fw, pw, V, s));
  LPA_TRY(exclusive_scan_u8_u32(fb, pb, V, s));
  LPA_TRY(fill_form_lists(fw, fb, pw, pb, V, *lists, s));
  LPA_HIP(hipMemcpyAsync(&n_rows[0], pw + V, sizeof(u32), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(&n_rows[1], pb + V, sizeof(u32), hipMemcpyDeviceToHost, s));
  return LPA_OK;
}

int simple_edges(lpa_graph* g, Tmp& tmp, SimpleEdges* e) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  e->E = 0;
  if (m == 0) return LPA_OK;
  const HalfShifts sh(bits_for((uint64_t)(V - 1)));   // the halves hold ids
  LPA_TRY(tmp.get(&e->keys, 2 * m));
  LPA_TRY(tmp.get(&e->first, m));
  LPA_TRY(tmp.get(&e->pos, m + 1));
  hipLaunchKernelGGL(k_edge_keys, dim3(grid_for(m)), dim3(256), 0, s, g->e_src, g->e_dst, m, (u32)V, e->keys);
  LPA_HIP(hipGetLastError());
  LPA_TRY(radix_sort_u64(e->keys, e->keys + m, m, sh.both(), 2 * sh.ns, s));
  hipLaunchKernelGGL(k_edge_mark, dim3(grid_for(m)), dim3(256), 0, s, e->keys, m, e->first);
  LPA_HIP(hipGetLastError());
  LPA_TRY(exclusive_scan_i32_i64(e->first, e->pos, m, s));
  LPA_HIP(hipMemcpyAsync(&e->E, e->pos + m, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  return LPA_OK;
}

int comp_sizes(Tmp& tmp, const int32_t* comp, int64_t V, int64_t* size_out, int32_t out_is_device, bool summary,
               ull** size, ull* h) {
  hipStream_t s = tmp.s;
  *size = reinterpret_cast<ull*>(size_out);
  if (!size_out || !out_is_device) LPA_TRY(tmp.get(size, V));
  LPA_HIP(hipMemsetAsync(*size, 0, sizeof(ull) * (size_t)V, s));
  hipLaunchKernelGGL(k_comp_sizes, dim3(grid_bh(V)), dim3(256), 0, s, comp, V, *size);
  LPA_HIP(hipGetLastError());
  if (summary) {
    ull* acc = nullptr;
    LPA_TRY(tmp.get(&acc, 3));
    LPA_HIP(hipMemsetAsync(acc, 0, sizeof(ull) * 3, s));
    hipLaunchKernelGGL(k_comp_summary, dim3(grid_bh(V)), dim3(256), 0, s, comp, *size, V, acc);
    LPA_HIP(hipGetLastError());
    LPA_HIP(hipMemcpyAsync(h, acc, sizeof(ull) * 3, hipMemcpyDeviceToHost, s));
  }
  return LPA_OK;
}

}  // namespace lpa
