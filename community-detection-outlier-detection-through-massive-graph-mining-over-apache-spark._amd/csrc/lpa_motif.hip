// Motif finding (GraphFrame.find): every assignment of vertices to the pattern's vertex variables
// and of INPUT EDGE ROWS to its positive terms such that every positive term's edge goes from
// its src variable's vertex to its dst variable's vertex and no negated term has an edge.  A
// homomorphism over the multigraph: variables need not differ, a duplicate edge row is one more
// row, a self-loop is an edge.  Integers throughout, row counts and offsets int64.
//
// The table of partial matches is column-wise: one int32 column per live vertex variable, one
// int64 column per positive term whose edge row is wanted.  A column is carried only while a
// later term or the output still reads it; an anonymous edge multiplies rows and has no
// column.  The terms run in the caller's order:
//
//   seed     the first term: flag per input edge row (in range; a self-loop when src_var ==
//            dst_var), int64 scan, the flagged rows written in edge-row order.  The valid rows
//            and the self-loops are counted here, block-reduced
//   lists    edge_lists (lpa_adj.hip), only when a second term follows: out-lists sorted by
//            (src, dst, edge row); in-lists by (dst, src, edge row) only for an extend-in
//   step     per later positive term, one of
//              extend-out  src bound, dst new: count = the out-list length of the bound vertex
//              extend-in   dst bound, src new: count = the in-list length
//              close       both bound: count = the equal range of dst in src's out-list (two
//                          binary searches); 0 drops the row, k > 1 multiplies it
//            then exclusive_scan_i64 of the counts, the total read on the host (the step's one
//            synchronisation), the cap checked, the child table allocated, and the fill
//   negate   a negated term: count = 1 where the equal range is empty, else 0; the same scan
//            and the same fill, which then is a compaction in order
//   fill     one child row per lane.  A block owns 2048 consecutive child rows: two threads
//            find the parents of its first and last row in the scanned offsets, every lane then
//            searches only between them (off[p] <= j < off[p + 1]), gathers the parent's live
//            columns and appends lists[start[p] + j - off[p]].  Every column write is
//            coalesced; a parent with 10^5 children is spread over 49 blocks like any other
//            stretch of rows, and its lanes read one parent row (a broadcast)
//
// Order.  The seed is in edge-row order; children of a parent are written in list order and
// parents keep their order (child j of parent p sits at off[p] + j, off ascending).  The lists
// are a function of (V, edge list): the sort is stable and the payload is the edge row.  So
// every table, row for row, is a function of (V, edge list, terms) alone: no atomics decide a
// position, and a count is a sum in a fixed tree.  Identical across runs and handles.
//
// Memory.  One allocation per table (the int64 columns first, then the int32 ones); the parent
// is released in stream order after the fill that read it.  count_only never fills the last
// table: its row count is the last scan's total.  The final table of a call that returns rows
// is plain device memory (hipMalloc, not the stream's pool) that the last fill writes straight
// into and the result object owns: nothing of the handle, so it outlives it, and a column goes
// to the host in one copy.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

namespace {

constexpr int kMotifVCols = 9;      // 8 positive terms bind at most 9 vertex variables
constexpr int kMotifECols = 8;
constexpr int kFillTile = 2048;     // child rows a block of the fill owns at a time
constexpr int kMaxVars = 32;

enum { M_EXTEND = 0, M_CLOSE = 1, M_NEGATE = 2 };
// slots of the counters the seed leaves
enum { S_VALID = 0, S_LOOPS = 1, S_LEN = 2 };

__device__ __forceinline__ ull motif_wave_add(ull x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// ---- seed ----
// cnt[e] = edge row e seeds a table row; acc[S_VALID] += the in-range rows, acc[S_LOOPS] += the
// self-loops among them
__global__ __launch_bounds__(256) void k_motif_seed_count(const int32_t* __restrict__ src,
                                                          const int32_t* __restrict__ dst, int64_t m, u32 V,
                                                          int loops_only, int64_t* __restrict__ cnt,
                                                          ull* __restrict__ acc) {
  __shared__ ull ws[2][4];
  ull nv = 0, nl = 0;
  GRID_STRIDE(e, m) {
    const u32 a = (u32)src[e], b = (u32)dst[e];
    const bool valid = a < V && b < V, loop = valid && a == b;
    cnt[e] = (loops_only ? loop : valid) ? 1 : 0;
    nv += valid ? 1 : 0;
    nl += loop ? 1 : 0;
  }
  nv = motif_wave_add(nv);
  nl = motif_wave_add(nl);
  if ((threadIdx.x & 63) == 0) {
    ws[0][threadIdx.x >> 6] = nv;
    ws[1][threadIdx.x >> 6] = nl;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const ull x = ws[threadIdx.x][0] + ws[threadIdx.x][1] + ws[threadIdx.x][2] + ws[threadIdx.x][3];
    if (x) atomicAdd(&acc[threadIdx.x], x);
  }
}

// the flagged edge rows at their scanned positions (off[e + 1] > off[e]: flagged); a null column is not kept
__global__ __launch_bounds__(256) void k_motif_seed_fill(const int32_t* __restrict__ src,
                                                         const int32_t* __restrict__ dst,
                                                         const int64_t* __restrict__ off, int64_t m,
                                                         int32_t* __restrict__ va, int32_t* __restrict__ vb,
                                                         int64_t* __restrict__ ve) {
  GRID_STRIDE(e, m) {
    const int64_t j = off[e];
    if (off[e + 1] == j) continue;
    if (va) va[j] = src[e];
    if (vb) vb[j] = dst[e];
    if (ve) ve[j] = e;
  }
}

// ---- counts ----
// the first position in col[lo, hi) (ascending) whose entry is >= w (kUpper: > w)
template <bool kUpper>
__device__ __forceinline__ int64_t motif_bound(const int32_t* __restrict__ col, int64_t lo, int64_t hi, int32_t w) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t x = col[mid];
    if (kUpper ? x <= w : x < w) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// a lane per table row.  M_EXTEND: a = the bound column, loff its lists' offsets: every entry
// of the list.  M_CLOSE: a = src, b = dst, loff / lcol the out-lists: the equal range of b.
// M_NEGATE: 1 where that range is empty
template <int kMode>
__global__ __launch_bounds__(256) void k_motif_count(const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                     int64_t n, const int64_t* __restrict__ loff,
                                                     const int32_t* __restrict__ lcol, int64_t* __restrict__ cnt,
                                                     int64_t* __restrict__ start) {
  GRID_STRIDE(r, n) {
    const int64_t u = a[r];
    const int64_t s = loff[u], e = loff[u + 1];
    if (kMode == M_EXTEND) {
      cnt[r] = e - s;
      start[r] = s;
    } else {
      const int32_t w = b[r];
      const int64_t lo = motif_bound<false>(lcol, s, e, w);
      if (kMode == M_NEGATE) {
        cnt[r] = lo < e && lcol[lo] == w ? 0 : 1;
      } else {
        cnt[r] = motif_bound<true>(lcol, lo, e, w) - lo;
        start[r] = lo;
      }
    }
  }
}

// ---- fill ----
struct FillArgs {
  const int64_t* off;     // [n_parent + 1] the scanned counts
  const int64_t* start;   // [n_parent] a parent's first list position (null: a compaction)
  int64_t n_parent, total;
  int nv, ne;             // columns gathered from the parent
  const int32_t* vs[kMotifVCols];
  int32_t* vd[kMotifVCols];
  const int64_t* es[kMotifECols];
  int64_t* ed[kMotifECols];
  const int32_t* lcol;    // the lists (null with start)
  const int64_t* leid;
  int32_t* newv;          // the new vertex column (nullable)
  int64_t* newe;          // the new edge column (nullable)
};

// the parent of child row j: the last p in [lo, hi] with off[p] <= j (off[lo] <= j is given).
// Parents without children repeat their offset and are stepped over
__device__ __forceinline__ int64_t motif_parent(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t j) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// child row j = the k-th child of parent p: the parent's kept columns, then the list entry
__device__ __forceinline__ void motif_child(const FillArgs& a, int64_t p, int64_t j, int64_t k) {
#pragma unroll
  for (int c = 0; c < kMotifVCols; ++c)
    if (c < a.nv) a.vd[c][j] = a.vs[c][p];
#pragma unroll
  for (int c = 0; c < kMotifECols; ++c)
    if (c < a.ne) a.ed[c][j] = a.es[c][p];
  if (a.start) {
    const int64_t pos = a.start[p] + k;
    if (a.newv) a.newv[j] = a.lcol[pos];
    if (a.newe) a.newe[j] = a.leid[pos];
  }
}

// a lane per child row, a block per kFillTile consecutive ones: the block's parents lie between
// those of its first and last row, found once by two threads
__global__ __launch_bounds__(256) void k_motif_fill(const FillArgs a) {
  __shared__ int64_t range[2];
  const int64_t tiles = (a.total + kFillTile - 1) / kFillTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // t is the same in every thread: barriers inside
    const int64_t j0 = t * kFillTile;
    const int64_t j1 = j0 + kFillTile < a.total ? j0 + kFillTile : a.total;
    if (threadIdx.x == 0) range[0] = motif_parent(a.off, 0, a.n_parent - 1, j0);
    if (threadIdx.x == 64) range[1] = motif_parent(a.off, 0, a.n_parent - 1, j1 - 1);
    __syncthreads();
    const int64_t plo = range[0], phi = range[1];
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
      const int64_t p = motif_parent(a.off, plo, phi, j);
      motif_child(a, p, j, j - a.off[p]);
    }
    __syncthreads();   // before the next tile rewrites range
  }
}

// ---- host ----
// a table: n rows, its columns in one allocation (the int64 ones first)
struct Table {
  int64_t n = 0;
  int nv = 0, ne = 0;
  int vvar[kMotifVCols] = {};
  int32_t* v[kMotifVCols] = {};
  int eterm[kMotifECols] = {};
  int64_t* e[kMotifECols] = {};
  uint8_t* slab = nullptr;
  int32_t* vcol(int var) const {
    for (int i = 0; i < nv; ++i)
      if (vvar[i] == var) return v[i];
    return nullptr;
  }
  int64_t* ecol(int term) const {
    for (int i = 0; i < ne; ++i)
      if (eterm[i] == term) return e[i];
    return nullptr;
  }
  size_t row_bytes() const { return sizeof(int64_t) * (size_t)ne + sizeof(int32_t) * (size_t)nv; }
  void carve() {
    uint8_t* p = slab;
    for (int i = 0; i < ne; ++i, p += sizeof(int64_t) * (size_t)n) e[i] = reinterpret_cast<int64_t*>(p);
    for (int i = 0; i < nv; ++i, p += sizeof(int32_t) * (size_t)n) v[i] = reinterpret_cast<int32_t*>(p);
  }
};

struct Plan {
  int32_t n_vars, n_terms;
  const lpa_motif_term* terms;
  bool out_var[kMaxVars];   // the variable is in the result
  bool out_edge[16];        // the term's edge row is in the result
  // the columns of the table after term t: the bound variables that a later term or the result
  // reads, the wanted edges of the positive terms so far
  void columns(int t, Table* tb) const {
    bool bound[kMaxVars] = {}, later[kMaxVars] = {};
    for (int i = 0; i <= t; ++i)
      if (!terms[i].negated) bound[terms[i].src_var] = bound[terms[i].dst_var] = true;
    for (int i = t + 1; i < n_terms; ++i) later[terms[i].src_var] = later[terms[i].dst_var] = true;
    tb->nv = tb->ne = 0;
    for (int v = 0; v < n_vars; ++v)
      if (bound[v] && (later[v] || out_var[v])) tb->vvar[tb->nv++] = v;
    for (int i = 0; i <= t; ++i)
      if (!terms[i].negated && out_edge[i]) tb->eterm[tb->ne++] = i;
  }
};

double motif_ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// a table's memory: a stream-ordered temporary, or, for the final table of a call that returns
// rows, plain device memory that the result object owns from here on (res != null)
int motif_alloc(Tmp& tmp, Table* tb, lpa_motif_result* res) {
  const size_t bytes = tb->row_bytes() * (size_t)tb->n;
  if (res) {
    const hipError_t e = hipMalloc(&res->slab, bytes > 0 ? bytes : 1);
    if (e != hipSuccess) {
      res->slab = nullptr;
      (void)hipGetLastError();
      set_error("lpa_motif: hipMalloc(%zu bytes) for a result of %lld rows failed: %s", bytes, (long long)tb->n,
                hipGetErrorString(e));
      return LPA_ENOMEM;
    }
    tb->slab = static_cast<uint8_t*>(res->slab);
  } else {
    LPA_TRY(tmp.get(&tb->slab, (int64_t)bytes));
  }
  tb->carve();
  return LPA_OK;
}

int motif_run(lpa_graph* g, const Plan& pl, int64_t max_rows, bool count_only, lpa_motif_result* res,
              lpa_motif_summary* sm) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  const lpa_motif_term* terms = pl.terms;
  const int n_terms = pl.n_terms;
  if (V == 0 || m == 0) return LPA_OK;
  // LPA_MOTIF_TIMES=1: one line per filled step on stderr, host clocks in ms: count = the counts,
  // the scan and the read of the total; fill = the fill, behind a synchronisation of its own
  const char* env_times = getenv("LPA_MOTIF_TIMES");
  const bool times = env_times && atoi(env_times) == 1;
  Tmp tmp(s);
  ull* pinned = nullptr;
  LPA_TRY(tmp.pin(&pinned, 4));
  const volatile ull* hp = pinned;
  auto over = [&](int t, int64_t need) {
    sm->overflow_step = t;
    sm->overflow_rows = need;
    set_error("lpa_motif: step %d needs %lld rows, more than max_rows = %lld", t, (long long)need,
              (long long)max_rows);
    return LPA_EOVERFLOW;
  };
  // ---- seed ----
  Table cur;
  {
    int64_t *cnt = nullptr, *off = nullptr;
    ull* acc = nullptr;
    LPA_TRY(tmp.get(&cnt, m));
    LPA_TRY(tmp.get(&off, m + 1));
    LPA_TRY(tmp.get(&acc, S_LEN));
    LPA_HIP(hipMemsetAsync(acc, 0, sizeof(ull) * S_LEN, s));
    const int sv = terms[0].src_var, dv = terms[0].dst_var;
    hipLaunchKernelGGL(k_motif_seed_count, dim3(grid_bh(m)), dim3(256), 0, s, g->e_src, g->e_dst, m, (u32)V,
                       sv == dv ? 1 : 0, cnt, acc);
    LPA_HIP(hipGetLastError());
    LPA_TRY(exclusive_scan_i64(cnt, off, m, s));
    LPA_HIP(hipMemcpyAsync(pinned, off + m, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LPA_HIP(hipMemcpyAsync(pinned + 1, acc, sizeof(ull) * S_LEN, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipStreamSynchronize(s));
    const int64_t total = (int64_t)hp[0];
    sm->edges = (int64_t)hp[1 + S_VALID];
    sm->self_loops = (int64_t)hp[1 + S_LOOPS];
    sm->steps = 1;
    sm->table_rows[0] = sm->peak_rows = sm->rows = total;
    if (max_rows > 0 && total > max_rows) return over(0, total);
    if (total == 0 || (count_only && n_terms == 1)) return LPA_OK;
    cur.n = total;
    pl.columns(0, &cur);
    LPA_TRY(motif_alloc(tmp, &cur, n_terms == 1 ? res : nullptr));
    hipLaunchKernelGGL(k_motif_seed_fill, dim3(grid_for(m)), dim3(256), 0, s, g->e_src, g->e_dst, off, m,
                       cur.vcol(sv), sv == dv ? nullptr : cur.vcol(dv), cur.ecol(0));
    LPA_HIP(hipGetLastError());
    tmp.drop(cnt);
    tmp.drop(off);
    tmp.drop(acc);
  }
  // ---- lists ----
  EdgeLists el;
  if (n_terms > 1) {
    bool bound[kMaxVars] = {}, want_in = false;
    for (int t = 0; t < n_terms; ++t) {
      if (terms[t].negated) continue;
      if (t > 0 && !bound[terms[t].src_var]) want_in = true;
      bound[terms[t].src_var] = bound[terms[t].dst_var] = true;
    }
    LPA_TRY(edge_lists(g, tmp, want_in, &el));
  }
  // ---- steps ----
  bool bound[kMaxVars] = {};
  bound[terms[0].src_var] = bound[terms[0].dst_var] = true;
  for (int t = 1; t < n_terms; ++t) {
    const lpa_motif_term& tm = terms[t];
    const auto t_step = std::chrono::steady_clock::now();
    const bool sb = bound[tm.src_var], db = bound[tm.dst_var];
    const int64_t n = cur.n;
    int64_t *cnt = nullptr, *start = nullptr, *off = nullptr;
    LPA_TRY(tmp.get(&cnt, n));
    LPA_TRY(tmp.get(&off, n + 1));
    const int32_t* lcol = el.ocol;
    const int64_t* leid = el.oeid;
    const unsigned grid = grid_for(n);
    if (tm.negated) {
      hipLaunchKernelGGL(k_motif_count<M_NEGATE>, dim3(grid), dim3(256), 0, s, cur.vcol(tm.src_var),
                         cur.vcol(tm.dst_var), n, el.oo, el.ocol, cnt, start);
    } else {
      LPA_TRY(tmp.get(&start, n));
      if (sb && db) {
        hipLaunchKernelGGL(k_motif_count<M_CLOSE>, dim3(grid), dim3(256), 0, s, cur.vcol(tm.src_var),
                           cur.vcol(tm.dst_var), n, el.oo, el.ocol, cnt, start);
      } else if (sb) {
        hipLaunchKernelGGL(k_motif_count<M_EXTEND>, dim3(grid), dim3(256), 0, s, cur.vcol(tm.src_var),
                           (const int32_t*)nullptr, n, el.oo, el.ocol, cnt, start);
      } else {
        lcol = el.icol;
        leid = el.ieid;
        hipLaunchKernelGGL(k_motif_count<M_EXTEND>, dim3(grid), dim3(256), 0, s, cur.vcol(tm.dst_var),
                           (const int32_t*)nullptr, n, el.io, el.icol, cnt, start);
      }
    }
    LPA_HIP(hipGetLastError());
    LPA_TRY(exclusive_scan_i64(cnt, off, n, s));
    LPA_HIP(hipMemcpyAsync(pinned, off + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LPA_HIP(hipStreamSynchronize(s));
    const int64_t total = (int64_t)hp[0];
    sm->steps = t + 1;
    sm->table_rows[t] = sm->rows = total;
    if (total > sm->peak_rows) sm->peak_rows = total;
    if (max_rows > 0 && total > max_rows) return over(t, total);
    if (!tm.negated) bound[tm.src_var] = bound[tm.dst_var] = true;
    if (total == 0 || (count_only && t == n_terms - 1)) return LPA_OK;
    Table next;
    next.n = total;
    pl.columns(t, &next);
    LPA_TRY(motif_alloc(tmp, &next, t == n_terms - 1 ? res : nullptr));
    FillArgs fa = {};
    fa.off = off;
    fa.start = start;
    fa.n_parent = n;
    fa.total = total;
    fa.lcol = lcol;
    fa.leid = leid;
    for (int i = 0; i < next.nv; ++i) {
      const int32_t* from = cur.vcol(next.vvar[i]);
      if (from) {
        fa.vs[fa.nv] = from;
        fa.vd[fa.nv++] = next.v[i];
      } else {
        fa.newv = next.v[i];   // the one variable this term binds
      }
    }
    for (int i = 0; i < next.ne; ++i) {
      if (next.eterm[i] == t) {
        fa.newe = next.e[i];
      } else {
        fa.es[fa.ne] = cur.ecol(next.eterm[i]);
        fa.ed[fa.ne++] = next.e[i];
      }
    }
    const int64_t tiles = (total + kFillTile - 1) / kFillTile;
    const auto t_fill = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_motif_fill, dim3(grid_rows(tiles, 1, 65536)), dim3(256), 0, s, fa);
    LPA_HIP(hipGetLastError());
    if (times) {
      // written: the child's columns; gathered: the parent's kept columns and the list entries
      LPA_HIP(hipStreamSynchronize(s));
      const size_t per_row = next.row_bytes() + sizeof(int32_t) * (size_t)fa.nv + sizeof(int64_t) * (size_t)fa.ne +
                             (fa.newv ? sizeof(int32_t) : 0) + (fa.newe ? sizeof(int64_t) : 0);
      fprintf(stderr, "lpa_motif: step=%d parents=%lld rows=%lld count_ms=%.3f fill_ms=%.3f fill_bytes=%llu\n", t,
              (long long)n, (long long)total, motif_ms(t_step, t_fill), motif_ms(t_fill, std::chrono::steady_clock::now()),
              (unsigned long long)(per_row * (size_t)total));
    }
    tmp.drop(cur.slab);
    tmp.drop(cnt);
    tmp.drop(off);
    if (start) tmp.drop(start);
    cur = next;
  }
  // ---- the result: the final table, which the last allocation gave to res ----
  if (count_only) return LPA_OK;
  LPA_HIP(hipStreamSynchronize(s));
  res->rows = cur.n;
  for (int i = 0; i < cur.ne; ++i) res->ecol[cur.eterm[i]] = cur.e[i];
  for (int i = 0; i < cur.nv; ++i) res->vcol[cur.vvar[i]] = cur.v[i];
  return LPA_OK;
}

}  // namespace

// Reads V, m, e_src / e_dst and the stream of the handle, nothing of the LPA state; every device
// array but the final table is a stream-ordered temporary.  The arguments are checked by the caller (lpa_capi.cpp):
// the first term is positive, every later positive term has a bound variable, a negated term
// has both bound, var_out names bound variables only.  res (null iff count_only) is empty
// (rows 0, no column) and is filled here
int motif(lpa_graph* g, int32_t n_vars, const uint8_t* var_out, const lpa_motif_term* terms, int32_t n_terms,
          int64_t max_rows, int32_t count_only, lpa_motif_result* res, lpa_motif_summary* summary) {
  lpa_motif_summary sm;
  memset(&sm, 0, sizeof sm);
  sm.overflow_step = -1;
  Plan pl;
  pl.n_vars = n_vars;
  pl.n_terms = n_terms;
  pl.terms = terms;
  for (int v = 0; v < kMaxVars; ++v) pl.out_var[v] = !count_only && v < n_vars && var_out && var_out[v] != 0;
  for (int t = 0; t < 16; ++t)
    pl.out_edge[t] = !count_only && t < n_terms && !terms[t].negated && terms[t].want_edge != 0;
  const int rc = motif_run(g, pl, max_rows, count_only != 0, res, &sm);
  if (summary) *summary = sm;
  return rc;
}

}  // namespace lpa
