// Pregel over the handle's directed input multigraph (GraphFrame.pregel, graphframes.lib.Pregel
// of GraphFrames 0.8; include/lpa.h states the semantics): vertex columns that stay on the device
// across max_iter iterations.  An iteration sends the message programs along every kept edge row,
// reduces what a vertex receives to one aggregate (msg, null where nothing arrived) and replaces
// every Pregel column by its update program over the vertex's old columns and msg.  IEEE binary64
// throughout, no contraction into fused multiply-adds.
//
//   lists    edge_lists() (lpa_adj.hip), the offsets of the message lists and form_lists(), once:
//            the message list of v is its in-list rows (when a to_dst program exists) and then its
//            out-list rows (when a to_src program exists); its length in ROWS picks the form, by
//            the boundaries of lpa_aggregate_messages (lpa_graph::am_short / am_wave)
//   upload   the programs, the static columns and the edge columns, once
//   state    two buffers [n_vcols + n_pcols][V]: the static columns are copied into both, so a
//            message program reads column c of either kind at cur + c V (am_eval's vcols)
//   init     k_pg_init: Pregel column j of the first buffer = init[j] per vertex
//   iterate  k_pg_short, k_pg_wave, k_pg_block per iteration, back to back on the handle's stream:
//            each reduces a row as the k_am_* kernel of its form does (lpa_agg.hip), over the
//            program lists, then evaluates the n_pcols update programs and stores into next.  The
//            three write disjoint vertices of next and read only cur, so stream order is the only
//            synchronisation; the buffers swap on the host.  No per-edge message array and no
//            per-vertex aggregate array exists
//   out      the Pregel columns of the last buffer, the counters and the error word, once
//
// A lane takes its strided share of the rows in list order and, within a row, that direction's
// programs in the order given; then the xor-shuffle tree; then, in the block form, the 16 wave
// partials in order: the shape of lpa_aggregate_messages' sum, which with one program per
// direction it is bit for bit.  After the tree every lane of a row's group holds the row's
// result, so the whole group evaluates the update programs and one lane stores: the op fetch stays
// scalar.  The vertex-program interpreter (vp_eval) keeps am_eval's stack discipline -- the top in
// a register, the slots below in LDS [slot][thread], validity bits in a register -- in the same
// LDS, so no kernel has a runtime-indexed private array.
//
// A null value of an init or update program is an error that must not cost a synchronisation per
// iteration: the kernel stores NaN, records (iteration << 33 | column << 31 | vertex) with one
// 64-bit atomicMin and goes on; the host reads the word once, after the last iteration.  The only
// other atomics are the integer ones of the summary, at most two per wave at a kernel's end.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "lpa_device.h"
#include "lpa_algo.h"
#include "lpa_am.h"

#pragma clang fp contract(off)

namespace lpa {

namespace {

constexpr ull kPgNoError = ~0ull;

struct PgProg {
  const lpa_am_program *to_src, *to_dst;   // device [n_to_src], [n_to_dst]
  const lpa_vp_program* upd;               // device [n_pcols]
  int n_to_src, n_to_dst, n_pcols, n_vcols, agg;
};

__device__ __forceinline__ ull pg_error_key(int iter, int col, int64_t v) {
  return (ull)iter << 33 | (ull)col << 31 | (ull)v;
}

// One vertex program: P over the columns of vertex v (column c at cols[c V + v]) and the
// aggregate msg (msg_ok: not null).  True when the value is not null, *out the value.  stk: this
// thread's column of the LDS stack, kNT doubles from slot to slot.
template <int kNT>
__device__ __forceinline__ bool vp_eval(const lpa_vp_program* __restrict__ P, const double* __restrict__ cols,
                                        int64_t V, int64_t v, double msg, bool msg_ok, double* stk, double* out) {
  double t = 0.0;   // the top of the stack; the value at depth i < sp - 1 is stk[i * kNT]
  u32 vb = 0;       // bit i: the value at depth i is not null
  int sp = 0;
  const int n = P->n_ops;
  for (int pc = 0; pc < n; ++pc) {
    const u32 w = P->ops[pc];
    const u32 op = w & 0xFFFFu, arg = w >> 16;
    if (op <= LPA_VP_MSG) {   // the pushes
      if (sp > 0) stk[(sp - 1) * kNT] = t;
      bool ok = true;
      switch (op) {
        case LPA_VP_CONST: t = P->consts[arg]; break;
        case LPA_VP_COL: t = cols[(int64_t)arg * V + v]; break;
        default: t = msg; ok = msg_ok; break;
      }
      vb = (vb & ~(1u << sp)) | ((ok ? 1u : 0u) << sp);
      ++sp;
    } else if (op == LPA_VP_NEG) {
      t = -t;
    } else if (op == LPA_VP_ABS) {
      t = __builtin_fabs(t);
    } else if (op == LPA_VP_NOT) {
      t = t != 0.0 ? 0.0 : 1.0;
    } else if (op == LPA_VP_ISNULL) {
      t = (vb >> (sp - 1)) & 1u ? 0.0 : 1.0;
      vb |= 1u << (sp - 1);
    } else if (op == LPA_VP_WHEN_ELSE) {   // condition, value, otherwise
      const double c = stk[(sp - 3) * kNT], x = stk[(sp - 2) * kNT];
      const bool take = ((vb >> (sp - 3)) & 1u) && c != 0.0;
      const bool ok = take ? (vb >> (sp - 2)) & 1u : (vb >> (sp - 1)) & 1u;
      t = take ? x : t;
      sp -= 2;
      vb = (vb & ((1u << (sp - 1)) - 1u)) | ((ok ? 1u : 0u) << (sp - 1));
    } else {   // the binary ops
      const double a = stk[(sp - 2) * kNT], b = t;
      const bool a_ok = (vb >> (sp - 2)) & 1u, b_ok = (vb >> (sp - 1)) & 1u;
      bool ok = a_ok && b_ok;
      switch (op) {
        case LPA_VP_ADD: t = a + b; break;
        case LPA_VP_SUB: t = a - b; break;
        case LPA_VP_MUL: t = a * b; break;
        case LPA_VP_DIV: t = a / b; ok = ok && b != 0.0; break;
        case LPA_VP_EQ: t = a == b ? 1.0 : 0.0; break;
        case LPA_VP_NE: t = a != b ? 1.0 : 0.0; break;
        case LPA_VP_LT: t = a < b ? 1.0 : 0.0; break;
        case LPA_VP_LE: t = a <= b ? 1.0 : 0.0; break;
        case LPA_VP_GT: t = a > b ? 1.0 : 0.0; break;
        case LPA_VP_GE: t = a >= b ? 1.0 : 0.0; break;
        case LPA_VP_AND: t = a != 0.0 && b != 0.0 ? 1.0 : 0.0; break;
        case LPA_VP_OR: t = a != 0.0 || b != 0.0 ? 1.0 : 0.0; break;
        case LPA_VP_COALESCE:
          t = a_ok ? a : b;
          ok = a_ok || b_ok;
          break;
        default:   // LPA_VP_WHEN: condition, value
          ok = a_ok && a != 0.0 && b_ok;
          break;
      }
      sp -= 1;
      vb = (vb & ((1u << (sp - 1)) - 1u)) | ((ok ? 1u : 0u) << (sp - 1));
    }
  }
  *out = t;
  return (vb & 1u) != 0;
}

// this lane's share of the message list of v, rows `stride` apart from `first`, in list order: the
// in-list rows under the to_dst programs, then the out-list rows under the to_src programs, a
// row's programs in the order given
template <int kNT>
__device__ __forceinline__ void pg_row(const PgProg& pg, const AmIn& in, const AmLists& l, int64_t v, int first,
                                       int stride, double* stk, AmRow& a) {
  int64_t i = first;
  if (l.io) {
    const int64_t b = l.io[v], L = l.io[v + 1] - b;
    for (; i < L; i += stride) {
      const int64_t s = l.icol[b + i], e = l.ieid[b + i];
      for (int p = 0; p < pg.n_to_dst; ++p) {
        double x;
        const bool ok = am_eval<kNT>(pg.to_dst + p, in, s, v, e, stk, &x);
        am_take(a, ok, x, a.c_dst);
      }
    }
    i -= L;
  }
  if (l.oo) {
    const int64_t b = l.oo[v], L = l.oo[v + 1] - b;
    for (; i < L; i += stride) {
      const int64_t d = l.ocol[b + i], e = l.oeid[b + i];
      for (int p = 0; p < pg.n_to_src; ++p) {
        double x;
        const bool ok = am_eval<kNT>(pg.to_src + p, in, v, d, e, stk, &x);
        am_take(a, ok, x, a.c_src);
      }
    }
  }
}

// the aggregate of a row's partial; false: nothing was delivered, msg is null
__device__ __forceinline__ bool pg_msg(int agg, const AmRow& a, double* msg) {
  const int64_t c = (int64_t)a.c_dst + (int64_t)a.c_src;
  switch (agg) {
    case LPA_PG_SUM: *msg = a.sum; break;
    case LPA_PG_MIN: *msg = a.mn; break;
    case LPA_PG_MAX: *msg = a.mx; break;
    case LPA_PG_AVG: *msg = a.sum / (double)c; break;
    default: *msg = (double)c; break;
  }
  return c != 0;
}

// Pregel column j of vertex v in next = update[j] over cur's columns and the row's aggregate.
// Called by every lane that holds the row's partial; `store`: the one lane that writes
template <int kNT>
__device__ __forceinline__ void pg_update(const PgProg& pg, const double* __restrict__ cur, double* __restrict__ next,
                                          int64_t V, int64_t v, const AmRow& a, int iter, bool store, double* stk,
                                          ull* __restrict__ err) {
  double msg;
  const bool msg_ok = pg_msg(pg.agg, a, &msg);
  for (int j = 0; j < pg.n_pcols; ++j) {
    double x;
    const bool ok = vp_eval<kNT>(pg.upd + j, cur, V, v, msg, msg_ok, stk, &x);
    if (store) {
      next[(int64_t)(pg.n_vcols + j) * V + v] = ok ? x : NAN;
      if (!ok) atomicMin(err, pg_error_key(iter, j, v));
    }
  }
}

// cnt[0] += messages delivered to destinations, [1] to sources: a thread's totals, two atomics
// per wave at the kernel's end
__device__ __forceinline__ void pg_counts(ull* __restrict__ cnt, ull n_dst, ull n_src) {
  for (int off = 32; off > 0; off >>= 1) {
    n_dst += __shfl_xor(n_dst, off, 64);
    n_src += __shfl_xor(n_src, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_dst) atomicAdd(&cnt[0], n_dst);
    if (n_src) atomicAdd(&cnt[1], n_src);
  }
}

// the start: Pregel column j of every vertex = init[j] over the static columns (iteration 0 of
// the error word)
__global__ __launch_bounds__(256) void k_pg_init(const lpa_vp_program* __restrict__ init, int n_pcols, int n_vcols,
                                                 double* __restrict__ cols, int64_t V, ull* __restrict__ err) {
  __shared__ double stk[kAmLdsSlots * 256];
  GRID_STRIDE(v, V) {
    for (int j = 0; j < n_pcols; ++j) {
      double x;
      const bool ok = vp_eval<256>(init + j, cols, V, v, 0.0, false, stk + threadIdx.x, &x);
      cols[(int64_t)(n_vcols + j) * V + v] = ok ? x : NAN;
      if (!ok) atomicMin(err, pg_error_key(0, j, v));
    }
  }
}

// every row in id order, kShortLanes lanes each; a row longer than short_max is not this
// form's (L = 0 always is)
__global__ __launch_bounds__(256) void k_pg_short(PgProg pg, AmIn in, AmLists l, int64_t short_max,
                                                  double* __restrict__ next, int iter, ull* __restrict__ cnt,
                                                  ull* __restrict__ err) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  __shared__ double stk[kAmLdsSlots * 256];
  const int sub = threadIdx.x & (G - 1);
  ull n_dst = 0, n_src = 0;
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < in.V; base += (int64_t)gridDim.x * kRows) {
    const int64_t v = base + threadIdx.x / G;
    bool mine = false;
    AmRow a = am_empty();
    if (v < in.V) {
      const int64_t L = am_len(l, v);
      mine = L == 0 || L <= short_max;
      if (mine) pg_row<256>(pg, in, l, v, sub, G, stk + threadIdx.x, a);
    }
    am_tree<G>(a);
    if (mine) {
      pg_update<256>(pg, in.vcols, next, in.V, v, a, iter, sub == 0, stk + threadIdx.x, err);
      if (sub == 0) {
        n_dst += a.c_dst;
        n_src += a.c_src;
      }
    }
  }
  pg_counts(cnt, n_dst, n_src);
}

// a wave per listed row
__global__ __launch_bounds__(256) void k_pg_wave(const int32_t* __restrict__ rows, int64_t nrows, PgProg pg, AmIn in,
                                                 AmLists l, double* __restrict__ next, int iter,
                                                 ull* __restrict__ cnt, ull* __restrict__ err) {
  __shared__ double stk[kAmLdsSlots * 256];
  const int lane = threadIdx.x & 63;
  ull n_dst = 0, n_src = 0;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t v = rows[k];
    AmRow a = am_empty();
    pg_row<256>(pg, in, l, v, lane, 64, stk + threadIdx.x, a);
    am_tree<64>(a);
    pg_update<256>(pg, in.vcols, next, in.V, v, a, iter, lane == 0, stk + threadIdx.x, err);
    if (lane == 0) {
      n_dst += a.c_dst;
      n_src += a.c_src;
    }
  }
  pg_counts(cnt, n_dst, n_src);
}

// a block per listed row (k is the same in every thread: barriers inside); the first wave merges
// the 16 partials in order, every lane of it the same, and evaluates the update
__global__ __launch_bounds__(kBlockThreads) void k_pg_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                            PgProg pg, AmIn in, AmLists l, double* __restrict__ next,
                                                            int iter, ull* __restrict__ cnt, ull* __restrict__ err) {
  constexpr int kWaves = kBlockThreads / 64;
  __shared__ double stk[kAmLdsSlots * kBlockThreads];
  __shared__ AmRow ws[kWaves];
  ull n_dst = 0, n_src = 0;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t v = rows[k];
    AmRow a = am_empty();
    pg_row<kBlockThreads>(pg, in, l, v, threadIdx.x, kBlockThreads, stk + threadIdx.x, a);
    am_tree<64>(a);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x < 64) {
      AmRow t = ws[0];
#pragma nounroll   // 16 partials loaded at once would cost the registers of all of them
      for (int i = 1; i < kWaves; ++i) am_merge(t, ws[i]);
      pg_update<kBlockThreads>(pg, in.vcols, next, in.V, v, t, iter, threadIdx.x == 0, stk + threadIdx.x, err);
      if (threadIdx.x == 0) {
        n_dst += t.c_dst;
        n_src += t.c_src;
      }
    }
    __syncthreads();   // before the next row rewrites ws
  }
  pg_counts(cnt, n_dst, n_src);
}

}  // namespace

// The programs and the other arguments were validated by the caller (lpa_capi.cpp).  Every array
// is a stream-ordered temporary; reads V, m, e_src / e_dst, the stream and the am_* boundaries of
// the handle.
int pregel(lpa_graph* g, int32_t max_iter, int32_t agg, const lpa_am_program* to_src, int32_t n_to_src,
           const lpa_am_program* to_dst, int32_t n_to_dst, const lpa_vp_program* init, const lpa_vp_program* update,
           int32_t n_pcols, const double* vcols, int32_t n_vcols, const double* ecols, int32_t n_ecols,
           double* cols_out, lpa_pregel_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  if (summary) *summary = lpa_pregel_summary{0, 0, 0, 0, V, 0, 0, 0, 0, -1, -1, -1};
  if (V == 0) return LPA_OK;
  // a row's delivered messages of one direction are counted in 32 bits (AmRow)
  if ((int64_t)(n_to_src > n_to_dst ? n_to_src : n_to_dst) * m > (int64_t)0xFFFFFFFFll) {
    set_error("lpa_pregel: %d messages along each of %lld edge rows are more than a vertex's 32-bit message counter "
              "admits", n_to_src > n_to_dst ? n_to_src : n_to_dst, (long long)m);
    return LPA_EINVAL;
  }
  Tmp tmp(s);
  // ---- lists ----
  EdgeLists el;
  LPA_TRY(edge_lists(g, tmp, n_to_dst > 0, &el));
  AmLists l{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (n_to_dst > 0) l.io = el.io, l.icol = el.icol, l.ieid = el.ieid;
  if (n_to_src > 0) l.oo = el.oo, l.ocol = el.ocol, l.oeid = el.oeid;
  int64_t* off = nullptr;
  ull* cnt = nullptr;   // messages to destinations, to sources, (unused), the longest list; [4] the error word
  int32_t* lists = nullptr;
  u32 h[2] = {0, 0};
  ull hc[5] = {0, 0, 0, 0, kPgNoError};
  LPA_TRY(tmp.get(&off, V + 1));
  LPA_TRY(tmp.get(&cnt, 5));
  LPA_HIP(hipMemcpyAsync(cnt, hc, sizeof(hc), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_am_offsets, dim3(grid_bh(V + 1)), dim3(256), 0, s, l, V, off, cnt);
  LPA_HIP(hipGetLastError());
  LPA_TRY(form_lists(tmp, off, V, (int64_t)g->am_short, (int64_t)g->am_wave, &lists, h));
  // ---- upload ----
  lpa_am_program* d_msg = nullptr;   // [n_to_src] then [n_to_dst]
  lpa_vp_program* d_vp = nullptr;    // [n_pcols] init then [n_pcols] update
  double *buf[2] = {nullptr, nullptr}, *de = nullptr;
  const int n_cols = n_vcols + n_pcols;
  LPA_TRY(tmp.get(&d_msg, n_to_src + n_to_dst));
  LPA_TRY(tmp.get(&d_vp, 2 * n_pcols));
  if (n_to_src > 0)
    LPA_HIP(hipMemcpyAsync(d_msg, to_src, sizeof(lpa_am_program) * (size_t)n_to_src, hipMemcpyHostToDevice, s));
  if (n_to_dst > 0)
    LPA_HIP(hipMemcpyAsync(d_msg + n_to_src, to_dst, sizeof(lpa_am_program) * (size_t)n_to_dst, hipMemcpyHostToDevice,
                           s));
  LPA_HIP(hipMemcpyAsync(d_vp, init, sizeof(lpa_vp_program) * (size_t)n_pcols, hipMemcpyHostToDevice, s));
  LPA_HIP(hipMemcpyAsync(d_vp + n_pcols, update, sizeof(lpa_vp_program) * (size_t)n_pcols, hipMemcpyHostToDevice, s));
  for (int b = 0; b < 2; ++b) LPA_TRY(tmp.get(&buf[b], (int64_t)n_cols * V));
  if (n_vcols > 0) {
    const size_t bytes = sizeof(double) * (size_t)n_vcols * (size_t)V;
    LPA_HIP(hipMemcpyAsync(buf[0], vcols, bytes, hipMemcpyHostToDevice, s));
    LPA_HIP(hipMemcpyAsync(buf[1], buf[0], bytes, hipMemcpyDeviceToDevice, s));
  }
  if (n_ecols > 0 && m > 0) {
    LPA_TRY(tmp.get(&de, (int64_t)n_ecols * m));
    LPA_HIP(hipMemcpyAsync(de, ecols, sizeof(double) * (size_t)n_ecols * (size_t)m, hipMemcpyHostToDevice, s));
  }
  // ---- init ----
  hipLaunchKernelGGL(k_pg_init, dim3(grid_bh(V)), dim3(256), 0, s, d_vp, (int)n_pcols, (int)n_vcols, buf[0], V,
                     cnt + 4);
  LPA_HIP(hipGetLastError());
  LPA_HIP(hipStreamSynchronize(s));   // h: the lists' lengths; the host arrays may go
  // ---- iterate: no synchronisation from here to the copies out ----
  const PgProg pg{d_msg, d_msg + n_to_src, d_vp + n_pcols, n_to_src, n_to_dst, n_pcols, n_vcols, agg};
  int cur = 0;
  for (int32_t it = 1; it <= max_iter; ++it, cur ^= 1) {
    const AmIn in{nullptr, buf[cur], de, V, m};
    double* next = buf[cur ^ 1];
    hipLaunchKernelGGL(k_pg_short, dim3(grid_rows(V, 256 / kShortLanes, kAmGrid)), dim3(256), 0, s, pg, in, l,
                       (int64_t)g->am_short, next, (int)it, cnt, cnt + 4);
    if (h[0])
      hipLaunchKernelGGL(k_pg_wave, dim3(grid_rows(h[0], 4, kAmGrid)), dim3(256), 0, s, lists, (int64_t)h[0], pg, in,
                         l, next, (int)it, cnt, cnt + 4);
    if (h[1])
      hipLaunchKernelGGL(k_pg_block, dim3(grid_rows(h[1], 1, 4096)), dim3(kBlockThreads), 0, s, lists + V,
                         (int64_t)h[1], pg, in, l, next, (int)it, cnt, cnt + 4);
    LPA_HIP(hipGetLastError());
  }
  // ---- out ----
  LPA_HIP(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  if (hc[4] != kPgNoError) {
    const long long it = (long long)(hc[4] >> 33), col = (long long)((hc[4] >> 31) & 3u),
                    v = (long long)(hc[4] & 0x7FFFFFFFull);
    if (summary) summary->null_iteration = it, summary->null_column = col, summary->null_vertex = v;
    if (it == 0)
      set_error("lpa_pregel: the initial program of Pregel column %lld is null at vertex %lld; a column holds no "
                "null: give the value with COALESCE",
                col, v);
    else
      set_error("lpa_pregel: in iteration %lld the update program of Pregel column %lld is null at vertex %lld; a "
                "column holds no null: give the value with COALESCE",
                it, col, v);
    return LPA_EINVAL;
  }
  LPA_HIP(hipMemcpyAsync(cols_out, buf[cur] + (int64_t)n_vcols * V, sizeof(double) * (size_t)n_pcols * (size_t)V,
                         hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    const int64_t evaluated = el.mv * (int64_t)(n_to_dst + n_to_src) * (int64_t)max_iter;
    summary->edges = el.mv;
    summary->messages_to_dst = (int64_t)hc[0];
    summary->messages_to_src = (int64_t)hc[1];
    summary->nulls = evaluated - (int64_t)hc[0] - (int64_t)hc[1];
    summary->rows_wave = (int64_t)h[0];
    summary->rows_block = (int64_t)h[1];
    summary->rows_short = V - (int64_t)h[0] - (int64_t)h[1];
    summary->max_row = (int64_t)hc[3];
    summary->iterations = max_iter;
  }
  return LPA_OK;
}

}  // namespace lpa
