// Message aggregation over the handle's directed input multigraph (GraphFrame.aggregateMessages,
// GraphX aggregateMessages): every kept edge row sends the value of a caller-supplied expression
// to its destination (the to_dst program), to its source (to_src), or both; every vertex reduces
// what it receives to count, sum, min and max.  A fused pull: no per-edge message array exists.
// IEEE binary64 throughout.
//
//   lists    edge_lists() (lpa_adj.hip): the in-lists sorted by (dst, src, edge row) and the
//            out-lists by (src, dst, edge row), each row with its index in the input
//   rows     the message list of v is its in-list rows (to_dst: dst = v, src = icol[i], edge =
//            ieid[i]) and then its out-list rows (to_src: src = v, dst = ocol[i], edge = oeid[i]);
//            a direction without a program contributes no rows.  off[] = the element-wise sum of
//            the offsets of the directions in use is the offset array of those lists: form_lists()
//            takes it
//   upload   the programs, the vertex columns [n_vcols][V] and the edge columns [n_ecols][m]
//   reduce   one launch per row form, by list length L (boundaries: lpa_graph::am_short / am_wave):
//     short   L <= am_short   8 lanes per row, 32 rows per block, rows in id order; L = 0 is
//             always a short row (count 0, sum 0.0, min and max NaN)
//     wave    L <= am_wave    a wave per listed row
//     block   above           a block of 1024 per listed row
//
// The interpreter (am_eval; it and the other pieces that lpa_pregel.hip shares are in lpa_am.h) is
// one loop over the postfix program's ops, which the C ABI validated on the host: the kernels
// trust it.  Every lane of a launch runs the same op at the same time (a
// lane's in-list share and its out-list share are two loops), so the op fetch is scalar and the
// switch does not diverge.  The operand stack never becomes a runtime-indexed private array: its
// top is a register and the seven slots below it live in LDS, laid out [slot][thread], so a slot
// is an LDS address computed from the (uniform) depth.  Validity -- "not null" -- is a bit per
// stack slot in one register.  Null rules: an operator with a null operand gives null, x / 0
// gives null, a when() whose condition is null or false gives its otherwise() value, or null
// without one; a null message is not delivered.
//
// No floating-point atomics.  Every lane accumulates count, sum, min and max over its strided
// share of the list in list order (one accumulator each), then an xor-shuffle tree (both sides of
// an exchange form the same commutative result), then, in the block form, the 16 wave partials in
// order.  So
//   - count, min, max and every summary integer except rows_* are a function of the inputs alone
//     (min prefers -0.0 to +0.0 and max +0.0 to -0.0, whatever the order);
//   - sum is bit-identical across calls and handles with the same boundaries;
//   - sum is bit-identical across input edge orders whenever parallel edges carry equal messages
//     (any program that reads no edge column): the lists are sorted by (dst, src, row).
// With finite inputs a NaN message can only come from overflow (inf - inf); min and max then
// follow the comparisons as written and are unspecified.  The only atomics are the integer ones
// of the summary: they commute.
//
// No contraction into fused multiply-adds in this file: a message is the double that numpy
// computes op by op.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>

#include "lpa_device.h"
#include "lpa_algo.h"
#include "lpa_am.h"

#pragma clang fp contract(off)

namespace lpa {

namespace {

struct AmOut {
  int64_t* count;
  double *sum, *mn, *mx;
};

// this lane's share of the message list of v, entries `stride` apart from `first`, in list order:
// the in-list rows under the to_dst program, then the out-list rows under the to_src program
template <int kNT>
__device__ __forceinline__ void am_row(const AmIn& in, const AmLists& l, int64_t v, int first, int stride, double* stk,
                                       AmRow& a) {
  int64_t i = first;
  if (l.io) {
    const int64_t b = l.io[v], L = l.io[v + 1] - b;
    for (; i < L; i += stride) {
      double x;
      const bool ok = am_eval<kNT>(in.prog + 1, in, (int64_t)l.icol[b + i], v, l.ieid[b + i], stk, &x);
      am_take(a, ok, x, a.c_dst);
    }
    i -= L;
  }
  if (l.oo) {
    const int64_t b = l.oo[v], L = l.oo[v + 1] - b;
    for (; i < L; i += stride) {
      double x;
      const bool ok = am_eval<kNT>(in.prog, in, v, (int64_t)l.ocol[b + i], l.oeid[b + i], stk, &x);
      am_take(a, ok, x, a.c_src);
    }
  }
}

__device__ __forceinline__ void am_store(const AmOut& o, int64_t v, const AmRow& a) {
  const int64_t c = (int64_t)a.c_dst + (int64_t)a.c_src;
  o.count[v] = c;
  o.sum[v] = c ? a.sum : 0.0;
  o.mn[v] = c ? a.mn : NAN;
  o.mx[v] = c ? a.mx : NAN;
}

// every row in id order, kShortLanes lanes each; a row longer than short_max is not this
// form's (L = 0 always is)
__global__ __launch_bounds__(256) void k_am_short(AmIn in, AmLists l, int64_t short_max, AmOut out,
                                                  ull* __restrict__ cnt) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  __shared__ double stk[kAmLdsSlots * 256];
  const int sub = threadIdx.x & (G - 1);
  ull n_dst = 0, n_src = 0, n_recv = 0;
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < in.V; base += (int64_t)gridDim.x * kRows) {
    const int64_t v = base + threadIdx.x / G;
    bool mine = false;
    AmRow a = am_empty();
    if (v < in.V) {
      const int64_t L = am_len(l, v);
      mine = L == 0 || L <= short_max;
      if (mine) am_row<256>(in, l, v, sub, G, stk + threadIdx.x, a);
    }
    am_tree<G>(a);
    if (mine && sub == 0) {
      am_store(out, v, a);
      n_dst += a.c_dst;
      n_src += a.c_src;
      n_recv += a.c_dst + a.c_src ? 1u : 0u;
    }
  }
  am_counts(cnt, n_dst, n_src, n_recv);
}

// a wave per listed row
__global__ __launch_bounds__(256) void k_am_wave(const int32_t* __restrict__ rows, int64_t nrows, AmIn in, AmLists l,
                                                 AmOut out, ull* __restrict__ cnt) {
  __shared__ double stk[kAmLdsSlots * 256];
  const int lane = threadIdx.x & 63;
  ull n_dst = 0, n_src = 0, n_recv = 0;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int64_t v = rows[k];
    AmRow a = am_empty();
    am_row<256>(in, l, v, lane, 64, stk + threadIdx.x, a);
    am_tree<64>(a);
    if (lane == 0) {
      am_store(out, v, a);
      n_dst += a.c_dst;
      n_src += a.c_src;
      n_recv += a.c_dst + a.c_src ? 1u : 0u;
    }
  }
  am_counts(cnt, n_dst, n_src, n_recv);
}

// a block per listed row (k is the same in every thread: barriers inside)
__global__ __launch_bounds__(kBlockThreads) void k_am_block(const int32_t* __restrict__ rows, int64_t nrows, AmIn in,
                                                            AmLists l, AmOut out, ull* __restrict__ cnt) {
  constexpr int kWaves = kBlockThreads / 64;
  __shared__ double stk[kAmLdsSlots * kBlockThreads];
  __shared__ AmRow ws[kWaves];
  ull n_dst = 0, n_src = 0, n_recv = 0;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int64_t v = rows[k];
    AmRow a = am_empty();
    am_row<kBlockThreads>(in, l, v, threadIdx.x, kBlockThreads, stk + threadIdx.x, a);
    am_tree<64>(a);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      AmRow t = ws[0];
      for (int i = 1; i < kWaves; ++i) am_merge(t, ws[i]);
      am_store(out, v, t);
      n_dst += t.c_dst;
      n_src += t.c_src;
      n_recv += t.c_dst + t.c_src ? 1u : 0u;
    }
    __syncthreads();   // before the next row rewrites ws
  }
  am_counts(cnt, n_dst, n_src, n_recv);
}

double am_ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

}  // namespace

// The programs were validated by the caller (lpa_capi.cpp).  Every array is a stream-ordered
// temporary; reads V, m, e_src / e_dst, the stream and the am_* boundaries of the handle.
int aggregate_messages(lpa_graph* g, const lpa_am_program* to_src, const lpa_am_program* to_dst, const double* vcols,
                       int32_t n_vcols, const double* ecols, int32_t n_ecols, int64_t* count_out, double* sum_out,
                       double* min_out, double* max_out, lpa_am_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  if (summary) *summary = lpa_am_summary{0, 0, 0, 0, 0, V, 0, 0, 0};
  if (V == 0) return LPA_OK;
  const auto empty = [&]() {
    for (int64_t v = 0; v < V; ++v) {
      if (count_out) count_out[v] = 0;
      if (sum_out) sum_out[v] = 0.0;
      if (min_out) min_out[v] = NAN;
      if (max_out) max_out[v] = NAN;
    }
    return (int)LPA_OK;
  };
  if (m == 0) return empty();
  // LPA_AM_TIMES=1: one line of stage times on stderr, host clocks in ms, each stage behind a
  // synchronisation of its own: lists = the edge lists, the offsets and the form lists; upload = the
  // programs and the columns; reduce = the three launches; out = the copies to the host
  const char* env_times = getenv("LPA_AM_TIMES");
  const bool times = env_times && atoi(env_times) == 1;
  const auto t0 = std::chrono::steady_clock::now();
  Tmp tmp(s);
  EdgeLists el;
  LPA_TRY(edge_lists(g, tmp, to_dst != nullptr, &el));
  if (el.mv == 0) return empty();
  AmLists l{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (to_dst) l.io = el.io, l.icol = el.icol, l.ieid = el.ieid;
  if (to_src) l.oo = el.oo, l.ocol = el.ocol, l.oeid = el.oeid;
  // ---- rows ----
  int64_t* off = nullptr;
  ull* cnt = nullptr;   // messages to destinations, to sources, receivers, the longest list
  int32_t* lists = nullptr;
  u32 h[2] = {0, 0};
  ull hc[4] = {0, 0, 0, 0};
  LPA_TRY(tmp.get(&off, V + 1));
  LPA_TRY(tmp.get(&cnt, 4));
  LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(ull) * 4, s));
  hipLaunchKernelGGL(k_am_offsets, dim3(grid_bh(V + 1)), dim3(256), 0, s, l, V, off, cnt);
  LPA_HIP(hipGetLastError());
  LPA_TRY(form_lists(tmp, off, V, (int64_t)g->am_short, (int64_t)g->am_wave, &lists, h));
  if (times) LPA_HIP(hipStreamSynchronize(s));
  const double ms_lists = am_ms_since(t0);
  const auto t1 = std::chrono::steady_clock::now();
  // ---- upload ----
  lpa_am_program* prog = nullptr;
  double *dv = nullptr, *de = nullptr;
  LPA_TRY(tmp.get(&prog, 2));
  if (to_src) LPA_HIP(hipMemcpyAsync(prog, to_src, sizeof(lpa_am_program), hipMemcpyHostToDevice, s));
  if (to_dst) LPA_HIP(hipMemcpyAsync(prog + 1, to_dst, sizeof(lpa_am_program), hipMemcpyHostToDevice, s));
  if (n_vcols > 0) {
    LPA_TRY(tmp.get(&dv, (int64_t)n_vcols * V));
    LPA_HIP(hipMemcpyAsync(dv, vcols, sizeof(double) * (size_t)n_vcols * (size_t)V, hipMemcpyHostToDevice, s));
  }
  if (n_ecols > 0) {
    LPA_TRY(tmp.get(&de, (int64_t)n_ecols * m));
    LPA_HIP(hipMemcpyAsync(de, ecols, sizeof(double) * (size_t)n_ecols * (size_t)m, hipMemcpyHostToDevice, s));
  }
  AmOut out{nullptr, nullptr, nullptr, nullptr};
  LPA_TRY(tmp.get(&out.count, V));
  LPA_TRY(tmp.get(&out.sum, V));
  LPA_TRY(tmp.get(&out.mn, V));
  LPA_TRY(tmp.get(&out.mx, V));
  LPA_HIP(hipStreamSynchronize(s));   // h: the lists' lengths
  const double ms_upload = am_ms_since(t1);
  const auto t2 = std::chrono::steady_clock::now();
  // ---- reduce ----
  // grids of at most kAmGrid blocks, eight to a CU (what the kernels' registers admit): every wave ends
  // with up to three atomics on the same counters, and 5 x 10^5 of those took 6 ms at R-MAT-22
  const AmIn in{prog, dv, de, V, m};
  hipLaunchKernelGGL(k_am_short, dim3(grid_rows(V, 256 / kShortLanes, kAmGrid)), dim3(256), 0, s, in, l,
                     (int64_t)g->am_short, out, cnt);
  if (h[0])
    hipLaunchKernelGGL(k_am_wave, dim3(grid_rows(h[0], 4, kAmGrid)), dim3(256), 0, s, lists, (int64_t)h[0], in, l, out,
                       cnt);
  if (h[1])
    hipLaunchKernelGGL(k_am_block, dim3(grid_rows(h[1], 1, 4096)), dim3(kBlockThreads), 0, s, lists + V, (int64_t)h[1],
                       in, l, out, cnt);
  LPA_HIP(hipGetLastError());
  if (times) LPA_HIP(hipStreamSynchronize(s));
  const double ms_reduce = am_ms_since(t2);
  const auto t3 = std::chrono::steady_clock::now();
  if (count_out) LPA_HIP(hipMemcpyAsync(count_out, out.count, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  if (sum_out) LPA_HIP(hipMemcpyAsync(sum_out, out.sum, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, s));
  if (min_out) LPA_HIP(hipMemcpyAsync(min_out, out.mn, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, s));
  if (max_out) LPA_HIP(hipMemcpyAsync(max_out, out.mx, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, s));
  LPA_HIP(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, s));
  LPA_HIP(hipStreamSynchronize(s));
  if (times)
    fprintf(stderr, "lpa_aggregate_messages: lists_ms=%.3f upload_ms=%.3f reduce_ms=%.3f out_ms=%.3f\n", ms_lists,
            ms_upload, ms_reduce, am_ms_since(t3));
  if (summary) {
    const int64_t evaluated = (to_dst ? el.mv : 0) + (to_src ? el.mv : 0);
    summary->edges = el.mv;
    summary->messages_to_dst = (int64_t)hc[0];
    summary->messages_to_src = (int64_t)hc[1];
    summary->nulls = evaluated - (int64_t)hc[0] - (int64_t)hc[1];
    summary->receivers = (int64_t)hc[2];
    summary->rows_wave = (int64_t)h[0];
    summary->rows_block = (int64_t)h[1];
    summary->rows_short = V - (int64_t)h[0] - (int64_t)h[1];
    summary->max_row = (int64_t)hc[3];
  }
  return LPA_OK;
}

}  // namespace lpa
