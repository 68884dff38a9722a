// Connected components of the handle's input multigraph, undirected view
// (GraphFrame.connectedComponents): comp[v] = the smallest dense id of v's component.
//
// Concurrent union-find over the kept edge list (e_src / e_dst, read once), no CSR:
//   init     parent[v] = v
//   hook     every edge (u, w), u != w: find both roots; if they differ, link the LARGER
//            root under the SMALLER one by atomicCAS(parent[larger], larger, smaller); a
//            failed CAS returns larger's new parent and the edge goes on from there
//   flatten  comp[v] = root(v)                                   (its own launch)
//   sizes    size[c] = members of c, then the summary (only when asked for; lpa_adj.hip)
//
// Invariant: every value ever stored in parent[x] is <= x and an ancestor of x.  A link
// stores a smaller root into a root; the path halving of find() stores x's grandparent,
// an ancestor again, and only into a non-root x (a non-root never becomes a root: its
// parent is < x for ever), so it never races a link.  Parent chains descend strictly,
// so every find ends; every root is the minimum of its tree; two vertices once in one
// tree stay in one; after the last edge every edge's endpoints share a tree, hence every
// root is a component minimum.  The result is a function of (V, edge set) alone,
// whatever the interleaving.
//
// Progress: lock-free.  A CAS fails only because another link of that root succeeded,
// and at most V - 1 links succeed.  No workgroup waits for another.
//
// Visibility: other CUs (and XCDs) link and halve while a wave reads.  Inside the hook
// kernel parent[] is touched only by agent-scope relaxed atomics (loads that bypass the
// CU's L1, CAS / stores performed at the memory side).  A stale read would still be an
// ancestor (values are never retracted), so relaxed order suffices: the CAS alone
// decides a link.  The flatten kernel runs after the kernel boundary: plain loads.
#include "lpa_device.h"
#include "lpa_algo.h"
#include "lpa_uf.h"

namespace lpa {

namespace {

__global__ __launch_bounds__(256) void k_cc_init(int32_t* __restrict__ parent, int64_t V) {
  GRID_STRIDE(v, V) parent[v] = (int32_t)v;
}

// m4: edges read as 16-byte vectors (a multiple of 4; 0 when a list is not 16-B aligned),
// the rest one by one.  The list is streamed once: non-temporal loads.
__global__ __launch_bounds__(256) void k_cc_hook(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                 int64_t m, int64_t m4, int32_t* __restrict__ parent) {
  const v4i* __restrict__ s4 = reinterpret_cast<const v4i*>(src);
  const v4i* __restrict__ d4 = reinterpret_cast<const v4i*>(dst);
  const int64_t n4 = m4 >> 2;
  GRID_STRIDE(q, n4) {
    const v4i s = __builtin_nontemporal_load(s4 + q);
    const v4i d = __builtin_nontemporal_load(d4 + q);
    // the eight parent reads of a quad go out together (independent L2 / HBM round
    // trips), then the few edges that still join two trees are linked
    int32_t a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] = cc_load(parent + s[k]);
      b[k] = cc_load(parent + d[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (s[k] != d[k] && a[k] != b[k]) cc_link(parent, s[k], a[k], d[k], b[k]);
  }
  const int64_t tail = m - m4;
  GRID_STRIDE(t, tail) {
    const int64_t e = m4 + t;
    cc_union(parent, __builtin_nontemporal_load(src + e), __builtin_nontemporal_load(dst + e));
  }
}

// after the hook kernel's end: parent[] is final, read with plain loads
__global__ __launch_bounds__(256) void k_cc_flatten(const int32_t* __restrict__ parent, int64_t V,
                                                    int32_t* __restrict__ comp) {
  GRID_STRIDE(v, V) comp[v] = cc_root(parent, (int32_t)v);
}

}  // namespace

// Reads V, m, e_src / e_dst and the stream of the handle, nothing of the LPA state.
int components(lpa_graph* g, int32_t* comp_out, int32_t out_is_device, int64_t* size_out,
               lpa_components_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  if (summary) *summary = lpa_components_summary{0, 0, 0, -1};
  if (V == 0) return LPA_OK;
  Tmp tmp(s);
  int32_t *parent = nullptr, *comp = comp_out;
  ull* size = nullptr;
  LPA_TRY(tmp.get(&parent, V));
  if (!out_is_device) LPA_TRY(tmp.get(&comp, V));
  hipLaunchKernelGGL(k_cc_init, dim3(grid_for(V)), dim3(256), 0, s, parent, V);
  LPA_HIP(hipGetLastError());
  if (m > 0) {
    const bool aligned = (((uintptr_t)g->e_src | (uintptr_t)g->e_dst) & 15u) == 0;
    const int64_t m4 = aligned ? (m & ~(int64_t)3) : 0;
    const int64_t items = m4 / 4 > m - m4 ? m4 / 4 : m - m4;
    hipLaunchKernelGGL(k_cc_hook, dim3(grid_for(items)), dim3(256), 0, s, g->e_src, g->e_dst, m, m4, parent);
    LPA_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_cc_flatten, dim3(grid_for(V)), dim3(256), 0, s, parent, V, comp);
  LPA_HIP(hipGetLastError());
  ull h[3] = {0, 0, 0};
  if (size_out || summary) LPA_TRY(comp_sizes(tmp, comp, V, size_out, out_is_device, summary != nullptr, &size, h));
  if (!out_is_device) {
    LPA_HIP(hipMemcpyAsync(comp_out, comp, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    if (size_out)
      LPA_HIP(hipMemcpyAsync(size_out, size, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  }
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->n_components = (int64_t)h[0];
    summary->n_singletons = (int64_t)h[1];
    summary->largest_size = (int64_t)(h[2] >> 32);
    summary->largest_id = (int64_t)(0xFFFFFFFFu - (u32)h[2]);
  }
  return LPA_OK;
}

}  // namespace lpa
