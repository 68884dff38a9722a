// Connected components of the handle's input multigraph, undirected view
// (GraphFrame.connectedComponents): comp[v] = the smallest dense id of v's component.
//
// Concurrent union-find over the kept edge list (e_src / e_dst, read once), no CSR:
//   init     parent[v] = v
//   hook     every edge (u, w), u != w: find both roots; if they differ, link the LARGER
//            root under the SMALLER one by atomicCAS(parent[larger], larger, smaller); a
//            failed CAS returns larger's new parent and the edge goes on from there
//   flatten  comp[v] = root(v)                                   (its own launch)
//   sizes    size[c] = members of c, then the summary            (only when asked for)
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

namespace lpa {

namespace {

inline unsigned grid_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > 65536) b = 65536;
  return (unsigned)b;
}
// block-aggregated passes: few blocks, each over a long stretch of the input
inline unsigned grid_bh(int64_t n) {
  const unsigned g = grid_for(n);
  return g < 2048u ? g : 2048u;
}

#define GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

#define CC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int32_t cc_load(int32_t* p) { return __hip_atomic_load(p, CC_RLX_AGENT); }

// root of x's tree, p = a value read from parent[x]; halves the path on the way (x's
// parent := its grandparent), x's own pointer included, so that a vertex met again shows
// a parent nearer the root -- in the end the root, which is what lets most edges of a
// large component leave at the equal-parents test
__device__ __forceinline__ int32_t cc_find(int32_t* __restrict__ parent, int32_t x, int32_t p) {
  while (p != x) {
    const int32_t gp = cc_load(parent + p);
    if (gp == p) return p;
    __hip_atomic_store(parent + x, gp, CC_RLX_AGENT);
    x = gp;
    p = cc_load(parent + x);
  }
  return x;
}

// join the trees of u and w; a, b = values read from parent[u], parent[w]
__device__ __forceinline__ void cc_link(int32_t* __restrict__ parent, int32_t u, int32_t a, int32_t w, int32_t b) {
  while (true) {
    const int32_t ru = cc_find(parent, u, a), rw = cc_find(parent, w, b);
    if (ru == rw) return;
    const int32_t hi = ru > rw ? ru : rw, lo = ru > rw ? rw : ru;
    int32_t expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, CC_RLX_AGENT)) return;
    u = hi;   // hi was linked meanwhile: go on from its new parent (< hi)
    a = expect;
    w = lo;
    b = cc_load(parent + lo);
  }
}

// One edge: skipped early when it is a self-loop or both endpoints already show the same
// parent.
__device__ __forceinline__ void cc_union(int32_t* __restrict__ parent, int32_t u, int32_t w) {
  if (u == w) return;
  const int32_t a = cc_load(parent + u), b = cc_load(parent + w);
  if (a != b) cc_link(parent, u, a, w, b);
}

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
  GRID_STRIDE(v, V) {
    int32_t x = (int32_t)v, p = parent[x];
    while (p != x) {
      x = p;
      p = parent[x];
    }
    comp[v] = x;
  }
}

// size[c] += 1 for every member; block-aggregated (the giant component is one counter)
__global__ __launch_bounds__(256) void k_cc_sizes(const int32_t* __restrict__ comp, int64_t V,
                                                  unsigned long long* __restrict__ size) {
  __shared__ u32 bk[dev::kBhSlots];
  __shared__ unsigned long long bv[dev::kBhSlots];
  __shared__ int bsat;
  dev::BlockHist<unsigned long long> bh{bk, bv, &bsat};
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
__global__ __launch_bounds__(256) void k_cc_summary(const int32_t* __restrict__ comp,
                                                    const unsigned long long* __restrict__ size, int64_t V,
                                                    unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long ws[3][4];
  unsigned long long n = 0, n1 = 0, best = 0;
  GRID_STRIDE(v, V) {
    if (comp[v] == (int32_t)v) {
      const unsigned long long sz = size[v];
      n += 1;
      n1 += sz == 1ull ? 1ull : 0ull;
      best = dev::umax64(best, (sz << 32) | (unsigned long long)(0xFFFFFFFFu - (u32)v));
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

struct Tmp {   // stream-ordered temporaries of one call
  hipStream_t s;
  void* ptrs[4];
  int n = 0;
  explicit Tmp(hipStream_t st) : s(st) {}
  int get(void** p, size_t bytes) {
    LPA_TRY(tmp_alloc(p, bytes, s));
    ptrs[n++] = *p;
    return LPA_OK;
  }
  ~Tmp() {
    for (int i = 0; i < n; ++i) tmp_free(ptrs[i], s);
  }
};

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
  unsigned long long *size = nullptr, *acc = nullptr;
  LPA_TRY(tmp.get((void**)&parent, sizeof(int32_t) * (size_t)V));
  if (!out_is_device) LPA_TRY(tmp.get((void**)&comp, sizeof(int32_t) * (size_t)V));
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
  unsigned long long h[3] = {0, 0, 0};
  if (size_out || summary) {
    size = reinterpret_cast<unsigned long long*>(size_out);
    if (!size_out || !out_is_device) LPA_TRY(tmp.get((void**)&size, sizeof(unsigned long long) * (size_t)V));
    LPA_HIP(hipMemsetAsync(size, 0, sizeof(unsigned long long) * (size_t)V, s));
    hipLaunchKernelGGL(k_cc_sizes, dim3(grid_bh(V)), dim3(256), 0, s, comp, V, size);
    LPA_HIP(hipGetLastError());
    if (summary) {
      LPA_TRY(tmp.get((void**)&acc, sizeof(h)));
      LPA_HIP(hipMemsetAsync(acc, 0, sizeof(h), s));
      hipLaunchKernelGGL(k_cc_summary, dim3(grid_bh(V)), dim3(256), 0, s, comp, size, V, acc);
      LPA_HIP(hipGetLastError());
      LPA_HIP(hipMemcpyAsync(h, acc, sizeof(h), hipMemcpyDeviceToHost, s));
    }
  }
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
