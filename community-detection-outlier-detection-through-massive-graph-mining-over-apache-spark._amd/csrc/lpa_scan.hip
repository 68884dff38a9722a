// SCAN structural clustering (Xu, Yuruk, Feng, Schweiger, KDD 2007) of the canonical simple
// undirected graph of the handle's input multigraph: clusters of cores, their borders, and the
// non-members split into hubs and outliers.  include/lpa.h states the definition.
//
//   build    tc_build (lpa_tc.hip): simple edges, degrees d[], rank orientation, the oriented
//            CSR rp[] / col[] with ascending out-lists and the row lists of the four forms; with
//            common_out also the sorted canonical keys and every slot's canonical index
//   support  sup[i] = c(u, v) of the oriented edge in slot i.  For every oriented edge u -> v,
//            every w in N+(u) n N+(v) closes a triangle (met exactly once: lpa_tc.hip's
//            orientation argument) and adds 1 to the slots of u -> v, u -> w and v -> w; all
//            three positions are known at the match
//   flat     over the E slots / the V vertices: the similarity bit and nsim, the core flags,
//            union-find over similar core-core edges (lpa_uf.h: the larger root under the
//            smaller, so a cluster's root is its smallest core), flatten, borders by atomicMin
//            of the adjacent cores' labels, the smallest and largest member label around every
//            non-member by atomicMin / atomicMax (hub iff min < max), the counters
//   rows     common_out[i]: binary search of input row i's (min, max) key in the canonical keys
//
// Support kernels, by out-list length L, the forms and boundaries of lpa_tc.hip (lpa_graph::
// tc_short / tc_wave / tc_lds): group, wave with LDS, block with LDS, block over global memory.
// In the team forms the chunk's T apex edges u -> v each own an LDS counter: a match adds there,
// and after the chunk every edge takes one device atomic for the team's sum.  The other two
// edges of a match take a device atomic each.  A group row has at most tc_short entries and a
// lane's successive items belong to different edges: three device atomics per match.
// A block's LDS holds the T counters beside the list, so a list above kTcLdsMax - 256 entries
// is searched in global memory even where tc_lds would have staged it.
//
// Every accumulation is a 32-bit (support, nsim) or 64-bit (counters) INTEGER atomic add, min
// or max: they commute and associate, so every interleaving leaves the same bits.  The only
// floating-point work is the three products of the similarity test, each rounded once
// (contraction off: no fused multiply-add), the same operations numpy performs.
#include "lpa_device.h"
#include "lpa_algo.h"
#include "lpa_tc.h"
#include "lpa_uf.h"

#pragma clang fp contract(off)

namespace lpa {

namespace {

constexpr int32_t kNoLabel = 0x7FFFFFFF;

// G lanes per row (256 / G rows per block).  Items: the ordered pairs (v, w) of N+(u).
template <int G>
__global__ __launch_bounds__(256) void k_scan_group(const int32_t* __restrict__ rows, int64_t nrows,
                                                    const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                    int32_t* __restrict__ sup) {
  constexpr int kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < nrows; base += (int64_t)gridDim.x * kRows) {
    const int64_t r = base + threadIdx.x / G;
    if (r >= nrows) continue;
    const int32_t u = rows[r];
    const int64_t ub = rp[u];
    const int64_t L = rp[u + 1] - ub;
    const int64_t n = L * (L - 1);
    for (int64_t t = sub; t < n; t += G) {
      const int64_t j = t / (L - 1);
      int64_t k = t - j * (L - 1);
      k += k >= j ? 1 : 0;
      const int32_t v = col[ub + j], w = col[ub + k];
      const int64_t vb = rp[v];
      const int32_t p = tc_pos(col + vb, (int32_t)(rp[v + 1] - vb), w);
      if (p >= 0) {
        atomicAdd(&sup[ub + j], 1);
        atomicAdd(&sup[ub + k], 1);
        atomicAdd(&sup[vb + p], 1);
      }
    }
  }
}

// LDS of one team, in 8-byte words: lpa_tc.h's rpv[T], pre[T + 2], then acc[T] (the chunk's
// apex-edge counters), then nu[cap]
template <int T>
constexpr int64_t scan_team_words(int64_t cap) { return tc_team_words<T>(cap) + T / 2; }

// A team of T lanes (a wave, or the block of 256) per row u: k_tc_team's walk.  kLds: N+(u) is
// staged in the team's LDS region (L <= cap); otherwise it is searched in col[] (any length).
template <int T, bool kLds>
__global__ __launch_bounds__(256) void k_scan_team(const int32_t* __restrict__ rows, int64_t nrows,
                                                   const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                   int32_t* __restrict__ sup, int32_t cap) {
  static_assert(T == 64 || T == 256, "a wave or the block");
  extern __shared__ ull scan_smem[];
  __shared__ int32_t wsum[4];
  constexpr int kTeams = 256 / T;
  const int team = threadIdx.x / T, tl = threadIdx.x % T, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  ull* region = scan_smem + (int64_t)team * scan_team_words<T>(kLds ? cap : 0);
  int64_t* rpv = reinterpret_cast<int64_t*>(region);
  int32_t* pre = reinterpret_cast<int32_t*>(region + T);
  int32_t* acc = pre + (T + 2);
  int32_t* nu = acc + T;
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
      acc[tl] = 0;
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
        const int64_t xs = rpv[c] + (t - pre[c]);   // the slot of v -> x
        const int32_t x = col[xs];
        const int32_t k = kLds ? tc_pos(nu, L, x) : tc_pos(gu, L, x);
        if (k >= 0) {
          atomicAdd(&acc[c], 1);   // LDS: u -> v
          atomicAdd(&sup[ub + k], 1);
          atomicAdd(&sup[xs], 1);
        }
      }
      tc_team_sync<T>();   // the chunk's counters are final; rpv / pre / nu may be rewritten
      // lane tl alone reads acc[tl] here and clears it in the next chunk
      const int32_t a = acc[tl];
      if (a) atomicAdd(&sup[ub + c0 + tl], a);   // a > 0: list tl of the chunk is not empty
    }
  }
}

template <int T, bool kLds>
int launch_scan_team(const int32_t* rows, int64_t nrows, const int64_t* rp, const int32_t* col, int32_t* sup,
                     int32_t cap, hipStream_t s) {
  if (nrows == 0) return LPA_OK;
  const size_t bytes = sizeof(ull) * (size_t)((256 / T) * scan_team_words<T>(kLds ? cap : 0));
  if (bytes > (size_t)64 * 1024) {   // the caller keeps every launch below
    set_error("scan: %zu bytes of LDS per block", bytes);
    return LPA_EINVAL;
  }
  hipLaunchKernelGGL((k_scan_team<T, kLds>), dim3(grid_rows(nrows, 256 / T, 16384)), dim3(256), bytes, s, rows, nrows,
                     rp, col, sup, cap);
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

// ek: the E oriented keys, sorted.  simb[i] = the edge of slot i is similar; nsim[] += 1 at both
// ends -- the `to` side one atomic per similar edge, the `from` side one per run of equal `from`
// inside a wave (k_tc_degrees' fold: the run's similar edges are the set bits of a ballot).
// acc[0] += the supports (3 per triangle), acc[1] += the similar edges.
__global__ __launch_bounds__(256) void k_scan_similar(const u64* __restrict__ ek, const int32_t* __restrict__ sup,
                                                      const int32_t* __restrict__ d, int64_t E, double ee,
                                                      uint8_t* __restrict__ simb, int32_t* __restrict__ nsim,
                                                      ull* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  ull ssum = 0, nsimilar = 0;
  BLOCK_STRIDE(b, E) {
    const int64_t i = b + threadIdx.x;
    const bool act = i < E;
    const u64 k = act ? ek[i] : ~0ull;
    const u32 from = (u32)(k >> 32), to = (u32)k;   // 0xFFFFFFFF on an idle lane: no vertex
    bool sim = false;
    if (act) {
      const int32_t c = sup[i];
      const double a = (double)(c + 2);
      const double lhs = a * a;
      const double dd = (double)(d[from] + 1) * (double)(d[to] + 1);
      const double rhs = ee * dd;
      sim = lhs >= rhs;
      simb[i] = sim ? 1 : 0;
      ssum += (ull)c;
      if (sim) atomicAdd(&nsim[to], 1);
    }
    const u64 sb = __ballot(sim);
    const u32 prev = (u32)__shfl_up((int)from, 1, 64);
    const bool head = act && (lane == 0 || prev != from);
    const u64 heads = __ballot(head);
    const int nact = __popcll(__ballot(act));   // the active lanes are lanes [0, nact)
    if (head) {
      const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
      const int end = above ? lane + 1 + (__ffsll((ull)above) - 1) : nact;
      const u64 run = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
      const int n = __popcll(sb & run);
      if (n) atomicAdd(&nsim[from], n);
    }
    if (lane == 0) nsimilar += (ull)__popcll(sb);
  }
  for (int off = 32; off > 0; off >>= 1) ssum += __shfl_xor(ssum, off, 64);
  if (lane == 0) {
    if (ssum) atomicAdd(&acc[0], ssum);
    if (nsimilar) atomicAdd(&acc[1], nsimilar);
  }
}

__global__ __launch_bounds__(256) void k_scan_cores(const int32_t* __restrict__ nsim, int64_t V, int32_t mu,
                                                    uint8_t* __restrict__ core, int32_t* __restrict__ parent) {
  GRID_STRIDE(v, V) {
    core[v] = (int64_t)nsim[v] + 1 >= (int64_t)mu ? 1 : 0;
    parent[v] = (int32_t)v;
  }
}

__global__ __launch_bounds__(256) void k_scan_union(const u64* __restrict__ ek, const uint8_t* __restrict__ simb,
                                                    const uint8_t* __restrict__ core, int64_t E,
                                                    int32_t* __restrict__ parent) {
  GRID_STRIDE(i, E) {
    if (!simb[i]) continue;
    const u64 k = ek[i];
    const int32_t a = (int32_t)(k >> 32), b = (int32_t)(u32)k;
    if (core[a] && core[b]) cc_union(parent, a, b);
  }
}

// after the union kernel's end: a core's label is its root, the smallest core of its cluster
__global__ __launch_bounds__(256) void k_scan_flatten(const int32_t* __restrict__ parent,
                                                      const uint8_t* __restrict__ core, int64_t V,
                                                      int32_t* __restrict__ label) {
  GRID_STRIDE(v, V) label[v] = core[v] ? cc_root(parent, (int32_t)v) : kNoLabel;
}

// a non-core end of a similar edge to a core takes the smallest such core's label (the cores'
// labels are final and not written here)
__global__ __launch_bounds__(256) void k_scan_attach(const u64* __restrict__ ek, const uint8_t* __restrict__ simb,
                                                     const uint8_t* __restrict__ core, int64_t E,
                                                     int32_t* __restrict__ label) {
  GRID_STRIDE(i, E) {
    if (!simb[i]) continue;
    const u64 k = ek[i];
    const int32_t a = (int32_t)(k >> 32), b = (int32_t)(u32)k;
    const bool ca = core[a] != 0, cb = core[b] != 0;
    if (ca && !cb) atomicMin(&label[b], label[a]);
    if (cb && !ca) atomicMin(&label[a], label[b]);
  }
}

// role: 3 core, 2 border, 0 non-member (label[v] = v; lo / hi preset for k_scan_span)
__global__ __launch_bounds__(256) void k_scan_roles(const uint8_t* __restrict__ core, int64_t V,
                                                    int32_t* __restrict__ label, uint8_t* __restrict__ role,
                                                    int32_t* __restrict__ lo, int32_t* __restrict__ hi) {
  GRID_STRIDE(v, V) {
    const bool member = label[v] != kNoLabel;
    role[v] = core[v] ? 3 : member ? 2 : 0;
    if (!member) label[v] = (int32_t)v;
    lo[v] = kNoLabel;
    hi[v] = -1;
  }
}

// every simple edge between a non-member and a member: the member's label onto the non-member
__global__ __launch_bounds__(256) void k_scan_span(const u64* __restrict__ ek, int64_t E,
                                                   const uint8_t* __restrict__ role, const int32_t* __restrict__ label,
                                                   int32_t* __restrict__ lo, int32_t* __restrict__ hi) {
  GRID_STRIDE(i, E) {
    const u64 k = ek[i];
    const int32_t a = (int32_t)(k >> 32), b = (int32_t)(u32)k;
    const bool ma = role[a] >= 2, mb = role[b] >= 2;
    if (ma == mb) continue;
    const int32_t x = ma ? b : a, l = label[ma ? a : b];   // a member's label is final
    atomicMin(&lo[x], l);
    atomicMax(&hi[x], l);
  }
}

__global__ __launch_bounds__(256) void k_scan_hubs(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                   int64_t V, uint8_t* __restrict__ role) {
  GRID_STRIDE(v, V) {
    if (role[v] == 0 && lo[v] < hi[v]) role[v] = 1;
  }
}

// acc[2 + r] vertices of role r, acc[6] clusters, acc[7] max of (size << 32 | 0xFFFFFFFF - label)
// over the clusters: the largest, the smallest label among equals.  size[l]: vertices of label l
__global__ __launch_bounds__(256) void k_scan_summary(const uint8_t* __restrict__ role,
                                                      const int32_t* __restrict__ label, const ull* __restrict__ size,
                                                      int64_t V, ull* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  ull n[5] = {0, 0, 0, 0, 0}, best = 0;
  BLOCK_STRIDE(b, V) {
    const int64_t v = b + threadIdx.x;
    const int r = v < V ? (int)role[v] : -1;
    const bool head = r == 3 && label[v] == (int32_t)v;
#pragma unroll
    for (int k = 0; k < 4; ++k) n[k] += (ull)__popcll(__ballot(r == k));
    n[4] += (ull)__popcll(__ballot(head));
    if (head) best = dev::umax64(best, (size[v] << 32) | (ull)(0xFFFFFFFFu - (u32)v));
  }
  for (int off = 32; off > 0; off >>= 1) best = dev::umax64(best, __shfl_xor(best, off, 64));
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (n[k]) atomicAdd(&acc[2 + k], n[k]);
    if (best) atomicMax(&acc[7], best);
  }
}

// csup[canonical index] = the support of its slot
__global__ __launch_bounds__(256) void k_scan_canon(const int32_t* __restrict__ sup, const u64* __restrict__ canon,
                                                    int64_t E, int32_t* __restrict__ csup) {
  GRID_STRIDE(i, E) csup[canon[i]] = sup[i];
}

// common[i] of input row i: its (min, max) key searched in the E sorted canonical keys
__global__ __launch_bounds__(256) void k_scan_rows(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                   int64_t m, u32 V, const u64* __restrict__ ckeys,
                                                   const int32_t* __restrict__ csup, int64_t E,
                                                   int32_t* __restrict__ common) {
  GRID_STRIDE(i, m) {
    const u32 a = (u32)__builtin_nontemporal_load(src + i), b = (u32)__builtin_nontemporal_load(dst + i);
    const u32 mn = a < b ? a : b, mx = a < b ? b : a;
    int32_t c = -1;
    if (mn != mx && mx < V) {
      const u64 key = ((u64)mn << 32) | mx;
      int64_t l = 0, h = E;
      while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (ckeys[mid] < key) l = mid + 1;
        else h = mid;
      }
      if (l < E && ckeys[l] == key) c = csup[l];
    }
    common[i] = c;
  }
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream and the tc_* boundaries of the handle, nothing of
// the LPA state; every array is a stream-ordered temporary.
int scan(lpa_graph* g, double eps, int32_t mu, int32_t* label_out, uint8_t* role_out, int32_t* nsim_out,
         int32_t* common_out, int32_t out_is_device, lpa_scan_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V, m = g->m;
  if (summary) *summary = lpa_scan_summary{0, 0, 0, 0, 0, 0, 0, 0, 0, -1};
  if (V == 0) return LPA_OK;
  Tmp tmp(s);
  int32_t *label = label_out, *nsim = nsim_out, *common = common_out;
  uint8_t* role = role_out;
  if (!out_is_device) {
    LPA_TRY(tmp.get(&label, V));
    LPA_TRY(tmp.get(&role, V));
    if (common_out) LPA_TRY(tmp.get(&common, m));
  }
  if (!out_is_device || !nsim_out) LPA_TRY(tmp.get(&nsim, V));
  int32_t *d = nullptr, *parent = nullptr, *lo = nullptr, *hi = nullptr, *sup = nullptr;
  uint8_t *core = nullptr, *simb = nullptr;
  ull* acc = nullptr;
  LPA_TRY(tmp.get(&d, V));
  LPA_TRY(tmp.get(&parent, V));
  LPA_TRY(tmp.get(&lo, V));
  LPA_TRY(tmp.get(&hi, V));
  LPA_TRY(tmp.get(&core, V));
  LPA_TRY(tmp.get(&acc, 8));
  LPA_HIP(hipMemsetAsync(d, 0, sizeof(int32_t) * (size_t)V, s));
  LPA_HIP(hipMemsetAsync(nsim, 0, sizeof(int32_t) * (size_t)V, s));
  LPA_HIP(hipMemsetAsync(acc, 0, sizeof(ull) * 8, s));
  TcLists t;
  LPA_TRY(tc_build(g, tmp, d, common_out != nullptr, &t));
  const int64_t E = t.E;
  if (E > 0) {
    LPA_TRY(tmp.get(&sup, E));
    LPA_TRY(tmp.get(&simb, E));
    LPA_HIP(hipMemsetAsync(sup, 0, sizeof(int32_t) * (size_t)E, s));
    if (t.rows[0]) {
      hipLaunchKernelGGL(k_scan_group<8>, dim3(grid_rows(t.rows[0], 32, 16384)), dim3(256), 0, s, t.lists,
                         (int64_t)t.rows[0], t.rp, t.col, sup);
      LPA_HIP(hipGetLastError());
    }
    const int32_t wcap = t.lmax < g->tc_wave ? t.lmax : g->tc_wave;
    const int32_t bcap = t.lmax < g->tc_lds ? t.lmax : g->tc_lds;
    LPA_TRY((launch_scan_team<64, true>(t.lists + V, t.rows[1], t.rp, t.col, sup, wcap, s)));
    if (bcap <= kTcLdsMax - 256)
      LPA_TRY((launch_scan_team<256, true>(t.lists + 2 * V, t.rows[2], t.rp, t.col, sup, bcap, s)));
    else   // the counters leave no room for so long a list
      LPA_TRY((launch_scan_team<256, false>(t.lists + 2 * V, t.rows[2], t.rp, t.col, sup, 0, s)));
    LPA_TRY((launch_scan_team<256, false>(t.lists + 3 * V, t.rows[3], t.rp, t.col, sup, 0, s)));
    hipLaunchKernelGGL(k_scan_similar, dim3(grid_bh(E)), dim3(256), 0, s, t.ek, sup, d, E, eps * eps, simb, nsim, acc);
    LPA_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_scan_cores, dim3(grid_for(V)), dim3(256), 0, s, nsim, V, mu, core, parent);
  if (E > 0) hipLaunchKernelGGL(k_scan_union, dim3(grid_for(E)), dim3(256), 0, s, t.ek, simb, core, E, parent);
  hipLaunchKernelGGL(k_scan_flatten, dim3(grid_for(V)), dim3(256), 0, s, parent, core, V, label);
  if (E > 0) hipLaunchKernelGGL(k_scan_attach, dim3(grid_for(E)), dim3(256), 0, s, t.ek, simb, core, E, label);
  hipLaunchKernelGGL(k_scan_roles, dim3(grid_for(V)), dim3(256), 0, s, core, V, label, role, lo, hi);
  if (E > 0) hipLaunchKernelGGL(k_scan_span, dim3(grid_for(E)), dim3(256), 0, s, t.ek, E, role, label, lo, hi);
  hipLaunchKernelGGL(k_scan_hubs, dim3(grid_for(V)), dim3(256), 0, s, lo, hi, V, role);
  LPA_HIP(hipGetLastError());
  ull h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (summary) {
    ull* size = nullptr;
    ull unused[3];
    LPA_TRY(comp_sizes(tmp, label, V, nullptr, 0, false, &size, unused));   // label[label[v]] == label[v]
    hipLaunchKernelGGL(k_scan_summary, dim3(grid_bh(V)), dim3(256), 0, s, role, label, size, V, acc);
    LPA_HIP(hipGetLastError());
    LPA_HIP(hipMemcpyAsync(h, acc, sizeof(h), hipMemcpyDeviceToHost, s));
  }
  if (common_out && m > 0) {
    int32_t* csup = nullptr;
    LPA_TRY(tmp.get(&csup, E));
    if (E > 0) hipLaunchKernelGGL(k_scan_canon, dim3(grid_for(E)), dim3(256), 0, s, sup, t.canon, E, csup);
    hipLaunchKernelGGL(k_scan_rows, dim3(grid_for(m)), dim3(256), 0, s, g->e_src, g->e_dst, m, (u32)V, t.ckeys, csup, E,
                       common);
    LPA_HIP(hipGetLastError());
  }
  if (!out_is_device) {
    LPA_HIP(hipMemcpyAsync(label_out, label, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipMemcpyAsync(role_out, role, sizeof(uint8_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    if (nsim_out) LPA_HIP(hipMemcpyAsync(nsim_out, nsim, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    if (common_out && m > 0)
      LPA_HIP(hipMemcpyAsync(common_out, common, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
  }
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->simple_edges = E;
    summary->triangles = (int64_t)(h[0] / 3ull);
    summary->similar_edges = (int64_t)h[1];
    summary->n_outliers = (int64_t)h[2];
    summary->n_hubs = (int64_t)h[3];
    summary->n_borders = (int64_t)h[4];
    summary->n_cores = (int64_t)h[5];
    summary->n_clusters = (int64_t)h[6];
    summary->largest_cluster = (int64_t)(h[7] >> 32);
    summary->largest_cluster_label = h[7] ? (int64_t)(0xFFFFFFFFu - (u32)h[7]) : -1;
  }
  return LPA_OK;
}

}  // namespace lpa
