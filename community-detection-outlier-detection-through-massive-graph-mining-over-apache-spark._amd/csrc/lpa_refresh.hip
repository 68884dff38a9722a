// The refresh stage of a superstep (lpa_iter.hip describes the whole superstep): the
// diff of the two label vectors, the al[] scatter with its frontier marks, the al[]
// rebuilds (plain, small, LDS hot set, class-blocked pieces), the giant label's pick and
// bits, the giant-code refresh, and their host schedule (launch_refresh and its callers'
// forms).
#include <algorithm>
#include <type_traits>

#include "lpa_codes.h"
#include "lpa_device.h"
#include "lpa_schedule.h"

namespace lpa {

using namespace dev;

namespace {

// ---------------------------------------------------------------------------
// refresh of the replicated neighbour labels al[]
// ---------------------------------------------------------------------------
// Scatter chunks: column u's al[] positions cpos[cptr[u] ..) are cut into chunks of
// kChunkPos, numbered statically at build time (chunks cch[u] .. cch[u+1] - 1,
// cowner[chunk] = u).  A changed column flags its chunks in the bytemap chflag[]
// (plain byte stores, no list to build); the scatter walks the bytemap.
__device__ __forceinline__ void flag_chunks(uint8_t* __restrict__ chflag, const int64_t* __restrict__ cch,
                                            int64_t u) {
  int64_t c = cch[u];
  const int64_t e = cch[u + 1];
  for (; c < e && (c & 15); ++c) chflag[c] = 1;  // hub columns: thousands of chunks,
  for (; c + 16 <= e; c += 16)                    // 16 flags per store
    *reinterpret_cast<uint4*>(chflag + c) = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
  for (; c < e; ++c) chflag[c] = 1;
}

// changed vertices of the slot range [s0, s1): a column with one scatter chunk (the
// vast majority) is appended to chlist[] (LDS queue, one atomic per block), a longer
// one flags its chunks in chflag[]; the dirty arcs are counted (one atomic per wave);
// with Lsync != nullptr the new label is also copied into Lc (the next superstep's
// output vector: frontier, a row the next superstep skips already holds its label
// there; inside the concurrent tally the scatter does it).  int4 quads (vpad is a
// multiple of 64), kDiffQuads per block; lanes outside the range masked (the
// neighbouring slots may belong to a bin another stream is still computing).
//
// Frontier superstep (lists != nullptr and *fr_all == 0): only the rows listed for
// bins [b0, b1) were re-tallied (every other row provably kept its label, and its
// output slot already holds it), so the diff walks those lists -- grid-stride over
// their concatenation -- instead of the slot range.
constexpr int kDiffQuads = 2048;
// counters[1] value that makes the refresh rebuild al[] (k_dense_decide)
constexpr unsigned long long kForcedRebuild = 1ull << 62;

// Label-dense supersteps (P = 1): the per-stream diffs only counted the changed slots.
// More than 1/10 of the slots changed: the refresh rebuilds al[] (counters[1] forced),
// so no position chunk is ever emitted; otherwise the full diff (mode 2) runs next.
// A superstep after a giant-code refresh (gword[GW_CODE]) always rebuilds: its al[] entries were
// never written for the rows that superstep settled from codes.
__global__ void k_dense_decide(unsigned long long* __restrict__ counters, int64_t n_slots,
                               const int32_t* __restrict__ gword) {
  if (threadIdx.x == 0 && ((int64_t)counters[2] * 10 > n_slots || gword[GW_CODE] != 0))
    counters[1] = kForcedRebuild;
}
// fcnt[] slot set by the row settle of a giant superstep (k_settle_*): the bin kernels
// walk lists of the unsettled rows, but the diff scans every slot (settled rows may
// have changed label)
__global__ __launch_bounds__(256) void k_diff(const int4* __restrict__ Lc4,
                                              const int4* __restrict__ Ln4, int32_t* __restrict__ Lsync,
                                              int64_t s0, int64_t s1,
                                              const int64_t* __restrict__ cptr,
                                              const int64_t* __restrict__ cch,
                                              uint8_t* __restrict__ chflag,
                                              int32_t* __restrict__ chlist,
                                              unsigned long long* __restrict__ counters,
                                              BinBounds bb, int b0, int b1,
                                              const int32_t* __restrict__ flist,
                                              const int32_t* __restrict__ fcnt,
                                              const int32_t* __restrict__ fr_all, int mode) {
  // mode 1 (label-dense supersteps): only count the changed slots (counters[2]); mode 2:
  // the full diff unless k_dense_decide already chose the rebuild (counters[1] forced)
  if (mode == 2 && counters[1] >= kForcedRebuild) return;
  if (mode == 1) {
    unsigned long long c = 0;
    const int64_t q0 = s0 / 4 + (int64_t)blockIdx.x * kDiffQuads;
    const int64_t q1 = min((s1 + 3) / 4, q0 + kDiffQuads);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
      const int4 a = Lc4[q], b = Ln4[q];
      int chg = (a.x != b.x) | ((a.y != b.y) << 1) | ((a.z != b.z) << 2) | ((a.w != b.w) << 3);
      if (q * 4 < s0 || q * 4 + 4 > s1) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (q * 4 + k < s0 || q * 4 + k >= s1) chg &= ~(1 << k);
      }
      c += (unsigned long long)__popc(chg);
    }
    // (the counts summed per block first: one atomic per block on the counter, not one
    // per wave -- the same-address atomics of ~8 K waves queue at the counter's channel)
    __shared__ unsigned long long csum;
    if (threadIdx.x == 0) csum = 0ull;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&csum, c);
    __syncthreads();
    if (threadIdx.x == 0 && csum) atomicAdd(&counters[2], csum);
    return;
  }
  __shared__ int32_t q_col[kDiffQuads * 4];
  __shared__ int qn;
  __shared__ unsigned long long base_s, dsum;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) {
    qn = 0;
    dsum = 0ull;
  }
  __syncthreads();
  unsigned long long dirty = 0;
  auto emit = [&](int64_t u, int32_t nb) {
    if (Lsync) Lsync[u] = nb;
    dirty += (unsigned long long)(cptr[u + 1] - cptr[u]);
    const int64_t nch = cch[u + 1] - cch[u];
    if (nch == 1) q_col[atomicAdd(&qn, 1)] = (int32_t)u;
    else if (nch > 1) flag_chunks(chflag, cch, u);
  };
  if (flist != nullptr && *fr_all == 0 && fcnt[kFcntSettled] == 0) {
    // a list holds at most its bin's rows, so the grid (sized for the slot range)
    // gives each thread <= 32 entries, inside the block's queue
    int64_t total = 0;
    for (int b = b0; b < b1; ++b) total += fcnt[b];
    const int32_t* Lc = reinterpret_cast<const int32_t*>(Lc4);
    const int32_t* Ln = reinterpret_cast<const int32_t*>(Ln4);
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
      int64_t acc = 0;
      int b = b0;
      while (v >= acc + fcnt[b]) acc += fcnt[b++];
      const int64_t u = flist[bb.b[b] + (v - acc)];
      const int32_t nb = Ln[u];
      if (Lc[u] != nb) emit(u, nb);
    }
  } else {
    const int64_t q0 = s0 / 4 + (int64_t)blockIdx.x * kDiffQuads;
    const int64_t q1 = min((s1 + 3) / 4, q0 + kDiffQuads);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
      const int4 a = Lc4[q], b = Ln4[q];
      int chg = (a.x != b.x) | ((a.y != b.y) << 1) | ((a.z != b.z) << 2) | ((a.w != b.w) << 3);
      if (q * 4 < s0 || q * 4 + 4 > s1) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (q * 4 + k < s0 || q * 4 + k >= s1) chg &= ~(1 << k);
      }
      if (chg) {
        const int32_t nb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((chg >> k) & 1) emit(q * 4 + k, nb[k]);
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) dirty += __shfl_xor(dirty, off, 64);
  if (lane == 0 && dirty) atomicAdd(&dsum, dirty);
  __syncthreads();
  if (threadIdx.x == 0 && dsum) atomicAdd(&counters[1], dsum);
  const int n = qn;
  if (n == 0) return;  // uniform
  if (threadIdx.x == 0) base_s = atomicAdd(&counters[0], (unsigned long long)n);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) chlist[base_s + i] = q_col[i];
}

// few changes: al[cpos[p]] = L_next[u] for the positions of each changed u.
// A chunk is (u << 32 | k): positions [cptr[u] + 256 k, ...).  A wave takes 64
// chunks, one per lane (independent loads of cptr and the label): chunks of <= 16
// positions are written by their own lane (4 stores in flight per step), longer
// ones by the whole wave (coalesced cpos).
// Frontier marks for the next superstep: the row holding arc position p (and, for a
// hub row, the 512-arc unit holding it) must be re-tallied.
struct FrontierMarks {
  const int32_t* crow;       // [arcs] row of each position
  const int64_t* rp;         // row offsets
  const int64_t* uoff;       // hub rows: first unit
  int64_t n_hub;
  uint8_t* rdirty;           // next parity
  uint8_t* udirty;           // next parity
  __device__ __forceinline__ void mark(int64_t p) const {
    const int32_t r = crow[p];
    rdirty[r] = 1;
    if (r < n_hub) udirty[uoff[r] + ((p - rp[r]) >> 9)] = 1;
  }
};
static_assert(kSegArcs == 512, "unit of a position: (p - rp[row]) >> 9");

// Wave-cooperative scatter of every lane's run: al[cpos[b + i]] = lab, i < n
// (n <= kChunkPos).  The runs are cut into 16-position pieces dealt over the wave's
// lanes (lane -> piece by a binary search over the inclusive piece prefix), so a
// wave whose lanes hold runs of 17..256 positions writes them in parallel instead of
// run after run with the whole wave.  Every lane of the wave must call it.
// clr (this lane's run): also clear the arc giant bits of its positions (a column that
// left G, superstep 3's scatter keeping the bits of the bits-mode rebuild: k_al_scatter)
__device__ __forceinline__ void scatter_runs(int64_t b, int n, int32_t lab, bool clr, const uint32_t* __restrict__ cpos,
                                             int32_t* __restrict__ al, bool all, const FrontierMarks& fm,
                                             unsigned long long* __restrict__ abits, int lane) {
  if (al == nullptr && all) return;  // gather mode without marks: nothing to write (uniform)
  const int k = (n + 15) >> 4;
  int incl = k;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  const int S = __shfl(incl, 63, 64);
  for (int r0 = 0; r0 < S; r0 += 64) {
    const int t = r0 + lane;
    int o = 0;  // the owner: first lane whose inclusive piece count exceeds t
#pragma unroll
    for (int st = 32; st >= 1; st >>= 1) {
      const int ic = __shfl(incl, o + st - 1, 64);
      if (ic <= t) o += st;
    }
    o = o < 64 ? o : 63;
    const int excl = __shfl(incl, o, 64) - __shfl(k, o, 64);
    const int64_t bo = __shfl(b, o, 64);
    const int no = __shfl(n, o, 64);
    const int32_t lv = __shfl(lab, o, 64);
    const bool cl = __shfl((int)clr, o, 64) != 0;
    if (t < S) {
      const int p0 = (t - excl) * 16;
      const int cnt = min(16, no - p0);
      const uint32_t* src = cpos + bo + p0;
      for (int q = 0; q < cnt; q += 4) {
        uint32_t p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = q + u < cnt ? src[q + u] : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (q + u < cnt) {
            if (al) al[p[u]] = lv;   // gather mode: marks only
            if (cl) atomicAnd(&abits[p[u] >> 6], ~(1ull << (p[u] & 63u)));
            if (!all) fm.mark(p[u]);
          }
      }
    }
  }
}

// al[i] = L[col[i]] over the whole arc array by the calling grid (grid-stride): each
// thread keeps 8 gathers in flight (two int4 column quads), col / al streamed
// non-temporally
__device__ __forceinline__ void rebuild_all(const int32_t* __restrict__ col, int64_t arcs,
                                            const int32_t* __restrict__ Ln, int32_t* __restrict__ al) {
  const int64_t n4 = arcs >> 2;
  const v4i* __restrict__ c4 = reinterpret_cast<const v4i*>(col);
  v4i* __restrict__ a4 = reinterpret_cast<v4i*>(al);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; q + stride < n4; q += 2 * stride) {
    const v4i c0 = __builtin_nontemporal_load(c4 + q);
    const v4i c1 = __builtin_nontemporal_load(c4 + q + stride);
    v4i r0, r1;
    r0.x = Ln[c0.x]; r0.y = Ln[c0.y]; r0.z = Ln[c0.z]; r0.w = Ln[c0.w];
    r1.x = Ln[c1.x]; r1.y = Ln[c1.y]; r1.z = Ln[c1.z]; r1.w = Ln[c1.w];
    __builtin_nontemporal_store(r0, a4 + q);
    __builtin_nontemporal_store(r1, a4 + q + stride);
  }
  if (q < n4) {
    const v4i c0 = __builtin_nontemporal_load(c4 + q);
    v4i r0;
    r0.x = Ln[c0.x]; r0.y = Ln[c0.y]; r0.z = Ln[c0.z]; r0.w = Ln[c0.w];
    __builtin_nontemporal_store(r0, a4 + q);
  }
  if (blockIdx.x == 0 && threadIdx.x < (arcs & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    al[i] = Ln[col[i]];
  }
}

// (defined with the fill-scatter form below)
__device__ __forceinline__ void sparse_mark(int32_t* __restrict__ gword, bool sparse, int32_t G);
__device__ __forceinline__ void fill_arc_bits(unsigned long long* __restrict__ abits, int32_t* __restrict__ al,
                                              int64_t arcs, int32_t G, int64_t nslots, int64_t tid, int64_t nth);

// fill3 (host-set in superstep 3's refresh alone, fill_step3_now; every other launch passes 0
// and does not read the word): gword[GW_FILL3] says that k_fill_decide's step-3 instance took the
// fill-scatter form.  This kernel then scatters nothing.  It does its housekeeping (the next
// counters, the chunk flags, *fr_all_next = 1), sets every arc bit, copies gbits_next over
// gbits and does the form's bookkeeping; k_fill_scatter follows in a launch of its own and
// writes the columns off the new G.  Four things hold this together:
//  - The fallback needs the OLD gbits: left_g below reads the bitmap of the vector the sparse
//    rebuild saw, so nothing writes gbits before this kernel has read gword[GW_FILL3], and the copy
//    happens only under it.
//  - The fill may not precede the decision (k_fill_decide's note): it is here, under the word.
//  - No block of one launch may clear a bit that another block of the same launch may still
//    fill: a taken form clears no bit in this launch at all, k_fill_scatter is the next one.
//  - A taken form writes no frontier mark and syncs no label into Lold.  That is valid only
//    because the next superstep writes every row: *fr_all_next = 1 here, and the host forces it
//    as well (settle3_now -> force_all_next, lpa_iter.hip run_supersteps).
// -DLPA_SPARSE_POISON: the fill poisons every al[] entry, as k_fill_decide's does.
__global__ __launch_bounds__(256) void k_al_scatter(const int32_t* __restrict__ chlist,
                                                    const uint4* __restrict__ chflag16, int64_t ngroups,
                                                    const int32_t* __restrict__ cowner,
                                                    const int64_t* __restrict__ cch,
                                                    const unsigned long long* __restrict__ counters,
                                                    unsigned long long* __restrict__ counters_next,
                                                    const int64_t* __restrict__ cptr,
                                                    const uint32_t* __restrict__ cpos,
                                                    const int32_t* __restrict__ Ln,
                                                    int32_t* __restrict__ al, int64_t thr,
                                                    FrontierMarks fm, int32_t* __restrict__ fr_all_next,
                                                    int frontier, int64_t fr_thr,
                                                    int32_t* __restrict__ Lold,
                                                    const int32_t* __restrict__ col_fold, int64_t arcs,
                                                    int32_t* __restrict__ gword, int keep_bits,
                                                    uint32_t* __restrict__ gbits,
                                                    unsigned long long* __restrict__ abits, int fill3 = 0,
                                                    const uint32_t* __restrict__ gbits_next = nullptr,
                                                    int64_t nslots = 0) {
  // the next superstep's counters (the other parity; no memset launch)
  if (blockIdx.x == 0 && threadIdx.x < 3) counters_next[threadIdx.x] = 0ull;
  // (uniform: no block of this launch writes gword[GW_FILL3])
  if (fill3 != 0 && gword[GW_FILL3] != 0) {
    const int32_t G = gword[GW_G3];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    if (tid == 0) {
      *fr_all_next = 1;
      // the sparse rebuild's bookkeeping, as k_fill_decide's after superstep 2; gword[GW_G] too, so that
      // the k_giant_pick that follows (the same pick) sees no new G and keeps gword[GW_ABITS_OK]
      gword[GW_G] = G;
      sparse_mark(gword, true, G);
      gword[GW_ABITS_OK] = 1;
      gword[GW_FILL_CNT] += 1;
    }
    fill_arc_bits(abits, al, arcs, G, nslots, tid, nth);
    // gbits = the bitmap of the vector this sparse refresh saw (nslots is a multiple of 64)
    {
      const unsigned long long* __restrict__ src = reinterpret_cast<const unsigned long long*>(gbits_next);
      unsigned long long* __restrict__ dst = reinterpret_cast<unsigned long long*>(gbits);
      for (int64_t i = tid; i < (nslots >> 6); i += nth) dst[i] = src[i];
    }
    // the changed columns' chunk flags (k_diff set them; the list needs no clearing)
    uint4* __restrict__ fl = const_cast<uint4*>(chflag16);
    for (int64_t gi = tid; gi < ngroups; gi += nth) {
      const uint4 f = chflag16[gi];
      if ((f.x | f.y | f.z | f.w) != 0u) fl[gi] = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  const bool rebuild = rebuild_wanted(counters, thr);
  // al changes here (scatter, or the plain folded rebuild), so the arc giant bits go
  // stale: gword[GW_ABITS_OK] = 0 -- except in superstep 3's scatter (keep_bits, host-set), right
  // after the bits-mode rebuild whose bits they are: a column that LEFT G (its gbits
  // bit, the rebuild's bitmap of the same vector and G) clears its positions' bits, one
  // atomic each (rare: R-MAT superstep 3 moves labels onto G); a column that joined G
  // leaves its bits clear.  The bits then hold a lower bound of every row's G votes, all
  // superstep 4's settle needs, and its k_abits_pass is skipped (round 6; exact upkeep
  // with an atomic per written position cost superstep 3 0.25 ms, round 3).  A wanted,
  // non-folded rebuild follows this kernel and sets gword[GW_ABITS_OK] itself.
  const bool keep = keep_bits != 0 && !rebuild;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (!rebuild || col_fold) && !keep) gword[GW_ABITS_OK] = 0;
  // A sparse al[] (gword[GW_AL_SPARSE], read before block 0 may clear it below: uniform over the
  // grid only while no rebuild is folded in, which is when it is used) keeps its invariant in
  // EVERY superstep: a changed column whose gbits bit is set (it held Gb when the sparse
  // rebuild ran) and whose new label is not Gb clears the bit of each of its positions and
  // writes al[] there; any other changed column writes al[] and leaves the bits alone (its
  // bits are clear already: a joiner ends with a clear bit and al = Gb).  Bits are only ever
  // cleared, so a repeated clear is harmless.
  const bool sparse = !rebuild && gword[GW_AL_SPARSE] != 0;
  const int32_t Gk = sparse ? gword[GW_AL_GB] : gword[GW_G];
  auto left_g = [&](int64_t u, int32_t lab) -> bool {
    return (keep || sparse) && lab != Gk && ((gbits[u >> 5] >> (u & 31)) & 1u);
  };
  // The next superstep tallies every row after a rebuild, with the frontier off, or
  // when more than fr_thr arcs changed: then nearly every row has a changed neighbour
  // anyway (R-MAT superstep 3 -> 4: 1.5 % of arcs dirty, 88 % of the arcs in dirty
  // rows) and the per-position marks would cost more than they save.
  const bool all = rebuild || !frontier || (int64_t)counters[1] > fr_thr;
  if (blockIdx.x == 0 && threadIdx.x == 0) *fr_all_next = all ? 1 : 0;
  const int lane = threadIdx.x & 63;
  const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // col_fold (captured converged supersteps): a wanted rebuild is done here, the plain
  // form, instead of by a k_al_rebuild_hot launch that nearly always returns at once
  // (one dependent launch fewer per converged superstep)
  if (rebuild && col_fold) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      gword[GW_AL_SPARSE] = 0;  // a dense al[] again
      gword[GW_FILL] = 0;
    }
    rebuild_all(col_fold, arcs, Ln, al);
  }
  // one-chunk columns from the list: a lane each, longer rows of positions by the wave
  if (!rebuild) {
    const int64_t nl = (int64_t)counters[0];
    for (int64_t c0 = wid * 64; c0 < nl; c0 += nw * 64) {
      const int64_t c = c0 + lane;
      int64_t b = 0;
      int n = 0;
      int32_t lab = 0;
      bool clr = false;
      if (c < nl) {
        const int64_t u = chlist[c];
        b = cptr[u];
        n = (int)(cptr[u + 1] - b);  // <= kChunkPos
        lab = Ln[u];
        Lold[u] = lab;  // frontier sync (after the join)
        clr = left_g(u, lab);
      }
      scatter_runs(b, n, lab, clr, cpos, al, all, fm, abits, lane);
    }
  }
  uint4* __restrict__ flw = const_cast<uint4*>(chflag16);
  // multi-chunk columns: a wave takes 64 groups of 16 chunk flags, one group per lane,
  // and clears them.  Lane l of wave w takes group g0 + l * nw + w: the consecutive
  // chunks of one changed hub column land in different waves (wave-consecutive
  // groups would hand a column's hundreds of chunks to one wave, one after another)
  for (int64_t g0 = 0; g0 < ngroups; g0 += nw * 64) {
    const int64_t gi = g0 + (int64_t)lane * nw + wid;
    uint4 f = make_uint4(0u, 0u, 0u, 0u);
    if (gi < ngroups) f = chflag16[gi];
    const bool any = (f.x | f.y | f.z | f.w) != 0u;
    if (any) flw[gi] = make_uint4(0u, 0u, 0u, 0u);
    if (rebuild || __ballot(any) == 0ull) continue;  // the rebuild re-gathers every arc
    u32 bits = 0u;
    const u32 fw[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if ((fw[k >> 2] >> (8 * (k & 3))) & 0xFFu) bits |= 1u << k;
    // every lane pops its next flagged chunk per round: chunks of <= 16 positions are
    // written by their own lane, longer ones by the whole wave (coalesced cpos)
    while (__ballot(bits != 0u)) {
      int64_t b = 0;
      int n = 0;
      int32_t lab = 0;
      bool clr = false;
      if (bits) {
        const int t = __ffs(bits) - 1;
        bits &= bits - 1u;
        const int64_t cid = gi * 16 + t;
        const int64_t u = cowner[cid];
        const int64_t kk = cid - cch[u];
        b = cptr[u] + kk * kChunkPos;
        n = (int)min((int64_t)kChunkPos, cptr[u + 1] - b);
        lab = Ln[u];
        // frontier sync of a changed label into the next superstep's output vector
        // (after the join; every changed vertex with local arcs has a chunk 0)
        if (kk == 0) Lold[u] = lab;
        clr = left_g(u, lab);
      }
      scatter_runs(b, n, lab, clr, cpos, al, all, fm, abits, lane);
    }
  }
}

// After a lazy reset (al0) the first refresh that only scatters needs the L0 arc
// labels in al first: copied here unless the rebuild that follows rewrites every arc.
__global__ __launch_bounds__(256) void k_al_fill_unless_rebuild(const unsigned long long* __restrict__ counters,
                                                                int64_t thr, const v4i* __restrict__ src,
                                                                v4i* __restrict__ dst, int64_t arcs) {
  if (rebuild_wanted(counters, thr)) return;
  const int64_t n4 = arcs >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x)
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + q), dst + q);
  if (blockIdx.x == 0 && threadIdx.x < (arcs & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    reinterpret_cast<int32_t*>(dst)[i] = reinterpret_cast<const int32_t*>(src)[i];
  }
}

// many changes: al[i] = L_next[col[i]].  Random label gathers: each thread
// keeps 8 gathers in flight (two int4 column quads), streams col/al non-temporally.
template <bool kIfWanted>
__global__ __launch_bounds__(256) void k_al_rebuild(const unsigned long long* __restrict__ counters,
                                                    int64_t thr, const int32_t* __restrict__ col,
                                                    int64_t arcs,
                                                    const int32_t* __restrict__ Ln,
                                                    int32_t* __restrict__ al, int32_t* __restrict__ gword) {
  if (kIfWanted && !rebuild_wanted(counters, thr)) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gword[GW_ABITS_OK] = 0;   // no arc giant bits from this form
    gword[GW_AL_SPARSE] = 0;  // ... and a dense al[]
    gword[GW_FILL] = 0;
  }
  rebuild_all(col, arcs, Ln, al);
}

// Giant-label bitmap of L (before a rebuild): bit u = (L[u] == G), G = L[0], the label
// of the highest-degree vertex.  Once the labels concentrate (R-MAT, after superstep
// 2: ~98.5 % of the arcs point at a column labelled G) the rebuild gathers one BIT per
// arc -- the hot slots' bits from LDS, the rest from this 1-bit-per-slot array, which
// stays in L2 (2 MB at C3 against the 64 MB label vector) -- and reads the label
// vector only for the columns whose bit is clear.  One ballot per 64 slots; lanes
// 0..7 store the wave's eight 64-bit words (64 contiguous bytes).
// The giant-label candidate of a label vector: the most frequent label among the
// kPickK highest-degree vertices (degree ranks k < kPickK; at P > 1 rank k lives at slot
// (k mod P) S + k / P), and whether it holds >= 1/5 of them (gword[GW_TRY]: the tallies'
// giant step is worth trying).  On R-MAT and Chung-Lu (oracle, scale 21-22) that label
// is the degree-weighted mode of the whole vector in every superstep -- the top hub's
// own label is not (Chung-Lu superstep 2: the mode holds 43 % of the arcs' columns, the
// top hub's label 0.3 %).  One block, a 2K-slot LDS table.  The choice of G only
// affects speed: every use of it is exact for any G.
constexpr int kHotLabels = kHotRankedLabels;  // rank-strided label set (P > 1: power-of-two shares)
constexpr int kHotLabelsSingle = 40960;    // P = 1: the whole 160 KB of LDS
// bits mode: 1,310,688 slots' bits (the last LDS word counts the set bits first)
constexpr int64_t kHotBits = 32ll * (kHotLabelsSingle - 1);
constexpr int kPickK = 1024;
// -> thread 0: the best table word (count << 32 | ~label) of the n = min(n_real, kPickK) top slots
__device__ __forceinline__ u64 giant_pick_best(const int32_t* __restrict__ L, int64_t n, int64_t S, int P) {
  __shared__ u64 tab[2 * kPickK];
  __shared__ u64 wbest[kPickK / 64];
  const int t = threadIdx.x;
  tab[t] = 0ull;
  tab[t + kPickK] = 0ull;
  __syncthreads();
  if (t < n) lds_insert(tab, 32 - 11, 2 * kPickK - 1, (u32)L[(int64_t)(t % P) * S + t / P], 1u);
  __syncthreads();
  const u64 b = wave_max_u64(umax64(tab[t], tab[t + kPickK]));
  if ((t & 63) == 0) wbest[t >> 6] = b;
  __syncthreads();
  u64 m = 0ull;
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < kPickK / 64; ++k) m = umax64(m, wbest[k]);
  }
  return m;
}
__global__ __launch_bounds__(1024) void k_giant_pick(const int32_t* __restrict__ L, int64_t n_real, int64_t S,
                                                     int P, int32_t* __restrict__ gword) {
  const int64_t n = n_real < kPickK ? n_real : kPickK;
  const u64 m = giant_pick_best(L, n, S, P);
  if (threadIdx.x == 0) {
    const int32_t G = (int32_t)(~(u32)m);
    if (G != gword[GW_G]) gword[GW_ABITS_OK] = 0;  // the arc giant bits are relative to the old G
    gword[GW_G] = G;
    gword[GW_HOT_BITS] = 0;  // k_giant_bits counts the set bits of the hot slots here
    gword[GW_CODE] = 0;  // no giant-code refresh unless k_code_mode takes it below
    gword[GW_ABITS_PASS] = 0;  // no k_abits_pass since this refresh
    gword[GW_PURE_CNT] = 0;  // superstep 4's impure-unit list (k_units_pure)
    gword[GW_FILL] = 0;      // no fill-scatter form unless k_fill_decide takes it below ...
    gword[GW_FILL_TICKET] = 0;  // ... in its last block
    gword[GW_TRY] = n > 0 && 5 * (int64_t)(m >> 32) >= n ? 1 : 0;
  }
}

// Superstep 3's fill-scatter form (launch_refresh): the same pick on the NEW vector, ahead of
// the scatter, into words of its own -- gword[GW_G], gword[GW_TRY] and gword[GW_FILL] keep the old vector's
// values until k_al_scatter has run, whose fallback reads them (k_giant_pick follows it as in
// every refresh and finds the same G).  gword[GW_TRY3], the gate of the two counting kernels
// below: no rebuild is wanted (the rebuild would redo the refresh anyway) and, for the device
// decision (mode 1), superstep 2's refresh took the form (gword[GW_FILL] still set: no pick ran
// since) and the new G is worth trying; other graphs then pay three empty launches and no
// pass over the label vector.
__global__ __launch_bounds__(1024) void k_giant_pick3(const unsigned long long* __restrict__ counters, int64_t thr,
                                                      const int32_t* __restrict__ L, int64_t n_real,
                                                      int32_t* __restrict__ gword, int mode) {
  const int64_t n = n_real < kPickK ? n_real : kPickK;
  const u64 m = giant_pick_best(L, n, 0, 1);
  if (threadIdx.x == 0) {
    const bool try3 = n > 0 && 5 * (int64_t)(m >> 32) >= n;
    gword[GW_G3] = (int32_t)(~(u32)m);
    gword[GW_HOT3] = 0;
    gword[GW_FILL3] = 0;
    gword[GW_FILL3_TICKET] = 0;
    gword[GW_TRY3] = !rebuild_wanted(counters, thr) && (mode == 2 || (gword[GW_FILL] != 0 && try3)) ? 1 : 0;
  }
}

// (abits / nzero: the class-blocked rebuild that follows ORs the arc giant bits of its
// pieces into abits[0, nzero): zeroed here, one launch ahead)
// gword[GW_HOT_BITS] counts the set bits of the hot slots, slot i with (i & hmask) < hlim: the first
// kHotBits slots at P = 1 (hmask all ones), the first hlim slots of every slice of a
// rank-strided vector (hmask = slice - 1) -- the degree-ranked top set either way
// kStep3 (superstep 3's fill-scatter form, launch_refresh): the bitmap of the NEW vector into
// `bits` = gbits_next, relative to gword[GW_G3], its hot-bit count into gword[GW_HOT3]; gword's sparse / fill words
// and gbits stay as they are (k_al_scatter's fallback reads them) and nothing is zeroed
template <bool kIfWanted, bool kStep3 = false>
__global__ __launch_bounds__(256) void k_giant_bits(const unsigned long long* __restrict__ counters, int64_t thr,
                                                    const int32_t* __restrict__ L, int64_t n,
                                                    int32_t* __restrict__ gword,
                                                    unsigned long long* __restrict__ bits,
                                                    unsigned long long* __restrict__ abits, int64_t nzero,
                                                    uint64_t hmask, int64_t hlim) {
  if (kIfWanted && !rebuild_wanted(counters, thr)) return;
  if (kStep3 && gword[GW_TRY3] == 0) return;  // uniform (k_giant_pick3)
  // the hot-bit count: summed per block in LDS, one global atomic per block (a returning
  // atomic per wave on the one word serialised: ~2,500 of them, ~30 us at C3)
  __shared__ u32 bcnt;
  if (threadIdx.x == 0) bcnt = 0u;
  // a full rebuild follows (the LDS hot-set, small or code form): al[] is dense again unless
  // that rebuild takes the bits mode of one GPU and sets the word itself
  if (!kStep3 && blockIdx.x == 0 && threadIdx.x == 0) {
    gword[GW_AL_SPARSE] = 0;
    gword[GW_FILL] = 0;
  }
  __syncthreads();
  if (!kStep3)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nzero; i += (int64_t)gridDim.x * blockDim.x)
      abits[i] = 0ull;
  const int32_t G = gword[kStep3 ? GW_G3 : GW_G];
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t g0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 512; g0 < n; g0 += nw * 512) {
    int32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t i = g0 + k * 64 + lane;
      v[k] = i < n ? (int32_t)ld_stream(L + i) : ~G;
    }
    unsigned long long mine = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned long long m = __ballot(v[k] == G);
      if (lane == k) mine = m;
    }
    if (lane < 8 && g0 + lane * 64 < n) bits[(g0 >> 6) + lane] = mine;
    // the hot slots' set bits (the rebuild's bits-mode test without an LDS fill); a ranked
    // hlim and the slice are multiples of 64, so a bit word is hot or cold as a whole there;
    // kHotBits (P = 1) ends mid-word, and that word counts its hot half only -- the count is
    // then exactly the one k_al_rebuild_hot takes of its LDS words, so k_fill_decide, k_code_mode
    // and both rebuild kernels agree on the bits mode
    const int64_t wi = g0 + lane * 64;
    const int64_t hrem = hlim - (int64_t)((uint64_t)wi & hmask);
    const bool hot = lane < 8 && wi < n && hrem > 0;
    if (__ballot(hot)) {
      const u32 c = wave_sum_u32(hot ? (u32)__popcll(hrem >= 64 ? mine : mine & ((1ull << hrem) - 1ull)) : 0u);
      if (lane == 0 && c) atomicAdd(&bcnt, c);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && bcnt) atomicAdd(&gword[kStep3 ? GW_HOT3 : GW_HOT_BITS], (int32_t)bcnt);
}

// al[i] = lab(col[i]) over every arc by the calling grid (one wave per 512-arc batch,
// grid-stride); bits: also the arc giant bits (abits: bit i = al[i] == G, one ballot
// per 64 arcs), which the next superstep's full tally settles rows from (k_settle_*).
// sparse (one GPU, bits mode, lpa_graph::sparse_al): an arc whose label is G is carried by its
// bit alone and its al[] entry is not stored -- 98.5 % of the stores at C3 -- which every
// reader of al[] honours while gword[GW_AL_SPARSE] is set (lpa_device.h arc_label).
// -DLPA_SPARSE_POISON (a check build, never the default): those entries are stored after
// all, with a valid label other than G, so a reader that misses the bit changes a label.
__device__ __forceinline__ int32_t sparse_poison(int32_t G, int64_t nslots) {
  return (G ^ 1) < nslots ? (G ^ 1) : (G > 0 ? G - 1 : G);
}
// the sparse rebuild's bookkeeping (one thread): the flag, Gb and the refresh count
__device__ __forceinline__ void sparse_mark(int32_t* __restrict__ gword, bool sparse, int32_t G) {
  gword[GW_AL_SPARSE] = sparse ? 1 : 0;
  if (sparse) {
    gword[GW_AL_GB] = G;
    gword[GW_SPARSE_CNT] += 1;
  }
}
template <typename Lab>
__device__ __forceinline__ void rebuild_stream(Lab lab, int32_t G, bool bits, const int32_t* __restrict__ col,
                                               int64_t arcs, int32_t* __restrict__ al,
                                               unsigned long long* __restrict__ abits, bool sparse = false,
                                               int32_t poison = 0) {
  // lane-consecutive arcs: one gather instruction covers 64 consecutive arcs of
  // a row, whose sorted columns often share lines (hub rows) -> fewer L2 requests.
  // Full 512-arc batches are software-pipelined: the next batch's column loads are in
  // flight while this batch's labels are looked up and stored.
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t step = nw * 512;
  const int64_t nfull = arcs & ~(int64_t)511;  // arcs of the full batches
  int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 512;
  int32_t c[8];
  if (base < nfull) {
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = __builtin_nontemporal_load(col + base + k * 64 + lane);
  }
  for (; base < nfull; base += step) {
    int32_t cn[8], r[8];
    const int64_t nb = base + step;
    if (nb < nfull) {
#pragma unroll
      for (int k = 0; k < 8; ++k) cn[k] = __builtin_nontemporal_load(col + nb + k * 64 + lane);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = lab(c[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#ifdef LPA_SPARSE_POISON
      __builtin_nontemporal_store(sparse && r[k] == G ? poison : r[k], al + base + k * 64 + lane);
#else
      if (!(sparse && r[k] == G)) __builtin_nontemporal_store(r[k], al + base + k * 64 + lane);
#endif
    }
    if (bits) {
      unsigned long long mine = 0ull;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned long long m = __ballot(r[k] == G);
        if (lane == k) mine = m;
      }
      if (lane < 8) abits[(base >> 6) + lane] = mine;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = cn[k];
  }
  // the partial last batch (one wave)
  if (nfull < arcs && base == nfull) {
    for (int k = 0; k < 8; ++k) {
      const int64_t i = base + k * 64 + lane;
      const bool v = i < arcs;
      const int32_t x = v ? lab(col[i]) : 0;
#ifdef LPA_SPARSE_POISON
      if (v) al[i] = sparse && x == G ? poison : x;
#else
      if (v && !(sparse && x == G)) al[i] = x;
#endif
      const unsigned long long m = __ballot(v && x == G);
      if (bits && lane == 0 && base + k * 64 < arcs) abits[(base >> 6) + k] = m;
    }
  }
}

// The same stream in a three-stage software pipeline over 512-arc batches (P = 1 hot
// kernel): at step t the column loads of batch t + 3 are issued, batch t + 2's probe
// words fetched (p1: an LDS word, or an L2 word of gbits for a cold column), batch
// t + 1's labels resolved (p2: from the word, else a gather of L[c]) and batch t stored,
// so each wave keeps three batches' dependent loads in flight instead of one batch's
// chain (col -> bit word -> label).  Rings of 3 column sets and 2 word / label sets,
// six steps unrolled so no set is copied while its loads are in flight.
// The main loop is branch-free (every stage's batch exists, and p1 / p2 issue their
// loads unconditionally, at a clamped address where the value is not needed): the
// vector-memory counter is then tracked exactly, and waiting for batch t's labels does
// not wait for the loads of batches t + 1 .. t + 3 -- with a conditional load in the
// loop the compiler waited for every outstanding load (vmcnt(0)) at each step, which
// serialised the pipeline.  The last few batches run guarded.
//   fetch(t, c)  batch t's columns        probe(c, w)   p1 words
//   resolve(c, w, r)  p2 labels          store(t, r)    stores (+ arc giant bits)
template <typename Pre, typename F, typename Q, typename R, typename St>
__device__ __forceinline__ void pipe3(int64_t nb, Pre pre, F fetch, Q probe, R resolve, St store) {
  int32_t c0[8], c1[8], c2[8], r0[8], r1[8];
  u32 w0[8], w1[8];
  int64_t t = 0;
  if (nb <= 0) return;
  // pre(t, slot): batch t's descriptors (six slots, batch t in slot t mod 6), four
  // steps ahead of its fetch
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < nb) pre(k, k);
  fetch(0, c0, 0);
  if (nb > 1) fetch(1, c1, 1);
  if (nb > 2) fetch(2, c2, 2);
  probe(c0, w0);
  if (nb > 1) probe(c1, w1);
  resolve(c0, w0, r0);
#define LPA_PIPE_STEP(GUARD, I, CA, CB, CC, WA, WB, RA, RB) \
  if (!GUARD || t + 4 < nb) pre(t + 4, (I + 4) % 6);      \
  if (!GUARD || t + 3 < nb) fetch(t + 3, CA, (I + 3) % 6); \
  if (!GUARD || t + 2 < nb) probe(CC, WA);                 \
  if (!GUARD || t + 1 < nb) resolve(CB, WB, RB);           \
  store(t, RA, I);                                         \
  ++t;                                                     \
  if (GUARD && t >= nb) break;
#define LPA_PIPE_CYCLE(GUARD)                                 \
  LPA_PIPE_STEP(GUARD, 0, c0, c1, c2, w0, w1, r0, r1)        \
  LPA_PIPE_STEP(GUARD, 1, c1, c2, c0, w1, w0, r1, r0)        \
  LPA_PIPE_STEP(GUARD, 2, c2, c0, c1, w0, w1, r0, r1)        \
  LPA_PIPE_STEP(GUARD, 3, c0, c1, c2, w1, w0, r1, r0)        \
  LPA_PIPE_STEP(GUARD, 4, c1, c2, c0, w0, w1, r0, r1)        \
  LPA_PIPE_STEP(GUARD, 5, c2, c0, c1, w1, w0, r1, r0)
  // unguarded cycles: their last step (t + 5) issues pre(t + 9), so t + 9 < nb keeps
  // every descriptor read inside the list (a piece list has no padding past its end)
  while (t + 10 <= nb) {
    LPA_PIPE_CYCLE(false)
  }
  while (true) {
    LPA_PIPE_CYCLE(true)
  }
#undef LPA_PIPE_CYCLE
#undef LPA_PIPE_STEP
}

// arc giant bits of one 64-lane chunk at arc position st (len lanes live, lanes
// consecutive): one word, or two when st is not word-aligned (ORed: other chunks share
// the words; nzero-ed by k_giant_bits beforehand)
__device__ __forceinline__ void or_arc_bits(unsigned long long* __restrict__ abits, u32 st, unsigned long long m,
                                            int lane) {
  const u32 wd = st >> 6, off = st & 63u;
  if (m && lane == 0) atomicOr(&abits[wd], m << off);
  if (m && lane == 1 && off && (m >> (64u - off))) atomicOr(&abits[wd + 1], m >> (64u - off));
}

// the plain stream: this wave's whole 512-arc batches of [0, arcs), then the partial
// last batch (one wave)
// (kSparse: the bits mode of one GPU, whose stores may leave the G lanes out -- `sparse`;
// the other modes keep their unconditional stores)
template <bool kSparse = false, typename P1, typename P2>
__device__ __forceinline__ void rebuild_pipe(P1 p1, P2 p2, int32_t G, bool bits, const int32_t* __restrict__ col,
                                             int64_t arcs, int32_t* __restrict__ al,
                                             unsigned long long* __restrict__ abits, bool sparse = false,
                                             int32_t poison = 0) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nbatch = arcs >> 9;
  const int64_t nb = wv < nbatch ? (nbatch - wv + nw - 1) / nw : 0;
  auto base = [&](int64_t t) { return (wv + t * nw) * 512; };
  auto pre = [](int64_t, int) {};
  auto fetch = [&](int64_t t, int32_t (&c)[8], int) {
    const int64_t b = base(t);
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = __builtin_nontemporal_load(col + b + k * 64 + lane);
  };
  auto probe = [&](const int32_t (&c)[8], u32 (&w)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = p1(c[k]);
  };
  auto resolve = [&](const int32_t (&c)[8], const u32 (&w)[8], int32_t (&r)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = p2(c[k], w[k]);
  };
  auto store = [&](int64_t t, const int32_t (&r)[8], int) {
    const int64_t b = base(t);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#ifdef LPA_SPARSE_POISON
      __builtin_nontemporal_store(kSparse && sparse && r[k] == G ? poison : r[k], al + b + k * 64 + lane);
#else
      // (an exec-masked store: the sparse form leaves the G lanes out)
      if (!(kSparse && sparse && r[k] == G)) __builtin_nontemporal_store(r[k], al + b + k * 64 + lane);
#endif
    }
    if (bits) {
      unsigned long long mine = 0ull;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned long long m = __ballot(r[k] == G);
        if (lane == k) mine = m;
      }
      if (lane < 8) abits[(b >> 6) + lane] = mine;
    }
  };
  pipe3(nb, pre, fetch, probe, resolve, store);
  // the partial last batch (one wave)
  const int64_t nfull = nbatch << 9;
  if (nfull < arcs && wv == nbatch % nw) {
    for (int k = 0; k < 8; ++k) {
      const int64_t i = nfull + k * 64 + lane;
      const bool v = i < arcs;
      const int32_t c = v ? col[i] : 0;
      const int32_t x = p2(c, p1(c));
#ifdef LPA_SPARSE_POISON
      if (v) al[i] = sparse && x == G ? poison : x;
#else
      if (v && !(sparse && x == G)) al[i] = x;
#endif
      const unsigned long long m = __ballot(v && x == G);
      if (bits && lane == 0 && nfull + k * 64 < arcs) abits[(nfull >> 6) + k] = m;
    }
  }
}

// The class-blocked part of a labels-mode rebuild (P = 1).  A labels-mode rebuild is
// bound by its L2-missing gathers (C3 superstep 1: 3.6x the algorithmic bytes); a block
// group (blocks b = x mod 8, one XCD under the observed round-robin placement, speed
// only) streams the pieces of column class x -- the class segments of the rows of degree
// > block_deg, which keep their columns in (class, column) order -- so an XCD's gathers
// touch 1/8 of the label lines and its L2 holds far more of them (C3, simulated: 0.18
// -> 0.02 missing gathers per arc).  8 pieces (<= 64 arcs, lane-consecutive) per batch
// and wave, in pipe3's pipeline; a lane past its piece carries column 0 (a hot-set LDS
// read) and stores nothing; the descriptors ride a register ring four batches ahead
// (scalar loads in the stage that used them cost a round trip per step: the pieces
// phase ran at ~7 us per batch and wave).  bits: the arc giant bits, ORed.
#ifdef LPA_BLKTIME
// diagnostic build only (csrc/Makefile blktime): per block of the last blocked rebuild,
// the wall clock at its start, after its pieces and at its end
__device__ unsigned long long g_blk_time[3 * 512];
extern "C" int lpa_diag_blk_times(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_blk_time), sizeof(g_blk_time)) != hipSuccess) return -1;
  static unsigned long long zero[3 * 512];
  return hipMemcpyToSymbol(HIP_SYMBOL(g_blk_time), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
struct BlkInfo {
  int64_t off[kMaxBlkClasses + 1];  // class x: pieces [off[x], off[x + 1]), multiples of 8
  int64_t a0;                       // listed arcs [0, a0) (0: no blocked part)
  int phases;                       // classes / 8: group x streams x, x + 8, ...
};
template <typename P1, typename P2>
__device__ __forceinline__ void rebuild_pieces(P1 p1, P2 p2, int32_t G, bool bits, const u64* __restrict__ pieces,
                                               int64_t q0, int64_t q1, int64_t wi, int64_t nwv,
                                               const int32_t* __restrict__ col, int32_t* __restrict__ al,
                                               unsigned long long* __restrict__ abits) {
  const int lane = threadIdx.x & 63;
  auto uni = [](int64_t v) -> int64_t {
    return (int64_t)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)((u64)v >> 32)) << 32) |
                     (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v));
  };
  const int64_t step = uni(nwv * 8), first = uni(q0 + wi * 8), last = uni(q1);
  const int64_t nb = first < last ? (last - first + step - 1) / step : 0;
  // descriptor ring: lane k < 8 of slot j holds piece k of the batch in slot j, loaded
  // four steps ahead (a vector load, so waiting for it never waits on newer loads);
  // the stages read it with readlane
  u64 dr[6];
  auto pre = [&](int64_t t, int j) {
    const int64_t qq = first + t * step;
    dr[j] = lane < 8 ? pieces[qq + lane] : 0ull;
  };
  auto desc = [&](int j, int k) -> u64 {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(dr[j] >> 32), k) << 32) |
           (u64)(u32)__builtin_amdgcn_readlane((int)(u32)dr[j], k);
  };
  auto fetch = [&](int64_t, int32_t (&c)[8], int j) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const u64 d = desc(j, k);
      const bool live = lane < (int)(d >> 32);
      const int32_t x = __builtin_nontemporal_load(col + (u32)d + (live ? lane : 0));
      c[k] = live ? x : 0;
    }
  };
  // the probe word is read where it is used (an LDS read in the labels / hybrid modes
  // this path serves): no word ring, 16 VGPRs fewer
  auto probe = [&](const int32_t (&)[8], u32 (&)[8]) {};
  auto resolve = [&](const int32_t (&c)[8], const u32 (&)[8], int32_t (&r)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = p2(c[k], p1(c[k]));
  };
  auto store = [&](int64_t, const int32_t (&r)[8], int j) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const u64 d = desc(j, k);
      const int ln = (int)(d >> 32);
      if (lane < ln) __builtin_nontemporal_store(r[k], al + (u32)d + lane);
      if (bits) or_arc_bits(abits, (u32)d, __ballot(lane < ln && r[k] == G), lane);
    }
  };
  pipe3(nb, pre, fetch, probe, resolve, store);
}

// al[] rebuild with an LDS hot set (the slots of the highest-degree vertices: at P = 1
// the first slots, 30-40 % of all arc targets on R-MAT).  The rebuild is bound by the
// line traffic of its L2-missing 4-B gathers, and every gather served from LDS is one
// L2 request fewer.  One 1024-thread block per CU, 160 KB of LDS, in one of two modes
// that every block picks alike from the same data:
//   bits    (most hot slots carry the giant label G): LDS holds the giant-label bits of
//           the first 1.31 M slots, the other columns' bits come from gbits (L2); a
//           set bit is G, a clear one reads L[c].
//   labels  LDS holds the labels of the first 40,960 slots; the rest read L[c].
// kRanked (P > 1, power-of-two slices and rank count): the hottest vertices of rank
// r's slice are its first slots (degree rank k lives at slot (k mod P) S + k / P),
// so the global top set is the first H slots of every slice: slot c is hot iff
// (c mod S) < H, at LDS index (c / S) H + c mod S (H = 2^hot_lg labels or 2^hb_lg bits).
// kPieces (P = 1, a class-blocked handle: its labels-mode rebuild goes through the pieces):
// its own instantiation, so that the plain one's registers are allocated without the
// pieces' descriptor ring (one form for both spilled 16 VGPRs to scratch at the 128 of
// four waves per SIMD)
template <bool kIfWanted, bool kRanked, bool kPieces = false>
__global__ __launch_bounds__(1024) void k_al_rebuild_hot(const unsigned long long* __restrict__ counters,
                                                         int64_t thr, const int32_t* __restrict__ col,
                                                         int64_t arcs, const int32_t* __restrict__ Ln,
                                                         int32_t nhot, int32_t* __restrict__ al,
                                                         int slice_lg, int hot_lg, int hb_lg,
                                                         const uint32_t* __restrict__ gbits, int64_t nbits,
                                                         int32_t* __restrict__ gword,
                                                         unsigned long long* __restrict__ abits,
                                                         const u64* __restrict__ pieces, BlkInfo blk,
                                                         const int32_t* __restrict__ skip, int sparse_ok) {
  if (kIfWanted && !rebuild_wanted(counters, thr)) return;
  if (skip && *skip) return;  // the giant-code refresh replaces this rebuild (k_code_mode)
  if (!kRanked && gword[GW_FILL] != 0) return;  // ... or the fill-scatter form (k_fill_decide)
  __shared__ u32 hot[kHotLabelsSingle];
  u32* s_cnt = &hot[kHotLabelsSingle - 1];   // beyond the bit words; labels mode refills it
  // ---- the giant-label bits of the hot slots, and how many are set ----
  const int64_t nhb = kRanked ? ((int64_t)(nbits >> slice_lg) << hb_lg) : (nbits < kHotBits ? nbits : kHotBits);
  const int nhw = (int)((nhb + 31) >> 5);
  if (threadIdx.x == 0) *s_cnt = 0u;
  __syncthreads();
  int cnt = 0;
  for (int q = threadIdx.x; q < nhw; q += 1024) {
    int64_t gw = q;
    if constexpr (kRanked) gw = ((int64_t)(q >> (hb_lg - 5)) << (slice_lg - 5)) + (q & ((1 << (hb_lg - 5)) - 1));
    const u32 w = gbits[gw];
    hot[q] = w;
    cnt += __popc(w);
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(s_cnt, (u32)cnt);
  __syncthreads();
  const bool bits = 2 * (int64_t)*s_cnt >= nhb && nhb > 0;  // uniform: the same data in every block
  // hybrid (P = 1): G on >= 1/8 of the bit-range slots but not on half -- labels-mode
  // gathers that also write the arc giant bits (the next superstep's settle).  (Taking a
  // cold column's G from its gbits bit instead of its label measured slower: C5 186.7 ->
  // 176.4 GTEPS.)
  const bool hyb = !kRanked && !bits && 8 * (int64_t)*s_cnt >= nhb && nhb > 0;
  const int32_t G = gword[GW_G];
  // bits / hybrid modes also write the arc giant bits (abits: bit i = al[i] == G, one
  // ballot per 64 arcs), which the next superstep's full tally settles rows from
  // (k_settle_*)
  if (blockIdx.x == 0 && threadIdx.x == 0) gword[GW_ABITS_OK] = (bits || hyb) ? 1 : 0;
  // one GPU, bits mode: the G arcs go unstored (rebuild_stream's note); every other mode
  // leaves al[] dense (k_giant_bits cleared the word)
  const bool sparse = !kRanked && bits && sparse_ok != 0;
  if (!kRanked && blockIdx.x == 0 && threadIdx.x == 0) sparse_mark(gword, sparse, G);
  const int32_t poison = sparse_poison(G, nbits);
  if (!bits) {
    __syncthreads();
    for (int i = threadIdx.x; i < nhot; i += 1024)
      hot[i] = (u32)(kRanked ? Ln[((int64_t)(i >> hot_lg) << slice_lg) + (i & ((1 << hot_lg) - 1))] : Ln[i]);
    __syncthreads();
  }
  const u32 nh = (u32)nhot;
  const u32 smask = kRanked ? (1u << slice_lg) - 1u : 0u, hcap = 1u << hot_lg, bcap = 1u << hb_lg;
  auto lab = [&](int c) -> int32_t {
    if (bits) {
      u32 w;
      if constexpr (kRanked) {
        const u32 j = (u32)c & smask;
        w = j < bcap ? hot[((((u32)c >> slice_lg) << hb_lg) + j) >> 5] : gbits[(u32)c >> 5];
      } else {
        w = (u32)c < (u32)nhb ? hot[(u32)c >> 5] : gbits[(u32)c >> 5];
      }
      return ((w >> ((u32)c & 31u)) & 1u) ? G : Ln[c];
    }
    if constexpr (kRanked) {
      const u32 j = (u32)c & smask;
      return j < hcap ? (int32_t)hot[(((u32)c >> slice_lg) << hot_lg) + j] : Ln[c];
    } else {
      return (u32)c < nh ? (int32_t)hot[c] : Ln[c];
    }
  };
  if constexpr (kRanked) {
    rebuild_stream(lab, G, bits, col, arcs, al, abits);
  } else {
    // branch-free probes (pipe3): both sources are read -- the LDS word at a clamped
    // index, the gbits word / the label at a fixed address where it is not needed (the
    // wave's lanes then share one line)
    const u32 nhbu = (u32)nhb;
    // (the slots' labels through a buffer descriptor: launch_rebuild takes this kernel at
    // P = 1 only up to kHotMaxSlots = 2^29 slots, so every byte offset fits the voffset)
    const auto ln_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Ln, 0, (int)(nbits * 4), 0x00020000);
    constexpr int kPast = (int)0x80000000u;  // past every record count: no request
    auto run = [&](auto p1, auto p2, bool wbits, auto sp) {
      // (sp: the bits mode -- its stream may be sparse; it never takes the pieces)
      // uniform: labels / hybrid mode of a blocked handle (the bits mode through the
      // pieces measured slower, round 6: C5 superstep 3 13.4 -> 17.4 ms, C4 superstep 2
      // 8.9 -> 12.8 ms -- its lookups hit LDS / L2 anyway, the split arc ranges cost)
      if (kPieces && !bits) {
        const int grp = blockIdx.x & 7;
        const int64_t nwv = (int64_t)(gridDim.x >> 3) * (blockDim.x >> 6);
        const int64_t wi = (int64_t)(blockIdx.x >> 3) * (blockDim.x >> 6) + (threadIdx.x >> 6);
#ifdef LPA_BLKTIME
        if (threadIdx.x == 0 && blockIdx.x < 512) g_blk_time[3 * blockIdx.x] = wall_clock64();
#endif
        for (int ph = 0; ph < blk.phases; ++ph)
          rebuild_pieces(p1, p2, G, wbits, pieces, blk.off[grp + 8 * ph], blk.off[grp + 8 * ph + 1], wi, nwv,
                         col, al, abits);
#ifdef LPA_BLKTIME
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 512) atomicMax(&g_blk_time[3 * blockIdx.x + 1], wall_clock64());
#endif
        // then every block: the plain stream over the rows below block_deg
        rebuild_pipe(p1, p2, G, wbits, col + blk.a0, arcs - blk.a0, al + blk.a0, abits + blk.a0 / 64);
#ifdef LPA_BLKTIME
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 512) atomicMax(&g_blk_time[3 * blockIdx.x + 2], wall_clock64());
#endif
      } else {
        rebuild_pipe<decltype(sp)::value>(p1, p2, G, wbits, col, arcs, al, abits, sparse, poison);
      }
    };
    if (bits) {
      // the gbits words and the labels through buffer descriptors (base + 32-bit offset:
      // two VGPRs fewer per address under the 128 of four waves per SIMD, where the 64-bit
      // form spilled 14), and a lane that needs no word or label takes an offset past the
      // records: the range check drops its request instead of re-reading a fixed line
      const auto gb_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)gbits, 0, (int)(((nbits + 31) >> 5) * 4), 0x00020000);
      run(
          [&](int c) -> u32 {
            const bool h = (u32)c < nhbu;
            const u32 hw = hot[(h ? (u32)c : nhbu - 1u) >> 5];
            const u32 gw = __builtin_amdgcn_raw_buffer_load_b32(gb_rsrc, h ? kPast : (int)(((u32)c >> 5) << 2), 0, 0);
            return h ? hw : gw;
          },
          [&](int c, u32 w) -> int32_t {
            const bool g = (w >> ((u32)c & 31u)) & 1u;
            const int32_t x = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ln_rsrc, g ? kPast : (int)((u32)c << 2), 0, 0);
            return g ? G : x;
          },
          true, std::true_type{});
    } else {
      run([&](int c) -> u32 { return hot[(u32)c < nh ? (u32)c : nh - 1u]; },
          [&](int c, u32 w) -> int32_t {
            const bool h = (u32)c < nh;
            const int32_t x = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ln_rsrc, h ? kPast : (int)((u32)c << 2), 0, 0);
            return h ? (int32_t)w : x;
          },
          hyb, std::false_type{});
    }
  }
}

// al[] rebuild of a small label vector (P = 1, < kHotMinSlots slots: it stays in L2 /
// the Infinity Cache, so an LDS hot set saves no misses while every block's 160 KB fill
// costs as much as the arcs' stream at C2 scale): the same bits / labels modes, the
// bits-mode test from k_giant_bits' count of the hot slots' set bits (gword[GW_HOT_BITS]).
template <bool kIfWanted>
__global__ __launch_bounds__(256) void k_al_rebuild_small(const unsigned long long* __restrict__ counters,
                                                          int64_t thr, const int32_t* __restrict__ col, int64_t arcs,
                                                          const int32_t* __restrict__ Ln, int32_t* __restrict__ al,
                                                          const uint32_t* __restrict__ gbits, int64_t nbits,
                                                          int32_t* __restrict__ gword,
                                                          unsigned long long* __restrict__ abits, int sparse_ok) {
  if (kIfWanted && !rebuild_wanted(counters, thr)) return;
  if (gword[GW_FILL] != 0) return;  // the fill-scatter form replaces this rebuild (k_fill_decide)
  const int64_t nhb = nbits < kHotBits ? nbits : kHotBits;
  const bool bits = nhb > 0 && 2 * (int64_t)gword[GW_HOT_BITS] >= nhb;  // uniform
  const int32_t G = gword[GW_G];
  if (blockIdx.x == 0 && threadIdx.x == 0) gword[GW_ABITS_OK] = bits ? 1 : 0;
  const bool sparse = bits && sparse_ok != 0;  // the G arcs go unstored (rebuild_stream's note)
  if (blockIdx.x == 0 && threadIdx.x == 0) sparse_mark(gword, sparse, G);
  if (!bits) {  // labels mode: the plain 16 B/lane gather stream (C2: 0.21 -> ~0.17 ms)
    rebuild_all(col, arcs, Ln, al);
    return;
  }
  auto lab = [&](int c) -> int32_t {
    if ((gbits[(u32)c >> 5] >> ((u32)c & 31u)) & 1u) return G;
    return Ln[c];
  };
  rebuild_stream(lab, G, true, col, arcs, al, abits, sparse, sparse_poison(G, nbits));
}

// ---------------------------------------------------------------------------
// The fill-scatter form of the sparse bits-mode rebuild (one GPU; LPA_FILL_SCATTER).
// A sparse al[] needs, of a bits-mode rebuild, the arc giant bits and the al[] entries of
// the arcs whose column is off G -- at C3 after superstep 2, 1.5 % of the arcs, all in short
// columns of low-degree vertices -- while the stream form reads every arc's column and probes
// a giant bit for it.  This form sets every arc bit and then visits only the columns off G
// through the CSC position index: al[p] = L[u] and bit p cleared for each position p of such
// a column u.  The result is the stream form's, bit for bit in abits and entry for entry in
// al[] wherever a bit is clear.
//
// k_fill_decide (after k_giant_bits, whose gbits and hot-bit count it reads): returns at once
// unless the rebuild is wanted and in bits mode (the test of both rebuild kernels; the code
// refresh needs the opposite, k_code_mode).  Then it
//   - sets the arc bits [0, arcs) (the last word's tail stays clear, as the stream leaves
//     it) -- already here, before the decision: a bits-mode stream that runs after all
//     rewrites every word, and the scatter then needs no launch between it and the fill;
//   - sums the positions of the columns off G below the isolated slots, and their longest
//     (cptr read for those slots only; a lane per slot, all-G bit words skipped), one partial
//     per block in part[] (4,096 blocks adding into gword cost ~150 us of same-address atomics);
//   - in its last block (ticket) sums the partials and takes the form when those arcs are <= frac_arcs and no
//     column is longer than cap (mode 2, tests: always), with the sparse rebuild's
//     bookkeeping: gword[GW_FILL], sparse_mark, gword[GW_ABITS_OK], gword[GW_FILL_CNT].
// -DLPA_SPARSE_POISON: every al[] entry is poisoned first (the stream, if it runs after all,
// rewrites every entry in that build).
// Every arc bit of [0, arcs) set (the last word's tail stays clear, as the stream leaves it) by
// the calling grid, thread tid of nth.  -DLPA_SPARSE_POISON: every al[] entry poisoned too.
__device__ __forceinline__ void fill_arc_bits(unsigned long long* __restrict__ abits, int32_t* __restrict__ al,
                                              int64_t arcs, int32_t G, int64_t nslots, int64_t tid, int64_t nth) {
  const int64_t nfw = arcs >> 6;
  {  // 16-B streaming stores (device allocations are 256-B aligned), the odd word and the tail apart
    v4i* __restrict__ a4 = reinterpret_cast<v4i*>(abits);
    v4i ones;
    ones.x = ones.y = ones.z = ones.w = -1;
#ifdef LPA_FILL_PLAIN_STORES  // A/B variant build: ordinary stores
    for (int64_t i = tid; i < (nfw >> 1); i += nth) a4[i] = ones;
#else
    for (int64_t i = tid; i < (nfw >> 1); i += nth) __builtin_nontemporal_store(ones, a4 + i);
#endif
  }
  if (tid == 0 && (nfw & 1)) abits[nfw - 1] = ~0ull;
  if (tid == 0 && (arcs & 63)) abits[nfw] = (1ull << (arcs & 63)) - 1ull;
#ifdef LPA_SPARSE_POISON
  {
    const int32_t poison = sparse_poison(G, nslots);
    for (int64_t i = tid; i < arcs; i += nth) al[i] = poison;
  }
#else
  (void)al;
  (void)nslots;
#endif
}

// kStep3 (superstep 3's fill-scatter form, launch_refresh): the count and the decision alone,
// on gbits64 = gbits_next and gword[GW_HOT3], into gword[GW_FILL3] and nothing else.  THE FILL MAY NOT PRECEDE
// THIS DECISION there: after superstep 2 a refused form is followed by a stream rebuild that
// rewrites every word, but here it is followed by k_al_scatter, which relies on the kept bits --
// so k_al_scatter fills, once the form is taken, and does the form's bookkeeping.  Taken when
// the new vector is in bits mode and (mode 2: always) no column off G is longer than cap, more
// than fr_thr arcs are dirty (below that share superstep 4 would want the frontier marks the
// form does not write, and the fill no longer pays) and the arcs of the columns off G are at
// most kFill3Ratio of the dirty arcs.
template <bool kIfWanted, bool kStep3 = false>
__global__ __launch_bounds__(1024) void k_fill_decide(const unsigned long long* __restrict__ counters, int64_t thr,
                                                     const unsigned long long* __restrict__ gbits64, int64_t n_iso,
                                                     const int64_t* __restrict__ cptr, int64_t arcs, int64_t nhb,
                                                     int64_t nslots, int32_t* __restrict__ gword,
                                                     unsigned long long* __restrict__ abits,
                                                     int32_t* __restrict__ al, int mode, int64_t frac_arcs,
                                                     int64_t cap, unsigned long long* __restrict__ part,
                                                     int64_t fr_thr = 0) {
  if (kIfWanted && !rebuild_wanted(counters, thr)) return;
  if (kStep3 && gword[GW_TRY3] == 0) return;  // uniform (k_giant_pick3)
  if (!(nhb > 0 && 2 * (int64_t)gword[kStep3 ? GW_HOT3 : GW_HOT_BITS] >= nhb)) return;  // not the bits mode (uniform)
  const int32_t G = gword[kStep3 ? GW_G3 : GW_G];
  (void)G;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  if constexpr (!kStep3) fill_arc_bits(abits, al, arcs, G, nslots, tid, nth);
  // ---- the arcs of the columns off G: a wave takes kDecideWords bit words at a time (one
  // load), then four words' slots per round, their cptr loads in flight together ----
  constexpr int kDecideWords = 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nw = nth >> 6, ngrp = (n_iso + 63) >> 6;
  unsigned long long sum = 0ull;
  u32 mx = 0u;
#ifdef LPA_FILL_ONLY_TIMING  // variant build that times the fill alone: no
  if (false)                 // count, so the form is always taken
#endif
  for (int64_t g0 = (tid >> 6) * kDecideWords; g0 < ngrp; g0 += nw * kDecideWords) {
    const unsigned long long off = lane < kDecideWords && g0 + lane < ngrp ? ~gbits64[g0 + lane] : 0ull;
    if (__ballot(off != 0ull) == 0ull) continue;
    for (int j0 = 0; j0 < kDecideWords; j0 += 4) {
      unsigned long long w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = __shfl(off, j0 + j, 64);
      if ((w[0] | w[1] | w[2] | w[3]) == 0ull) continue;  // uniform
      int64_t a[4], e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t u = (g0 + j0 + j) * 64 + lane;
        const bool on = ((w[j] >> lane) & 1ull) && u < n_iso;
        a[j] = on ? cptr[u] : 0;
        e[j] = on ? cptr[u + 1] : 0;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sum += (unsigned long long)(e[j] - a[j]);
        mx = max(mx, (u32)min(e[j] - a[j], (int64_t)0x7FFFFFFF));
      }
    }
  }
  // ---- per block one partial (no same-address atomics beyond the ticket: ~12 ns each) ----
  __shared__ unsigned long long s_sum[16];
  __shared__ u32 s_max[16];
  __shared__ int s_last;
  auto reduce = [&]() {  // -> thread 0: the block's sum and max
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o, 64);
      mx = max(mx, (u32)__shfl_xor((int)mx, o, 64));
    }
    if (lane == 0) {
      s_sum[wv] = sum;
      s_max[wv] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = 1; k < (int)(blockDim.x >> 6); ++k) {
        sum += s_sum[k];
        mx = max(mx, s_max[k]);
      }
  };
  reduce();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = sum;
    part[2 * blockIdx.x + 1] = mx;
    __threadfence();
    s_last = atomicAdd(&gword[kStep3 ? GW_FILL3_TICKET : GW_FILL_TICKET], 1) == (int32_t)gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;  // uniform over the block
  __threadfence();
  sum = 0ull;
  mx = 0u;
  for (unsigned k = threadIdx.x; k < gridDim.x; k += blockDim.x) {
    sum += __hip_atomic_load(&part[2 * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mx = max(mx, (u32)__hip_atomic_load(&part[2 * k + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  __syncthreads();  // (s_sum / s_max reused)
  reduce();
  if (threadIdx.x != 0) return;
  if constexpr (kStep3) {
    const int64_t dirty = (int64_t)counters[1];
    if (mode == 2 || ((int64_t)mx <= cap && dirty > fr_thr && (double)sum <= kFill3Ratio * (double)dirty))
      gword[GW_FILL3] = 1;
    return;
  }
  if (mode == 2 || ((int64_t)sum <= frac_arcs && (int64_t)mx <= cap)) {
    gword[GW_FILL] = 1;
    sparse_mark(gword, true, G);
    gword[GW_ABITS_OK] = 1;
    gword[GW_FILL_CNT] += 1;
  }
}

// Clear the arc bits `m` of word `wd` for the wave's active lanes (act), one atomic per run of
// neighbouring lanes on the same word: the positions of consecutive slots ascend (the
// locality order of the build; columns ascend inside a row), so the lanes of one step mostly
// share a few words, and same-word atomics of one wave would otherwise queue at the word's
// channel.  A suffix OR over each run (a lane that matches a farther lane across another
// word only repeats a clear: harmless); the run's first lane issues the atomic.  Runs end at
// the 16-lane DPP rows: row shifts are VALU moves, while the wave-wide shuffles of a 64-lane
// merge went through the LDS pipe (18 ds_bpermute per step: the scatter was bound by them).
template <int kCtrl>
__device__ __forceinline__ u32 dpp_or_old(u32 old, u32 v) {  // a lane without a source keeps `old`
  return (u32)__builtin_amdgcn_update_dpp((int)old, (int)v, kCtrl, 0xF, 0xF, false);
}
__device__ __forceinline__ void clear_bits_merged(unsigned long long* __restrict__ abits, bool act, u32 wd,
                                                  unsigned long long m) {
  const u32 key = act ? wd : 0xFFFFFFFFu;  // (no word has this index: arcs < 2^32)
  u32 lo = act ? (u32)m : 0u, hi = act ? (u32)(m >> 32) : 0u;
#define LPA_MERGE_STEP(O)                                             \
  {                                                                   \
    const u32 ko = dpp_or_old<0x100 + O>(0xFFFFFFFEu, key); /* row_shl: lane + O */ \
    const u32 l2 = dpp_or_old<0x100 + O>(0u, lo), h2 = dpp_or_old<0x100 + O>(0u, hi); \
    if (ko == key) {                                                  \
      lo |= l2;                                                       \
      hi |= h2;                                                       \
    }                                                                 \
  }
  LPA_MERGE_STEP(1)
  LPA_MERGE_STEP(2)
  LPA_MERGE_STEP(4)
  LPA_MERGE_STEP(8)
#undef LPA_MERGE_STEP
  const u32 kp = dpp_or_old<0x111>(0xFFFFFFFEu, key);  // row_shr 1: lane - 1, a row's first lane none
  if (act && kp != key) atomicAnd(&abits[wd], ~(((unsigned long long)hi << 32) | lo));
}

// The scatter of the fill-scatter form: a wave takes 64 consecutive slots at a time (one gbits
// word; all-G words skipped), a lane per column off G for its cptr and label.  The columns'
// positions are cut into pieces of kFillPiece dealt over the lanes, so a round writes 64
// pieces whatever the columns' lengths (mean 2.4 at C3, a tail up to ~100: a lane per
// column left most lanes idle behind the longest) with kFillPiece position loads in flight
// per lane; most columns are one piece, so neighbouring lanes still hold the same step's
// positions of neighbouring columns, which are neighbours in al[] and abits.  A long column
// is many pieces of one wave (k_fill_decide refuses the form above its cap, lpa_internal.h).
// kMerge: clear_bits_merged, else one atomic per lane.
constexpr int kFillPiece = 4;
constexpr int kFillGroups = 4;
#ifdef LPA_FILL_PLAIN_ATOMICS  // A/B variant build: the per-lane atomics
constexpr bool kFillMerge = false;
#else
constexpr bool kFillMerge = true;
#endif
// kSlot: the gword word that says the form is taken (gword[GW_FILL3] in superstep 3's refresh)
template <bool kIfWanted, bool kMerge, int kSlot = GW_FILL>
__global__ __launch_bounds__(256) void k_fill_scatter(const unsigned long long* __restrict__ counters, int64_t thr,
                                                      const unsigned long long* __restrict__ gbits64, int64_t n_iso,
                                                      const int64_t* __restrict__ cptr,
                                                      const uint32_t* __restrict__ cpos,
                                                      const int32_t* __restrict__ L, int32_t* __restrict__ al,
                                                      unsigned long long* __restrict__ abits,
                                                      const int32_t* __restrict__ gword) {
  if (kIfWanted && !rebuild_wanted(counters, thr)) return;
  if (gword[kSlot] == 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6, ngrp = (n_iso + 63) >> 6;
  auto put = [&](bool act, u32 p, int32_t lab) {
    if (act) al[p] = lab;
    if (kMerge) clear_bits_merged(abits, act, p >> 6, 1ull << (p & 63u));
    else if (act) atomicAnd(&abits[p >> 6], ~(1ull << (p & 63u)));
  };
  // a wave takes kFillGroups bit words at a time (one load), then group after group
  for (int64_t g0 = (tid >> 6) * kFillGroups; g0 < ngrp; g0 += nw * kFillGroups) {
    const unsigned long long offs = lane < kFillGroups && g0 + lane < ngrp ? ~gbits64[g0 + lane] : 0ull;
    if (__ballot(offs != 0ull) == 0ull) continue;
    // every group's cptr and label loads first, in flight together
    int64_t bs[kFillGroups], es[kFillGroups];
    int32_t ls[kFillGroups];
#pragma unroll
    for (int gj = 0; gj < kFillGroups; ++gj) {
      const unsigned long long off = __shfl(offs, gj, 64);
      const int64_t u = (g0 + gj) * 64 + lane;
      const bool on = ((off >> lane) & 1ull) && u < n_iso;
      bs[gj] = on ? cptr[u] : 0;
      es[gj] = on ? cptr[u + 1] : 0;
      ls[gj] = on ? L[u] : 0;
    }
#pragma unroll
    for (int gj = 0; gj < kFillGroups; ++gj) {
      const int64_t b = bs[gj];
      const int n = (int)(es[gj] - b);
      const int32_t lab = ls[gj];
      if (__ballot(n != 0) == 0ull) continue;
      // pieces of kFillPiece positions, dealt over the lanes (scatter_runs' search)
      const int k = (n + kFillPiece - 1) / kFillPiece;
      int incl = k;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      const int S = __shfl(incl, 63, 64);
      for (int r0 = 0; r0 < S; r0 += 64) {
        const int t = r0 + lane;
        int o = 0;  // the owner: first lane whose inclusive piece count exceeds t
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) {
          const int ic = __shfl(incl, o + st - 1, 64);
          if (ic <= t) o += st;
        }
        o = o < 64 ? o : 63;
        const int excl = __shfl(incl, o, 64) - __shfl(k, o, 64);
        const int64_t bo = __shfl(b, o, 64);
        const int no = __shfl(n, o, 64);
        const int32_t lv = __shfl(lab, o, 64);
        const int p0 = (t - excl) * kFillPiece;
        const int cnt = t < S ? min(kFillPiece, no - p0) : 0;
        u32 p[kFillPiece];
#pragma unroll
        for (int j = 0; j < kFillPiece; ++j) p[j] = j < cnt ? cpos[bo + p0 + j] : 0u;
#pragma unroll
        for (int j = 0; j < kFillPiece; ++j) put(j < cnt, p[j], lv);
      }
    }
  }
}

// gword[GW_CODE] = take the giant-code refresh: a rebuild is wanted, G is worth trying, and the
// bits-mode rebuild (G on >= half the hot slots) does not apply; no arc giant bits then
__global__ void k_code_mode(const unsigned long long* __restrict__ counters, int64_t thr, int64_t nhb,
                            int32_t* __restrict__ gword) {
  if (threadIdx.x != 0) return;
  const bool on =
      rebuild_wanted(counters, thr) && gword[GW_TRY] != 0 && 2 * (int64_t)gword[GW_HOT_BITS] < nhb;
  gword[GW_CODE] = on ? 1 : 0;
  if (on) gword[GW_ABITS_OK] = 0;
}

// code2 for every slot: 16 labels (four int4 loads) -> one word (vpad is a multiple of 64)
__global__ __launch_bounds__(256) void k_code_build(const int4* __restrict__ L4, int64_t nw,
                                                   const int32_t* __restrict__ gword, uint32_t* __restrict__ code2) {
  if (gword[GW_CODE] == 0) return;
  const u32 G = (u32)gword[GW_G];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nw; q += (int64_t)gridDim.x * blockDim.x) {
    u32 w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int4 v = L4[4 * q + k];
      w |= (giant_code2((u32)v.x, G) | (giant_code2((u32)v.y, G) << 2) | (giant_code2((u32)v.z, G) << 4) |
            (giant_code2((u32)v.w, G) << 6))
           << (8 * k);
    }
    code2[q] = w;
  }
}

// pipe3 over this wave's whole 512-arc batches in [bat0, bat1) (grid-stride by waves)
template <typename P1, typename P2, typename St>
__device__ __forceinline__ void range_pipe(P1 p1, P2 p2, St st, const int32_t* __restrict__ col, int64_t bat0,
                                           int64_t bat1) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nb = bat0 + wv < bat1 ? (bat1 - bat0 - wv + nw - 1) / nw : 0;
  auto base = [&](int64_t t) { return (bat0 + wv + t * nw) * 512; };
  auto pre = [](int64_t, int) {};
  auto fetch = [&](int64_t t, int32_t (&c)[8], int) {
    const int64_t b = base(t);
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = __builtin_nontemporal_load(col + b + k * 64 + lane);
  };
  auto probe = [&](const int32_t (&c)[8], u32 (&w)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = p1(c[k]);
  };
  auto resolve = [&](const int32_t (&c)[8], const u32 (&w)[8], int32_t (&r)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = p2(c[k], w[k]);
  };
  auto store = [&](int64_t t, const int32_t (&r)[8], int) { st(base(t), r); };
  pipe3(nb, pre, fetch, probe, resolve, store);
}

// al for [pB, arcs) (pB = code_pcut rounded down to a 512-arc batch) and al2 for [0, pA)
// (pA = code_pcut rounded up, at most the full batches): the batch across code_pcut gets
// both; the partial last batch (one wave) writes whichever applies.  One 1024-thread
// block per CU, 160 KB of LDS: the labelled rows (code_lbin) first, with the 40,960
// hottest labels in LDS, then the codes, with the 655,360 hottest slots' codes in LDS --
// the gathers are bound by their lane count, not their bytes, so the LDS share is the
// lever -- and the others from the 2-bit code array (vpad / 4 bytes: L2-resident at C3).
// kRanked (a partitioned job's rank, round 6): the hot sets are the first 2^hot_lg labels
// and the first 2^hc_lg codes of EVERY slice (degree rank k lives at slot (k mod P) S +
// k / P, so these are the global top degree ranks), at LDS index (c / S) H + c mod S as in
// k_al_rebuild_hot's ranked form; at P = 1 they are the first slots.
template <bool kRanked>
__global__ __launch_bounds__(1024) void k_code_rebuild(const int32_t* __restrict__ gword,
                                                       const int32_t* __restrict__ col, int64_t arcs,
                                                       const int32_t* __restrict__ Ln, int64_t nslots,
                                                       const uint32_t* __restrict__ code2, int64_t p64,
                                                       uint32_t* __restrict__ al2, int32_t* __restrict__ al,
                                                       int slice_lg, int hot_lg, int hc_lg) {
  if (gword[GW_CODE] == 0) return;
  __shared__ u32 hot[kHotLabelsSingle];
  const u32 G = (u32)gword[GW_G];
  const int lane = threadIdx.x & 63;
  const int64_t nfull = arcs >> 9;
  const int64_t bA = min((p64 + 511) >> 9, nfull), bB = p64 >> 9;
  const u32 smask = kRanked ? (1u << slice_lg) - 1u : 0u;
  // slot c -> its hot-set index (h: whether it has one) for a set of 2^lg per slice
  auto hot_at = [&](int c, int lg, u32 nflat, bool& h) -> u32 {
    if constexpr (kRanked) {
      const u32 j = (u32)c & smask;
      h = j < (1u << lg);
      return (((u32)c >> slice_lg) << lg) + j;
    } else {
      h = (u32)c < nflat;
      return (u32)c;
    }
  };
  // ---- the labels of the rows below the cut ----
  const u32 nh = kRanked ? (u32)((nslots >> slice_lg) << hot_lg)
                         : (u32)(nslots < kHotLabelsSingle ? nslots : kHotLabelsSingle);
  for (u32 i = threadIdx.x; i < nh; i += 1024)
    hot[i] = (u32)Ln[kRanked ? ((int64_t)(i >> hot_lg) << slice_lg) + (i & ((1u << hot_lg) - 1u)) : (int64_t)i];
  __syncthreads();
  range_pipe([&](int c) -> u32 {
               bool h;
               const u32 k = hot_at(c, hot_lg, nh, h);
               return hot[h ? k : nh - 1u];
             },
             [&](int c, u32 w) -> int32_t {
               bool h;
               (void)hot_at(c, hot_lg, nh, h);
               const int32_t x = Ln[h ? 0 : c];
               return h ? (int32_t)w : x;
             },
             [&](int64_t b, const int32_t (&r)[8]) {
#pragma unroll
               for (int k = 0; k < 8; ++k) __builtin_nontemporal_store(r[k], al + b + k * 64 + lane);
             },
             col, bB, nfull);
  // ---- the codes of the rows above ----
  __syncthreads();
  // (a multiple of 16 either way: ranked, 2^hc_lg >= 16 codes per slice)
  const u32 nc = kRanked ? (u32)((nslots >> slice_lg) << hc_lg)
                         : (u32)(nslots < 16 * kHotLabelsSingle ? nslots : 16 * kHotLabelsSingle);
  for (u32 q = threadIdx.x; q < nc / 16; q += 1024)
    hot[q] = code2[kRanked ? ((int64_t)(q >> (hc_lg - 4)) << (slice_lg - 4)) + (q & ((1u << (hc_lg - 4)) - 1u))
                           : (int64_t)q];
  __syncthreads();
  auto cp1 = [&](int c) -> u32 {
    bool h;
    const u32 k = hot_at(c, hc_lg, nc, h);
    const u32 cc = h ? k : nc - 1u;
    return (hot[cc >> 4] >> (((u32)c & 15u) * 2u)) & 3u;   // (k = c mod 16 where hot)
  };
  auto cp2 = [&](int c, u32 w) -> int32_t {
    bool h;
    (void)hot_at(c, hc_lg, nc, h);
    const u32 x = code2[h ? 0u : ((u32)c >> 4)];
    return (int32_t)(h ? w : ((x >> (((u32)c & 15u) * 2u)) & 3u));
  };
  range_pipe(cp1, cp2, [&](int64_t b, const int32_t (&r)[8]) { store_code2(al2, b, r, lane); }, col, 0, bA);
  // the partial last batch
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t t0 = nfull << 9;
  if (t0 < arcs && wv == nfull % nw) {
    int32_t r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t i = t0 + k * 64 + lane;
      r[k] = 0;
      if (i < arcs) {
        const u32 x = (u32)Ln[col[i]];
        if (i < p64) r[k] = (int32_t)giant_code2(x, G);
        else al[i] = (int32_t)x;
      }
    }
    if (t0 < p64) store_code2(al2, t0, r, lane);   // uniform; al2 covers this batch then
  }
}

// al[] rebuild: the LDS hot-label kernel on a single-GPU handle (hub slots are
// [0, kHotLabels) there), the plain one otherwise
constexpr int64_t kHotMaxSlots = int64_t(1) << 29;  // k_al_rebuild_hot's 32-bit label offsets (P = 1)
int launch_rebuild(lpa_graph* g, bool if_wanted, int64_t thr, const int32_t* L,
                   const unsigned long long* ctr, bool allow_sparse = false) {
  hipStream_t s = g->stream;
  const bool code = if_wanted && code_refresh_now(g);
  // the giant label of the refreshed vector: the rebuild's bits below and the next
  // superstep's tallies (launch_tally's gsel) read it
  if (g->V > 0) {
    hipLaunchKernelGGL(k_giant_pick, dim3(1), dim3(kPickK), 0, s, L, g->V, g->slice, g->nranks, g->gword);
    LPA_HIP(hipGetLastError());
  }
  const bool ranked = rebuild_ranked(g);
  // one GPU outside gather mode: a bits-mode rebuild leaves al[] sparse (LPA_SPARSE_AL)
  // -- only in a superstep's own refresh (allow_sparse): the L0 rebuild, whose al[] superstep
  // 1's column runs read as it is, and the rebuild after a caller's put stay dense
  const int sparse_ok = (allow_sparse && g->sparse_al && g->nranks == 1 && !g->gather) ? 1 : 0;
  // hot slots of the bits-mode / code-mode test (k_giant_bits' count in gword[GW_HOT_BITS]): the
  // first kHotBits slots at P = 1, the first kHotBits / P (whole bit words) of every slice
  // of a rank-strided vector -- the same degree-ranked top set
  const uint64_t hmask = ranked ? (uint64_t)(g->slice - 1) : ~0ull;
  const int64_t hlim = ranked ? std::min<int64_t>(g->slice, kHotBits / g->nranks / 64 * 64) : kHotBits;
  const int64_t nhot_bits = ranked ? g->nranks * hlim : std::min<int64_t>(g->vpad, kHotBits);
  // the fill-scatter form of the sparse bits-mode rebuild (LPA_FILL_SCATTER; needs the CSC
  // position index): its decision and its scatter, launched between k_giant_bits and the
  // stream rebuild, which stands down when the form is taken
  auto launch_fill = [&]() -> int {
    if (!sparse_ok || g->fill_scatter == 0 || g->no_scatter || !g->cptr || !g->cpos || !g->fill_part)
      return LPA_OK;
    const int64_t n_iso = g->bin_begin[BIN_ISO];
    const unsigned long long* gb64 = (const unsigned long long*)g->gbits;
    const unsigned gd = cap_grid(std::max<int64_t>((n_iso + 1023) / 1024, (g->arcs / 64 + 8191) / 8192), kFillBlocks);
    const unsigned gs = cap_grid((n_iso + 64 * 4 * kFillGroups - 1) / (64 * 4 * kFillGroups), 8192);
    const int64_t frac_arcs = (int64_t)(kFillFrac * (double)g->arcs);
    const int64_t cap = std::max<int64_t>(kFillCap, g->arcs >> kFillCapShift);
    if (if_wanted) {
      hipLaunchKernelGGL(k_fill_decide<true>, dim3(gd), dim3(1024), 0, s, ctr, thr, gb64, n_iso, g->cptr, g->arcs,
                         nhot_bits, g->vpad, g->gword, g->abits, g->al, g->fill_scatter, frac_arcs,
                         cap, g->fill_part);
      hipLaunchKernelGGL((k_fill_scatter<true, kFillMerge>), dim3(gs), dim3(256), 0, s, ctr, thr, gb64, n_iso,
                         g->cptr, g->cpos, L, g->al, g->abits, g->gword);
    } else {
      hipLaunchKernelGGL(k_fill_decide<false>, dim3(gd), dim3(1024), 0, s, ctr, thr, gb64, n_iso, g->cptr, g->arcs,
                         nhot_bits, g->vpad, g->gword, g->abits, g->al, g->fill_scatter, frac_arcs,
                         cap, g->fill_part);
      hipLaunchKernelGGL((k_fill_scatter<false, kFillMerge>), dim3(gs), dim3(256), 0, s, ctr, thr, gb64, n_iso,
                         g->cptr, g->cpos, L, g->al, g->abits, g->gword);
    }
    LPA_HIP(hipGetLastError());
    return LPA_OK;
  };
  if (g->rebuild_hot && g->nranks == 1 && g->vpad < kHotMinSlots) {
    const int64_t ngrp = (g->vpad + 511) / 512;
    const unsigned gb = cap_grid((ngrp + 3) / 4, 4096), gr = cap_grid((g->arcs + 2047) / 2048, 8192);
    if (if_wanted)
      hipLaunchKernelGGL(k_giant_bits<true>, dim3(gb), dim3(256), 0, s, ctr, thr, L, g->vpad, g->gword,
                         (unsigned long long*)g->gbits, g->abits, (int64_t)0, hmask, hlim);
    else
      hipLaunchKernelGGL(k_giant_bits<false>, dim3(gb), dim3(256), 0, s, ctr, thr, L, g->vpad, g->gword,
                         (unsigned long long*)g->gbits, g->abits, (int64_t)0, hmask, hlim);
    LPA_HIP(hipGetLastError());
    LPA_TRY(launch_fill());
    if (if_wanted)
      hipLaunchKernelGGL(k_al_rebuild_small<true>, dim3(gr), dim3(256), 0, s, ctr, thr, g->col, g->arcs, L, g->al,
                         g->gbits, g->vpad, g->gword, g->abits, sparse_ok);
    else
      hipLaunchKernelGGL(k_al_rebuild_small<false>, dim3(gr), dim3(256), 0, s, ctr, thr, g->col, g->arcs, L, g->al,
                         g->gbits, g->vpad, g->gword, g->abits, sparse_ok);
  } else if (g->rebuild_hot && ((g->nranks == 1 && g->vpad <= kHotMaxSlots) || ranked)) {
    int dev_cus = 256;
    (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, g->device);
    int slice_lg = 0, hot_lg = 0, hb_lg = 0;
    int32_t nhot = (int32_t)(g->vpad < kHotLabelsSingle ? g->vpad : kHotLabelsSingle);
    if (ranked) {
      while ((int64_t(1) << slice_lg) < g->slice) ++slice_lg;
      while ((int64_t(1) << hot_lg) < kHotLabels / g->nranks) ++hot_lg;
      nhot = (int32_t)(g->nranks << hot_lg);
      // bits per slice: the largest power of two with P of them in the LDS bit budget,
      // at least one word and at most the slice
      while ((int64_t(2) << hb_lg) * g->nranks <= kHotBits && (int64_t(2) << hb_lg) <= g->slice) ++hb_lg;
      if (hb_lg < 5 || slice_lg < 5) hb_lg = 0;
    }
    // the giant-label bitmap of L first (same wanted-check: both return at once when
    // the scatter refreshes instead)
    const int64_t ngrp = (g->vpad + 511) / 512;
    // class-blocked labels-mode rebuild (P = 1): a grid of whole 8-block groups
    const bool blk = !ranked && g->blk_pieces && g->blk_a0 > 0 && dev_cus >= 8;
    if (blk) dev_cus &= ~7;
    const int64_t nzero = blk ? g->blk_a0 / 64 : 0;
    if (if_wanted)
      hipLaunchKernelGGL(k_giant_bits<true>, dim3(cap_grid((ngrp + 3) / 4, 4096)), dim3(256), 0, s, ctr, thr, L,
                         g->vpad, g->gword, (unsigned long long*)g->gbits, g->abits, nzero, hmask, hlim);
    else
      hipLaunchKernelGGL(k_giant_bits<false>, dim3(cap_grid((ngrp + 3) / 4, 4096)), dim3(256), 0, s, ctr, thr, L,
                         g->vpad, g->gword, (unsigned long long*)g->gbits, g->abits, nzero, hmask, hlim);
    LPA_HIP(hipGetLastError());
    LPA_TRY(launch_fill());
    // ranked without a usable bit share: nbits 0 keeps every block in labels mode
    const int64_t nbits = (ranked && hb_lg == 0) ? 0 : g->vpad;
    BlkInfo binfo;
    for (int x = 0; x <= kMaxBlkClasses; ++x) binfo.off[x] = g->blk_off[x];
    binfo.a0 = blk ? g->blk_a0 : 0;
    binfo.phases = g->blk_classes / 8;
#define LPA_HOT_LAUNCH(W, R, B)                                                                  \
  hipLaunchKernelGGL((k_al_rebuild_hot<W, R, B>), dim3(dev_cus), dim3(1024), 0, s, ctr, thr, g->col, \
                     g->arcs, L, nhot, g->al, slice_lg, hot_lg, hb_lg, g->gbits, nbits, g->gword, g->abits, \
                     blk ? g->blk_pieces : nullptr, binfo, code ? g->gword + GW_CODE : nullptr, sparse_ok)
    if (code) {
      hipLaunchKernelGGL(k_code_mode, dim3(1), dim3(64), 0, s, ctr, thr, nhot_bits, g->gword);
      LPA_HIP(hipGetLastError());
    }
    if (if_wanted) {
      if (ranked) LPA_HOT_LAUNCH(true, true, false);
      else if (blk) LPA_HOT_LAUNCH(true, false, true);
      else LPA_HOT_LAUNCH(true, false, false);
    } else {
      if (ranked) LPA_HOT_LAUNCH(false, true, false);
      else if (blk) LPA_HOT_LAUNCH(false, false, true);
      else LPA_HOT_LAUNCH(false, false, false);
    }
#undef LPA_HOT_LAUNCH
    if (code) {
      LPA_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_code_build, dim3(cap_grid((g->vpad / 16 + 255) / 256, 4096)), dim3(256), 0, s,
                         (const int4*)L, g->vpad / 16, g->gword, g->code2);
      LPA_HIP(hipGetLastError());
      // ranked: 2^hc_lg codes of every slice in LDS (P << hc_lg <= 16 kHotLabelsSingle)
      int hc_lg = 4;
      while (ranked && (int64_t(g->nranks) << (hc_lg + 1)) <= 16ll * kHotLabelsSingle &&
             (int64_t(1) << (hc_lg + 1)) <= g->slice)
        ++hc_lg;
      if (ranked)
        hipLaunchKernelGGL(k_code_rebuild<true>, dim3(dev_cus), dim3(1024), 0, s, g->gword, g->col, g->arcs, L,
                           g->vpad, g->code2, g->code_pcut, g->al2, g->al, slice_lg, hot_lg, hc_lg);
      else
        hipLaunchKernelGGL(k_code_rebuild<false>, dim3(dev_cus), dim3(1024), 0, s, g->gword, g->col, g->arcs, L,
                           g->vpad, g->code2, g->code_pcut, g->al2, g->al, 0, 0, 0);
    }
  } else {
    const unsigned grid = cap_grid((g->arcs / 4 + 511) / 512, 8192);
    if (if_wanted)
      hipLaunchKernelGGL(k_al_rebuild<true>, dim3(grid), dim3(256), 0, s, ctr, thr, g->col,
                         g->arcs, L, g->al, g->gword);
    else
      hipLaunchKernelGGL(k_al_rebuild<false>, dim3(grid), dim3(256), 0, s, ctr, thr, g->col,
                         g->arcs, L, g->al, g->gword);
  }
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

}  // namespace

// changed slots in [s0, s1) -> position chunks + dirty-arc count (counters of this
// superstep's parity)
int launch_diff(lpa_graph* g, hipStream_t st, const int32_t* Lc, const int32_t* Ln, int64_t s0,
                int64_t s1, bool sync, int par, int b0, int b1, int mode) {
  if (s1 <= s0) return LPA_OK;
  const int64_t nq = (s1 + 3) / 4 - s0 / 4;
  BinBounds bnd;
  for (int b = 0; b <= LPA_NBINS; ++b) bnd.b[b] = g->bin_begin[b];
  // bins [b0, b1) given: the frontier list mode is available (the concurrent tally
  // of this superstep; its lists are those of g->par)
  const bool lists = b1 > b0;
  hipLaunchKernelGGL(k_diff, dim3((unsigned)((nq + kDiffQuads - 1) / kDiffQuads)), dim3(256), 0, st,
                     (const int4*)Lc, (const int4*)Ln, sync ? const_cast<int32_t*>(Lc) : nullptr, s0, s1,
                     g->cptr, g->cch, g->chflag, g->chlist, g->counters + 4 * par, bnd, b0, b1,
                     lists ? g->flist : nullptr, g->fcnt + 16 * g->par, g->fr_all + g->par, mode);
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

// refresh al[] for L_next (after the exchange, so every rank sees all changes) of the
// superstep of parity `par`; diff_done: the tally schedule already ran the diff per
// stream (launch_tally) or the exchange listed the changes
// fold_rebuild: k_al_scatter does a wanted rebuild itself (captured converged
// supersteps: saves the rebuild launch, which is almost never wanted there)
int launch_refresh(lpa_graph* g, const int32_t* Lc, const int32_t* Ln, bool diff_done, int par,
                   hipEvent_t ev_scatter, bool fold_rebuild) {
  if (g->arcs == 0) return LPA_OK;
  hipStream_t s = g->stream;
  // this superstep's counters (zeroed by the previous k_al_scatter or at build)
  unsigned long long* ctr = g->counters + 4 * par;
  // one rank: its isolated slots (and the padding) never change; P > 1: the whole
  // replicated vector (other ranks' slots change through the exchange)
  const int64_t nd = !exchanges(g) ? g->bin_begin[BIN_ISO] : g->vpad;
  // diff_done means, at P = 1, that the tally's per-stream diffs ran (count-only ones in
  // a label-dense superstep); at P > 1, that the delta exchange queued every change
  // already (nothing left to count or diff)
  if (dense_refresh(g) && !(diff_done && exchanges(g))) {
    // counted changed slots (in the tally, or here) -> rebuild, or the full diff
    if (!diff_done) LPA_TRY(launch_diff(g, s, Lc, Ln, 0, nd, false, par, 0, 0, 1));
    hipLaunchKernelGGL(k_dense_decide, dim3(1), dim3(64), 0, s, ctr, nd, g->gword);
    LPA_HIP(hipGetLastError());
    LPA_TRY(launch_diff(g, s, Lc, Ln, 0, nd, true, par, 0, 0, 2));
  } else {
    if (!diff_done) LPA_TRY(launch_diff(g, s, Lc, Ln, 0, nd, true, par));
    // P > 1, superstep 2 after a giant-code refresh, its changes exchanged as a delta
    // (the change chunks are queued): the rows it settled from codes have no al[] entries,
    // so this refresh rebuilds whatever the change count (k_dense_decide's code clause)
    if (code_tally_now(g)) {
      hipLaunchKernelGGL(k_dense_decide, dim3(1), dim3(64), 0, s, ctr, INT64_MAX, g->gword);
      LPA_HIP(hipGetLastError());
    }
  }
  LPA_TRACE_POINT("diff");
  // (a handle without the CSC position index rebuilds every time: counters[1] >= 0 > -1)
  const int64_t thr = g->no_scatter ? -1 : (int64_t)(kRebuildFrac * (double)g->arcs);
  FrontierMarks fm;
  fm.crow = g->crow;
  fm.rp = g->rp;
  fm.uoff = g->hub_uoff;
  fm.n_hub = g->n_hub;
  fm.rdirty = g->rdirty[par ^ 1];
  fm.udirty = g->udirty[par ^ 1];
  if (code_tally3_now(g)) {
    // superstep 3 after a giant-code refresh: its settled rows' al[] entries were never
    // written, so this refresh rebuilds (k_dense_decide's code clause; n_slots: no count)
    hipLaunchKernelGGL(k_dense_decide, dim3(1), dim3(64), 0, s, ctr, INT64_MAX, g->gword);
    LPA_HIP(hipGetLastError());
  }
  // gather mode (lpa_build): no al[] to keep -- the scatter only marks the rows the next
  // superstep re-tallies (and syncs the changed labels into Lc), no rebuild
  const bool gnow = gather_now(g);
  // superstep 3's refresh keeps the arc giant bits of superstep 2's bits-mode rebuild
  // (k_al_scatter; superstep 4's row settle reads them)
  const bool keep_bits = keep_bits_now(g);
  if (g->al_pending && !gnow) {  // the column-run superstep after a lazy reset (al holds nothing)
    hipLaunchKernelGGL(k_al_fill_unless_rebuild, dim3(cap_grid((g->arcs / 4 + 255) / 256, 8192)), dim3(256), 0, s,
                       ctr, thr, (const v4i*)g->al0, (v4i*)g->al, g->arcs);
    LPA_HIP(hipGetLastError());
    g->al_pending = false;  // the rebuild below (or this fill + the scatter) makes al valid
  }
  // superstep 3 (fill_step3_now): the fill-scatter form in place of the scatter, decided on the
  // device -- the pick, the bitmap and the count of the NEW vector ahead of k_al_scatter, which
  // either scatters as ever or fills, and k_fill_scatter after it (k_al_scatter's note; the
  // wanted-rebuild launches below follow either way and return at once when the form ran).
  // Every other superstep and handle: none of these launches.
  const bool fill3 = fill_step3_now(g) && !fold_rebuild && !gnow && g->vpad <= kHotMaxSlots;
  const int64_t n_iso = g->bin_begin[BIN_ISO];
  const int64_t fr_thr = (int64_t)(kFrontierFrac * (double)g->arcs);
  if (fill3) {
    const int64_t ngrp = (g->vpad + 511) / 512;
    const unsigned gd = cap_grid(std::max<int64_t>((n_iso + 1023) / 1024, (g->arcs / 64 + 8191) / 8192), kFillBlocks);
    hipLaunchKernelGGL(k_giant_pick3, dim3(1), dim3(kPickK), 0, s, ctr, thr, Ln, g->V, g->gword, g->fill_step3);
    hipLaunchKernelGGL((k_giant_bits<false, true>), dim3(cap_grid((ngrp + 3) / 4, 4096)), dim3(256), 0, s, ctr, thr,
                       Ln, g->vpad, g->gword, (unsigned long long*)g->gbits_next, g->abits, (int64_t)0, ~0ull,
                       kHotBits);
    hipLaunchKernelGGL((k_fill_decide<false, true>), dim3(gd), dim3(1024), 0, s, ctr, thr,
                       (const unsigned long long*)g->gbits_next, n_iso, g->cptr, g->arcs,
                       std::min<int64_t>(g->vpad, kHotBits), g->vpad, g->gword, g->abits, g->al, g->fill_step3,
                       (int64_t)0, std::max<int64_t>(kFillCap, g->arcs >> kFillCapShift), g->fill_part, fr_thr);
    LPA_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_al_scatter, dim3(2048), dim3(256), 0, s, g->chlist, (const uint4*)g->chflag,
                     (g->n_chunk_scan + 15) / 16, g->cowner, g->cch, ctr,
                     g->counters + 4 * (par ^ 1), g->cptr,
                     g->cpos, Ln, gnow ? (int32_t*)nullptr : g->al, thr, fm, g->fr_all + (par ^ 1),
                     g->frontier, fr_thr, const_cast<int32_t*>(Lc),
                     (fold_rebuild && !gnow) ? g->col : (const int32_t*)nullptr, g->arcs, g->gword,
                     keep_bits ? 1 : 0, g->gbits, g->abits, fill3 ? 1 : 0, (const uint32_t*)g->gbits_next, g->vpad);
  LPA_HIP(hipGetLastError());
  if (fill3) {
    // (unchanged: it reads gbits, now the new vector's, as it does after superstep 2)
    hipLaunchKernelGGL((k_fill_scatter<false, kFillMerge, GW_FILL3>),
                       dim3(cap_grid((n_iso + 64 * 4 * kFillGroups - 1) / (64 * 4 * kFillGroups), 8192)), dim3(256), 0,
                       s, ctr, thr, (const unsigned long long*)g->gbits, n_iso, g->cptr, g->cpos, Ln, g->al, g->abits,
                       g->gword);
    LPA_HIP(hipGetLastError());
  }
  LPA_TRACE_POINT("scatter");
  if (ev_scatter) LPA_HIP(hipEventRecord(ev_scatter, s));  // profiling: scatter | rebuild
  if (gnow && gather_last_step(g)) {
    // the last gather-mode superstep: al[] for the supersteps after it, one plain rebuild
    const unsigned grid = cap_grid((g->arcs / 4 + 511) / 512, 8192);
    hipLaunchKernelGGL(k_al_rebuild<false>, dim3(grid), dim3(256), 0, s, ctr, thr, g->col, g->arcs, Ln, g->al,
                       g->gword);
    LPA_HIP(hipGetLastError());
  } else if (!fold_rebuild && !gnow) {
    LPA_TRY(launch_rebuild(g, true, thr, Ln, ctr, true));
  }
  LPA_HIP(hipGetLastError());
  return LPA_OK;
}

// (the caller-driven delta exchange, lpa_exchange_put_delta: the refresh of the superstep
// lpa_step just ran, which since_reset already counts -- it is seen as the in-library
// refresh of that superstep sees it: dense / code-settled supersteps, code refresh allowed)
int launch_refresh_ext(lpa_graph* g, const int32_t* Lc, const int32_t* Ln, bool diff_done, int par) {
  const bool back = g->since_reset > 0;
  if (back) --g->since_reset;
  const int rc = launch_refresh(g, Lc, Ln, diff_done, par);
  if (back) ++g->since_reset;
  return rc;
}

int rebuild_arc_labels(lpa_graph* g) {
  if (g->arcs == 0) return LPA_OK;
  return launch_rebuild(g, false, 0, g->lab[g->cur], g->counters);
}

int refresh_after_put(lpa_graph* g) {
  if (g->arcs == 0) return LPA_OK;
  if (at_l0(g)) return rebuild_arc_labels(g);   // no superstep ran since L0
  // the refresh of the superstep lpa_step just ran (since_reset counted it already): an
  // unconditional rebuild (thr = -1: every rebuild_wanted test passes), the giant codes
  // allowed after superstep 1 or 2 as in the in-library schedule
  --g->since_reset;
  const int rc = launch_rebuild(g, true, -1, g->lab[g->cur], g->counters + 4 * (g->par ^ 1));
  ++g->since_reset;
  return rc;
}

}  // namespace lpa
