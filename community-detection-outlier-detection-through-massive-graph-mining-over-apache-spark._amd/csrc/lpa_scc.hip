// Strongly connected components of the handle's directed input graph
// (GraphFrame.stronglyConnectedComponents, GraphX lib.StronglyConnectedComponents):
// comp[v] = the smallest dense id of v's SCC once the rounds have converged; stopped early
// by max_iter, a vertex whose SCC has not been written yet holds its own id, as in GraphX.
// Duplicates change nothing; an edge with an end outside [0, V) is no edge; a self-loop is a
// fact about its vertex (loop[v]: it is never trimmed).  Integers throughout.
//
// GraphX's rounds are Orzan's colouring algorithm, and so are these:
//   build    the E distinct non-loop arcs (lpa_adj.hip: arcs_count, arcs_lists): out-lists
//            oo / ocol, in-lists io / icol.  loop[v] = 1 by plain byte stores from the raw
//            edge list.  outc[v] / inc[v] = the list lengths: the live out- and in-counts
//   round    while a vertex is alive and rounds < max_iter: ++rounds, then
//   write    (from round 2 on) every marked v: comp[v] = colour[v], dead, appended to the
//            removal queue.  Round 1 instead: every v without a loop and with an empty
//            out- or in-list is dead and queued (the trim's first level)
//   trim     level by level over the removal queue: a queued u (written or trimmed) takes 1
//            from inc[w] of its alive successors and from outc[p] of its alive predecessors
//            (relaxed agent-scope atomics); the thread that takes a count to 0 claims the
//            vertex, unless it has a loop, by an atomic OR on the word of its state byte
//            (the old byte tells the one winner) and appends it to the queue.  Every vertex
//            enters the queue once in a call: it is one array with a head and a tail per row
//            form, V - sum(tails) is the number alive, and the tails' growth during the trim
//            is `trimmed`.  A level of at most scc_block vertices runs in ONE block, which
//            goes on level by level (the level's vertices in an LDS queue, __syncthreads
//            between levels) until the queue empties or a level outgrows the LDS queue; a
//            larger level is a launch per row form and one host read of the tails
//   colour   (only if rounds < max_iter) level 0: every alive v pulls the minimum of its own
//            id and its alive predecessors' ids over its in-list (colour[] = id is never
//            stored: no atomics); v joins the frontier if its colour dropped.  Level k: a
//            frontier u pushes colour[u] along its out-list with a relaxed agent-scope
//            atomicMin; a w whose colour dropped joins the next frontier (once: a flag byte
//            per level parity, claimed like the state byte, cleared by the level that
//            expands w).  Until a frontier is empty
//   mark     roots = alive v with colour[v] == v; a backward breadth-first search over the
//            in-lists, restricted to alive unmarked vertices of the frontier vertex's colour
//            (bit ST_MARK of the state byte, claimed by the same atomic OR)
//   finish   sizes and the summary from comp[], exact integers (lpa_adj.hip: comp_sizes)
//
// Row forms, by list length L (kSccShort / kSccWave; out + in for the trim, out for the
// colour push, in for the colour pull and the mark):
//   short   L <= kSccShort   8 lanes per listed row (the pull: every row in id order)
//   wave    L <= kSccWave    a wave per listed row
//   block   above            a block of 1024 per listed row (a hub of 10^5 arcs: 98 trips a lane)
// A vertex is put on the list of its form when it is appended; the pull's lists are static.
//
// Why the interleaving does not matter.  Trim: a count only falls, by exactly one per dead
// neighbour, so a vertex is claimed exactly when the peeling removes it, in whatever order;
// the fixpoint of peeling is unique.  Colour: every value ever stored in colour[v] is the id
// of an alive vertex with a path to v, and the stored value only falls (atomicMin is
// commutative, associative and idempotent); a vertex whose colour fell is expanded again, so
// at an empty frontier colour[w] <= colour[u] along every alive arc u -> w: the least
// fixpoint, the smallest alive ancestor, whatever the order of the atomics, of a list (its
// positions come from an atomic cursor) or of the levels.  A stale read of colour[u] pushes
// a larger value than the one that re-queues u.  Mark: the set reached by a search does not
// depend on its order.  So comp, rounds and every summary field are functions of
// (V, arc set, loop set, max_iter) alone; only the number of launches tells the schedule.
//
// Visibility.  Inside a kernel, state bytes and flags are read with plain loads and may be
// stale (another CU's L1 is never refreshed): a stale "alive" costs one needless atomic and a
// claim that fails, never a wrong one, since the atomic OR alone decides.  The counts and
// colour[] are only touched by agent-scope atomics where they are shared.  Lists written by
// one kernel are read by the next.
#include "lpa_device.h"
#include "lpa_algo.h"

namespace lpa {

namespace {

constexpr u32 ST_DEAD = 1, ST_MARK = 2;   // bits of a state byte (0: alive and unmarked)

// slots of the call's counters (u32): the removal queue's tails and, after an in-block trim,
// its heads, per row form; the frontier lists' lengths per level parity and row form
enum { Q_TAIL = 0, Q_HEAD = 3, F_CNT = 6, C_LEN = 12 };

struct Adj {   // the distinct non-loop arcs: out-lists and in-lists
  const int64_t* oo;
  const int32_t* ocol;
  const int64_t* io;
  const int32_t* icol;
};

__device__ __forceinline__ int form_of(int64_t L) { return L <= kSccShort ? 0 : L <= kSccWave ? 1 : 2; }
__device__ __forceinline__ int64_t out_len(const Adj& a, int64_t v) { return a.oo[v + 1] - a.oo[v]; }
__device__ __forceinline__ int64_t in_len(const Adj& a, int64_t v) { return a.io[v + 1] - a.io[v]; }

// bytes[v] |= bit by an atomic OR on the aligned word that holds the byte (the arrays are
// padded to whole words); true for the one caller that set it
__device__ __forceinline__ bool claim(uint8_t* bytes, int32_t v, u32 bit) {
  u32* w = reinterpret_cast<u32*>(bytes) + ((u32)v >> 2);
  const u32 m = bit << (8 * ((u32)v & 3u));
  return (__hip_atomic_fetch_or(w, m, LPA_RLX_AGENT) & m) == 0;
}

// v at the end of the list of form f (lists + f V, length cnt[f]); the address of each add
// is uniform over the lanes that take it
__device__ __forceinline__ void append(int32_t* __restrict__ lists, int64_t V, u32* __restrict__ cnt, int f,
                                       int32_t v) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (f == k) lists[(int64_t)k * V + atomicAdd(cnt + k, 1u)] = v;
}

// ---- listed rows, by form: op.begin(u) once per lane, then op.visit(ctx, j, w) for every
// entry w of u's list j (Op::kLists lists, op.list(j, off, col)) ----
template <class Op>
__device__ __forceinline__ void walk(const Op& op, int32_t u, int lane, int nlanes) {
  const auto ctx = op.begin(u);
#pragma unroll
  for (int j = 0; j < Op::kLists; ++j) {
    const int64_t* off;
    const int32_t* col;
    op.list(j, off, col);
    const int64_t b = off[u], L = off[u + 1] - b;
    for (int64_t i = lane; i < L; i += nlanes) op.visit(ctx, j, col[b + i]);
  }
}

template <class Op>
__global__ __launch_bounds__(256) void k_scc_rows_short(const int32_t* __restrict__ rows, int64_t nrows, Op op) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t k = (int64_t)blockIdx.x * kRows + threadIdx.x / G; k < nrows; k += (int64_t)gridDim.x * kRows)
    walk(op, rows[k], sub, G);
}

template <class Op>
__global__ __launch_bounds__(256) void k_scc_rows_wave(const int32_t* __restrict__ rows, int64_t nrows, Op op) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4)
    walk(op, rows[k], lane, 64);
}

template <class Op>
__global__ __launch_bounds__(kBlockThreads) void k_scc_rows_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                  Op op) {
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) walk(op, rows[k], threadIdx.x, kBlockThreads);
}

// ---- trim ----
struct TrimOp {
  static constexpr int kLists = 2;
  Adj a;
  int32_t* outc;
  int32_t* inc;
  const uint8_t* loop;
  uint8_t* st;
  int32_t* queue;
  int64_t V;
  u32* cnt;
  __device__ __forceinline__ int begin(int32_t) const { return 0; }
  __device__ __forceinline__ void list(int j, const int64_t*& off, const int32_t*& col) const {
    off = j == 0 ? a.oo : a.io;
    col = j == 0 ? a.ocol : a.icol;
  }
  __device__ __forceinline__ int form(int32_t v) const { return form_of(out_len(a, v) + in_len(a, v)); }
  // the dead u's neighbour w (j = 0: a successor, 1: a predecessor) loses an arc; true when
  // that emptied a count of w and this thread is the one that removes w
  __device__ __forceinline__ bool take(int j, int32_t w) const {
    if (st[w] & ST_DEAD) return false;
    if (__hip_atomic_fetch_add((j == 0 ? inc : outc) + w, -1, LPA_RLX_AGENT) != 1 || loop[w]) return false;
    return claim(st, w, ST_DEAD);
  }
  __device__ __forceinline__ void visit(int, int j, int32_t w) const {
    if (take(j, w)) append(queue, V, cnt + Q_TAIL, form(w), w);
  }
};

// the trim inside one block: the same walk, a removed vertex also goes to the next level's
// LDS queue (next[*nnext]; the count runs on when the queue is full)
struct BlockTrimOp {
  static constexpr int kLists = 2;
  TrimOp t;
  int32_t* next;
  u32* nnext;
  __device__ __forceinline__ int begin(int32_t) const { return 0; }
  __device__ __forceinline__ void list(int j, const int64_t*& off, const int32_t*& col) const { t.list(j, off, col); }
  __device__ __forceinline__ void visit(int, int j, int32_t w) const {
    if (!t.take(j, w)) return;
    append(t.queue, t.V, t.cnt + Q_TAIL, t.form(w), w);
    const u32 i = atomicAdd(nnext, 1u);
    if (i < (u32)kSccTrimCap) next[i] = w;
  }
};

// Round 1's start: the counts, comp[v] = v, and the trim's first level
__global__ __launch_bounds__(256) void k_scc_init(TrimOp op, int32_t* __restrict__ comp) {
  GRID_STRIDE(v, op.V) {
    const int64_t Lo = out_len(op.a, v), Li = in_len(op.a, v);
    op.outc[v] = (int32_t)Lo;
    op.inc[v] = (int32_t)Li;
    comp[v] = (int32_t)v;
    if (!op.loop[v] && (Lo == 0 || Li == 0)) {
      op.st[v] = (uint8_t)ST_DEAD;
      append(op.queue, op.V, op.cnt + Q_TAIL, form_of(Lo + Li), (int32_t)v);
    }
  }
}

// A later round's start: the marked vertices get their colour and leave
__global__ __launch_bounds__(256) void k_scc_write(TrimOp op, const int32_t* __restrict__ colour,
                                                   int32_t* __restrict__ comp) {
  GRID_STRIDE(v, op.V) {
    if (op.st[v] & ST_MARK) {
      comp[v] = colour[v];
      op.st[v] = (uint8_t)ST_DEAD;
      append(op.queue, op.V, op.cnt + Q_TAIL, op.form((int32_t)v), (int32_t)v);
    }
  }
}

// Levels of the trim in one block, from the queue's entries [h_f, tail_f) (at most
// kSccTrimCap in all, the caller's check).  A level's vertices sit in q[cur]; a short row is
// one thread's, a longer one is set aside and walked by the whole block.  Ends when a level
// removes nothing, or more than q[] holds: the heads it leaves (cnt[Q_HEAD + f]) tell the
// caller what is still to expand.
__global__ __launch_bounds__(kBlockThreads) void k_scc_trim_block(TrimOp op, u32 h0, u32 h1, u32 h2) {
  __shared__ int32_t q[2][kSccTrimCap];
  __shared__ int32_t big[kSccTrimCap];
  __shared__ u32 nq[2], nbig, hd[3];
  const int tid = threadIdx.x;
  {
    const u32 h[3] = {h0, h1, h2};
    u32 base = 0;
    for (int f = 0; f < 3; ++f) {
      const u32 t = __hip_atomic_load(op.cnt + Q_TAIL + f, LPA_RLX_AGENT);
      for (u32 i = h[f] + tid; i < t; i += kBlockThreads)
        if (base + (i - h[f]) < (u32)kSccTrimCap) q[0][base + (i - h[f])] = op.queue[(int64_t)f * op.V + i];
      base += t - h[f];
      if (tid == 0) hd[f] = t;
    }
    if (tid == 0) nq[0] = base < (u32)kSccTrimCap ? base : (u32)kSccTrimCap;
  }
  int cur = 0;
  while (true) {
    __syncthreads();   // q[cur], nq[cur] and hd are settled
    const u32 n = nq[cur];
    if (n == 0) break;
    if (tid == 0) {
      nq[cur ^ 1] = 0;
      nbig = 0;
    }
    __syncthreads();
    const BlockTrimOp bop{op, q[cur ^ 1], &nq[cur ^ 1]};
    for (u32 k = tid; k < n; k += kBlockThreads) {
      const int32_t u = q[cur][k];
      if (op.form(u) == 0) walk(bop, u, 0, 1);
      else big[atomicAdd(&nbig, 1u)] = u;
    }
    __syncthreads();
    const u32 nb = nbig;
    for (u32 k = 0; k < nb; ++k) walk(bop, big[k], tid, kBlockThreads);
    __syncthreads();   // every append of the level has returned
    if (nq[cur ^ 1] > (u32)kSccTrimCap) break;   // outgrown: hd stays at this level's start
    if (tid == 0)
      for (int f = 0; f < 3; ++f) hd[f] = __hip_atomic_load(op.cnt + Q_TAIL + f, LPA_RLX_AGENT);
    cur ^= 1;
  }
  if (tid == 0)
    for (int f = 0; f < 3; ++f) op.cnt[Q_HEAD + f] = hd[f];
}

// ---- colour ----
struct Colour0 {   // what level 0 needs besides the arcs
  const uint8_t* st;
  int32_t* colour;
  uint8_t* flag;     // level parity 0
  int32_t* lists;    // the frontier lists of parity 0
  int64_t V;
  u32* cnt;          // their lengths
};

// v's colour after level 0; v joins the frontier if it dropped and v has somewhere to push it
__device__ __forceinline__ void colour0_store(const Colour0& c, const Adj& a, int32_t v, int32_t col) {
  c.colour[v] = col;
  if (col < v) {
    const int64_t Lo = out_len(a, v);
    if (Lo > 0) {
      c.flag[v] = 1;
      append(c.lists, c.V, c.cnt, form_of(Lo), v);
    }
  }
}

__device__ __forceinline__ int32_t colour0_scan(const Colour0& c, const Adj& a, int64_t b, int64_t L, int lane,
                                                int nlanes, int32_t col) {
  for (int64_t i = lane; i < L; i += nlanes) {
    const int32_t p = a.icol[b + i];
    if (c.st[p] == 0) col = p < col ? p : col;
  }
  return col;
}

// every row in id order, kShortLanes lanes each; a longer row is not this form's
__global__ __launch_bounds__(256) void k_scc_pull_short(Adj a, Colour0 c) {
  constexpr int G = kShortLanes, kRows = 256 / G;
  const int sub = threadIdx.x & (G - 1);
  for (int64_t base = (int64_t)blockIdx.x * kRows; base < c.V; base += (int64_t)gridDim.x * kRows) {
    const int64_t v = base + threadIdx.x / G;
    bool mine = false;
    int32_t col = 0x7FFFFFFF;
    if (v < c.V && c.st[v] == 0) {
      const int64_t b = a.io[v], L = a.io[v + 1] - b;
      mine = L <= kSccShort;
      if (mine) col = colour0_scan(c, a, b, L, sub, G, (int32_t)v);
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      const int32_t o = __shfl_xor(col, off, 64);
      col = o < col ? o : col;
    }
    if (mine && sub == 0) colour0_store(c, a, (int32_t)v, col);
  }
}

__global__ __launch_bounds__(256) void k_scc_pull_wave(const int32_t* __restrict__ rows, int64_t nrows, Adj a,
                                                       Colour0 c) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < nrows; k += (int64_t)gridDim.x * 4) {
    const int32_t v = rows[k];
    if (c.st[v] != 0) continue;
    const int64_t b = a.io[v];
    int32_t col = colour0_scan(c, a, b, a.io[v + 1] - b, lane, 64, v);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int32_t o = __shfl_xor(col, off, 64);
      col = o < col ? o : col;
    }
    if (lane == 0) colour0_store(c, a, v, col);
  }
}

// a block per listed row (k and st[v] are the same in every thread: barriers inside)
__global__ __launch_bounds__(kBlockThreads) void k_scc_pull_block(const int32_t* __restrict__ rows, int64_t nrows,
                                                                  Adj a, Colour0 c) {
  constexpr int kWaves = kBlockThreads / 64;
  __shared__ int32_t ws[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t k = blockIdx.x; k < nrows; k += gridDim.x) {
    const int32_t v = rows[k];
    if (c.st[v] != 0) continue;
    const int64_t b = a.io[v];
    int32_t col = colour0_scan(c, a, b, a.io[v + 1] - b, threadIdx.x, kBlockThreads, v);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int32_t o = __shfl_xor(col, off, 64);
      col = o < col ? o : col;
    }
    if (lane == 0) ws[wave] = col;
    __syncthreads();
    if (threadIdx.x == 0) {
      int32_t t = ws[0];
      for (int i = 1; i < kWaves; ++i) t = ws[i] < t ? ws[i] : t;
      colour0_store(c, a, v, t);
    }
    __syncthreads();   // before the next row rewrites ws
  }
}

// level k >= 1: a frontier row pushes its colour along its out-list
struct PushOp {
  static constexpr int kLists = 1;
  Adj a;
  const uint8_t* st;
  int32_t* colour;
  uint8_t* flag_cur;    // this level's parity: cleared for the rows expanded
  uint8_t* flag_next;   // the other parity: claimed for the rows whose colour dropped
  int32_t* next;        // the next frontier's lists
  int64_t V;
  u32* cnt;             // their lengths
  __device__ __forceinline__ int32_t begin(int32_t u) const {
    flag_cur[u] = 0;
    return __hip_atomic_load(colour + u, LPA_RLX_AGENT);
  }
  __device__ __forceinline__ void list(int, const int64_t*& off, const int32_t*& col) const {
    off = a.oo;
    col = a.ocol;
  }
  __device__ __forceinline__ void visit(int32_t c, int, int32_t w) const {
    if (st[w] != 0) return;
    if (__hip_atomic_fetch_min(colour + w, c, LPA_RLX_AGENT) <= c) return;
    const int64_t Lo = out_len(a, w);
    if (Lo > 0 && claim(flag_next, w, 1u)) append(next, V, cnt, form_of(Lo), w);
  }
};

// ---- mark ----
__global__ __launch_bounds__(256) void k_scc_roots(Adj a, uint8_t* __restrict__ st,
                                                   const int32_t* __restrict__ colour, int64_t V,
                                                   int32_t* __restrict__ lists, u32* __restrict__ cnt) {
  GRID_STRIDE(v, V) {
    if (st[v] == 0 && colour[v] == (int32_t)v) {
      st[v] = (uint8_t)ST_MARK;
      const int64_t Li = in_len(a, v);
      if (Li > 0) append(lists, V, cnt, form_of(Li), (int32_t)v);
    }
  }
}

struct MarkOp {
  static constexpr int kLists = 1;
  Adj a;
  uint8_t* st;
  const int32_t* colour;
  int32_t* next;
  int64_t V;
  u32* cnt;
  __device__ __forceinline__ int32_t begin(int32_t u) const { return colour[u]; }
  __device__ __forceinline__ void list(int, const int64_t*& off, const int32_t*& col) const {
    off = a.io;
    col = a.icol;
  }
  __device__ __forceinline__ void visit(int32_t c, int, int32_t p) const {
    if (st[p] != 0 || colour[p] != c || !claim(st, p, ST_MARK)) return;
    const int64_t Li = in_len(a, p);
    if (Li > 0) append(next, V, cnt, form_of(Li), p);
  }
};

// the listed rows [head[f], head[f] + n[f]) of every form f
template <class Op>
void launch_rows(const Op& op, const int32_t* lists, int64_t V, const u32* head, const u32* n, hipStream_t s) {
  if (n[0])
    hipLaunchKernelGGL(k_scc_rows_short<Op>, dim3(grid_rows(n[0], 256 / kShortLanes, 65536)), dim3(256), 0, s,
                       lists + head[0], (int64_t)n[0], op);
  if (n[1])
    hipLaunchKernelGGL(k_scc_rows_wave<Op>, dim3(grid_rows(n[1], 4, 16384)), dim3(256), 0, s, lists + V + head[1],
                       (int64_t)n[1], op);
  if (n[2])
    hipLaunchKernelGGL(k_scc_rows_block<Op>, dim3(grid_rows(n[2], 1, 4096)), dim3(kBlockThreads), 0, s,
                       lists + 2 * V + head[2], (int64_t)n[2], op);
}

}  // namespace

// Reads V, m, e_src / e_dst, the stream and scc_block of the handle, nothing of the LPA
// state; every array is a stream-ordered temporary.
int strongly_connected_components(lpa_graph* g, int32_t max_iter, int32_t* comp_out, int32_t out_is_device,
                                  int64_t* size_out, lpa_scc_summary* summary) {
  hipStream_t s = g->stream;
  const int64_t V = g->V;
  if (summary) *summary = lpa_scc_summary{0, 0, 0, -1, 0, 0, 0};
  if (V == 0) return LPA_OK;
  Tmp tmp(s);
  // ---- build ----
  uint8_t* loop = nullptr;
  LPA_TRY(tmp.get(&loop, V));
  LPA_HIP(hipMemsetAsync(loop, 0, (size_t)V, s));
  ArcLists arcs;
  LPA_TRY(arcs_count(g, tmp, loop, &arcs));
  LPA_TRY(arcs_lists(g, tmp, &arcs));
  const Adj adj{arcs.oo, arcs.ocol, arcs.io, arcs.icol};
  // the pull's static lists, by in-list length
  int32_t* plists = nullptr;
  u32 hp[2] = {0, 0};   // the pull's wave rows and block rows (read after the first read_counts below)
  LPA_TRY(form_lists(tmp, arcs.io, V, kSccShort, kSccWave, &plists, hp));
  // ---- state ----
  const int64_t vbytes = (V + 3) & ~(int64_t)3;   // byte arrays claimed through their words
  int32_t *outc = nullptr, *inc = nullptr, *colour = nullptr, *queue = nullptr, *flists = nullptr, *comp = comp_out;
  uint8_t *st = nullptr, *fl = nullptr;
  u32* cnt = nullptr;
  LPA_TRY(tmp.get(&outc, V));
  LPA_TRY(tmp.get(&inc, V));
  LPA_TRY(tmp.get(&colour, V));
  LPA_TRY(tmp.get(&queue, 3 * V));
  LPA_TRY(tmp.get(&flists, 6 * V));   // the frontier's lists, per level parity and form
  LPA_TRY(tmp.get(&st, vbytes));
  LPA_TRY(tmp.get(&fl, 2 * vbytes));  // the colour frontier's flags, per level parity
  LPA_TRY(tmp.get(&cnt, C_LEN));
  if (!out_is_device) LPA_TRY(tmp.get(&comp, V));
  u32* pinned = nullptr;
  LPA_TRY(tmp.pin(&pinned, C_LEN));
  LPA_HIP(hipMemsetAsync(st, 0, (size_t)vbytes, s));
  LPA_HIP(hipMemsetAsync(fl, 0, (size_t)(2 * vbytes), s));
  LPA_HIP(hipMemsetAsync(cnt, 0, sizeof(u32) * C_LEN, s));
  const volatile u32* hc = pinned;
  const auto read_counts = [&]() -> int {
    LPA_HIP(hipMemcpyAsync(pinned, cnt, sizeof(u32) * C_LEN, hipMemcpyDeviceToHost, s));
    LPA_HIP(hipStreamSynchronize(s));
    return LPA_OK;
  };
  const TrimOp top{adj, outc, inc, loop, st, queue, V, cnt};
  const int64_t in_block = g->scc_block < kSccTrimCap ? g->scc_block : kSccTrimCap;
  const unsigned g_short = grid_rows(V, 256 / kShortLanes, 65536);
  u32 head[3] = {0, 0, 0}, tail[3] = {0, 0, 0};
  int64_t rounds = 0, trimmed = 0, removed = 0;
  while (removed < V && rounds < (int64_t)max_iter) {
    ++rounds;
    // ---- write (round 1: the counts and the trim's first level) ----
    if (rounds == 1) hipLaunchKernelGGL(k_scc_init, dim3(grid_for(V)), dim3(256), 0, s, top, comp);
    else hipLaunchKernelGGL(k_scc_write, dim3(grid_for(V)), dim3(256), 0, s, top, colour, comp);
    LPA_HIP(hipGetLastError());
    LPA_TRY(read_counts());
    for (int f = 0; f < 3; ++f) tail[f] = hc[Q_TAIL + f];
    const int64_t written = rounds == 1 ? 0 : (int64_t)tail[0] + tail[1] + tail[2] - removed;
    // ---- trim to the fixpoint ----
    while (true) {
      const u32 n[3] = {tail[0] - head[0], tail[1] - head[1], tail[2] - head[2]};
      const int64_t pending = (int64_t)n[0] + n[1] + n[2];
      if (pending == 0) break;
      if (pending <= in_block) {
        hipLaunchKernelGGL(k_scc_trim_block, dim3(1), dim3(kBlockThreads), 0, s, top, head[0], head[1], head[2]);
        LPA_HIP(hipGetLastError());
        LPA_TRY(read_counts());
        for (int f = 0; f < 3; ++f) head[f] = hc[Q_HEAD + f];
      } else {
        launch_rows(top, queue, V, head, n, s);
        LPA_HIP(hipGetLastError());
        LPA_TRY(read_counts());
        for (int f = 0; f < 3; ++f) head[f] = tail[f];
      }
      for (int f = 0; f < 3; ++f) tail[f] = hc[Q_TAIL + f];
    }
    const int64_t gone = (int64_t)tail[0] + tail[1] + tail[2];
    trimmed += gone - removed - written;
    removed = gone;
    if (removed == V || rounds == (int64_t)max_iter) break;
    // ---- colour ----
    LPA_HIP(hipMemsetAsync(cnt + F_CNT, 0, sizeof(u32) * 6, s));
    const Colour0 c0{st, colour, fl, flists, V, cnt + F_CNT};
    hipLaunchKernelGGL(k_scc_pull_short, dim3(g_short), dim3(256), 0, s, adj, c0);
    if (hp[0])
      hipLaunchKernelGGL(k_scc_pull_wave, dim3(grid_rows(hp[0], 4, 16384)), dim3(256), 0, s, plists, (int64_t)hp[0],
                         adj, c0);
    if (hp[1])
      hipLaunchKernelGGL(k_scc_pull_block, dim3(grid_rows(hp[1], 1, 4096)), dim3(kBlockThreads), 0, s, plists + V,
                         (int64_t)hp[1], adj, c0);
    LPA_HIP(hipGetLastError());
    const u32 zero[3] = {0, 0, 0};
    for (int cur = 0;; cur ^= 1) {
      LPA_TRY(read_counts());
      const u32 n[3] = {hc[F_CNT + 3 * cur], hc[F_CNT + 3 * cur + 1], hc[F_CNT + 3 * cur + 2]};
      if (n[0] + n[1] + n[2] == 0) break;   // each at most V
      const int nxt = cur ^ 1;
      LPA_HIP(hipMemsetAsync(cnt + F_CNT + 3 * nxt, 0, sizeof(u32) * 3, s));
      const PushOp pop{adj, st, colour, fl + cur * vbytes, fl + nxt * vbytes, flists + 3 * V * nxt, V,
                       cnt + F_CNT + 3 * nxt};
      launch_rows(pop, flists + 3 * V * cur, V, zero, n, s);
      LPA_HIP(hipGetLastError());
    }
    // ---- mark ----
    LPA_HIP(hipMemsetAsync(cnt + F_CNT, 0, sizeof(u32) * 6, s));
    hipLaunchKernelGGL(k_scc_roots, dim3(grid_for(V)), dim3(256), 0, s, adj, st, colour, V, flists, cnt + F_CNT);
    LPA_HIP(hipGetLastError());
    for (int cur = 0;; cur ^= 1) {
      LPA_TRY(read_counts());
      const u32 n[3] = {hc[F_CNT + 3 * cur], hc[F_CNT + 3 * cur + 1], hc[F_CNT + 3 * cur + 2]};
      if (n[0] + n[1] + n[2] == 0) break;
      const int nxt = cur ^ 1;
      LPA_HIP(hipMemsetAsync(cnt + F_CNT + 3 * nxt, 0, sizeof(u32) * 3, s));
      const MarkOp mop{adj, st, colour, flists + 3 * V * nxt, V, cnt + F_CNT + 3 * nxt};
      launch_rows(mop, flists + 3 * V * cur, V, zero, n, s);
      LPA_HIP(hipGetLastError());
    }
  }
  // ---- sizes and the summary ----
  ull h[3] = {0, 0, 0};
  ull* size = nullptr;
  if (size_out || summary) LPA_TRY(comp_sizes(tmp, comp, V, size_out, out_is_device, summary != nullptr, &size, h));
  if (!out_is_device) {
    LPA_HIP(hipMemcpyAsync(comp_out, comp, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, s));
    if (size_out) LPA_HIP(hipMemcpyAsync(size_out, size, sizeof(int64_t) * (size_t)V, hipMemcpyDeviceToHost, s));
  }
  LPA_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->n_components = (int64_t)h[0];
    summary->n_singletons = (int64_t)h[1];
    summary->largest_size = (int64_t)(h[2] >> 32);
    summary->largest_id = (int64_t)(0xFFFFFFFFu - (u32)h[2]);
    summary->rounds = rounds;
    summary->trimmed = trimmed;
    summary->unresolved = V - removed;
  }
  return LPA_OK;
}

}  // namespace lpa
