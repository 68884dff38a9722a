/*
 * lpa.h -- C ABI of the MI355X-native label-propagation + outlier library
 * (liblpa_hip.so, hand-written HIP for gfx950, RCCL for the multi-GPU label
 * exchange).  Plain pointers and sizes only; no torch types.
 *
 * Each entry point replaces one piece of the reference's hot path, which is
 * the JVM call chain behind
 *     /root/reference/CommunityDetection/Graphframes.py:78   GraphFrame(v, e)
 *     /root/reference/CommunityDetection/Graphframes.py:81   .labelPropagation(maxIter=5)
 *     /root/reference/CommunityDetection/Graphframes.py:92-137 outlier stage
 * (GraphFrames 0.6.0 / Spark 2.4.5 GraphX, not vendored; see SURVEY.md §2.2
 * U1-U5).  Semantics: SURVEY.md Appendix A (LPA-DET) and Appendix B
 * (OUTLIER-DET).  Bindings a host would add: INTEGRATION.md.
 *
 * Conventions
 *   - vertex ids are dense int32 in [0, V); the dense order is the ascending
 *     order of the caller's original ids, so "smallest label" is preserved;
 *   - every function returns LPA_OK (0) or a negative LPA_E* code; the
 *     message is available from lpa_last_error() (thread-local);
 *   - calls block until the device work they issued has finished;
 *   - a handle is not thread-safe; distinct handles are independent.
 */
#ifndef LPA_H_
#define LPA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPA_OK 0
#define LPA_EINVAL (-22)   /* bad argument (maxIter <= 0, id out of range, ...) */
#define LPA_ENOMEM (-12)   /* device or host allocation failed                  */
#define LPA_ENODEV (-19)   /* no HIP device / bad device ordinal                */
#define LPA_EHIP (-1000)   /* HIP runtime error                                  */
#define LPA_ERCCL (-2000)  /* RCCL error                                         */
#define LPA_EOVERFLOW (-75) /* kernel-side capacity overflow (hub combine table) */

/* lpa_graph_create* flags */
#define LPA_INPUT_DEVICE 0x1u /* src/dst are device pointers on `device`        */

#define LPA_NBINS 13   /* 0 seg 1 w16 2 w8 3 w4 4 w2 5 g64 6 g32 7 g16 8 g8 9 g4 10 g2 11 g1 12 isolated */
#define LPA_NKERNELS 17 /* timed: 0 seg 1 hub 2 w16 3 w8 4 w4 5 w2 6 g64 7 g32 8 g16 9 g8 10 g4 11 g2 12 g1
                          13 refresh (diff + al[] scatter) 14 al[] rebuild 15 frontier lists
                          16 block-per-row hub tally (label-dense supersteps) */
#define LPA_STATS_MAX_ITERS 64

typedef struct lpa_graph lpa_graph;

/* Per-call timing, filled by lpa_step / lpa_run (HIP events on the handle's stream).
 * iter_ms: always (events around each superstep; converged single-GPU supersteps
 * still replay their captured graph).  kernel_ms / exchange_ms: only on a handle in
 * the serialized profiling schedule (lpa_set_serial(g, 1)), where events bracket
 * every tally kernel so each time is that kernel's standalone duration. */
typedef struct lpa_stats {
  int32_t iters;                           /* supersteps executed by this call          */
  int32_t n_iter_ms;                       /* entries filled in iter_ms                 */
  float iter_ms[LPA_STATS_MAX_ITERS];      /* device time per superstep (incl. exchange) */
  float kernel_ms[LPA_NKERNELS];           /* summed device time per kernel (serial)    */
  float exchange_ms;                       /* summed label-exchange time (serial)       */
  double total_ms;                         /* device time of all supersteps of the call */
} lpa_stats;

/* Layout facts of a built graph (this rank's slice). */
typedef struct lpa_graph_info {
  int64_t V;            /* vertices (global)                                  */
  int64_t m;            /* input directed edges (global)                      */
  int64_t arcs;         /* symmetrised arcs owned by this rank (= 2m at P=1)  */
  int64_t slice;        /* vertex slots per rank (V padded to P * slice)      */
  int64_t own_begin;    /* first global (internal) vertex slot of this rank   */
  int32_t rank, nranks, device;
  int32_t max_degree;   /* global maximum symmetrised degree                  */
  int64_t bin_vertices[LPA_NBINS]; /* degree bins, see LPA_NBINS */
  int64_t bin_arcs[LPA_NBINS];
  int64_t hub_vertices; /* vertices split over several segments (global merge) */
  int64_t segments;     /* segment count of bin 0                             */
  int64_t device_bytes; /* device memory held by the handle                   */
  int64_t exchanges_full;  /* P > 1: label exchanges done as a full allgather   */
  int64_t exchanges_delta; /* P > 1: label exchanges done as changed-label deltas */
  int64_t exchanges_giant; /* P > 1: label exchanges done giant-compressed (bitmap of the
                              giant label + changed non-giant labels) */
  int64_t blocked_rows;    /* P = 1: rows whose columns are in (class, column) order for
                              the class-blocked al[] rebuild (0: off, LPA_BLOCK_DEG)  */
  int64_t blocked_pieces;  /* ... and the rebuild's piece-list length                */
  int64_t code_refresh;    /* 1: the last refresh took the giant codes (the next superstep
                              settles rows from 2-bit label codes; every
                              rank of a partitioned job since ABI 7) -- read after a
                              superstep-1 step; 0 otherwise (since ABI 6)              */
  int64_t graph_replays;   /* supersteps run by replaying a captured HIP graph (the
                              converged ones, P = 1 also supersteps 2-3; since ABI 6)  */
  int64_t exchanges_posted; /* P > 1: delta exchanges sent at a capacity fixed before the
                              count read, so the GPU works through it (since ABI 6)   */
  int64_t exchanges_post_missed; /* ... posted ones whose counts exceeded the posted
                              capacity: exchanged again in the form that fits          */
  int64_t gather_mode;     /* 1: the tallies read L[col[i]] and no al[] refresh runs (one
                              GPU, label vector <= 4 MB, no row above 128 arcs; since ABI 6) */
  int64_t host_allgathers; /* allgathers served by the host collective's function
                              (lpa_graph_create_hostcoll; since ABI 7)                 */
  int64_t sparse_refreshes; /* refreshes since the build or the last reset that left al[]
                              sparse: a one-GPU bits-mode rebuild carries the arcs on the
                              giant label in the arc giant bits and stores only the other
                              arcs' labels (LPA_SPARSE_AL=0: never; since ABI 15)      */
  int64_t fill_refreshes;  /* ... those of them that took the fill-scatter form: every arc
                              bit set, then only the columns off the giant label visited
                              through the CSC index (LPA_FILL_SCATTER=0: never; since ABI 17;
                              superstep 3's refresh in that form, LPA_FILL_STEP3, counts too) */
} lpa_graph_info;

/* Outlier summary. */
typedef struct lpa_outlier_summary {
  int64_t n_groups;      /* L1: distinct communities; L2: distinct (community, sub-label) groups */
  int64_t k;             /* L1: n_groups / 10                                        */
  int64_t threshold;     /* L1: size threshold (flag iff size < threshold)           */
  int64_t n_flagged;     /* vertices flagged                                         */
  int64_t n_communities; /* distinct top-level communities                           */
  int64_t n_communities_flagged; /* L2: communities with >= 1 flagged sub-community  */
  int64_t distinct_edges;        /* distinct directed (s,d) pairs                     */
} lpa_outlier_summary;

/*
 * Build the symmetrised, degree-sorted CSR of the multigraph (src[i], dst[i]),
 * i < m, on HIP device `device`.  Duplicate edges are kept (each is a vote),
 * a self-loop gives two votes (GraphX sendMessage both ways).
 * Replaces: GraphFrame.__init__ + cachedTopologyGraphX / GraphX Graph build
 * (Graphframes.py:78; U1, U2, U5 in SURVEY.md §2.2).
 */
int lpa_graph_create(const int32_t* src, const int32_t* dst, int64_t m, int32_t V,
                     int32_t device, uint32_t flags, lpa_graph** out);

/* RCCL unique id (128 bytes) for lpa_graph_create_dist; produced on one rank and
 * broadcast by the caller (MPI, torch.distributed, ...). */
int lpa_comm_unique_id(uint8_t id_out[128]);

/*
 * Multi-GPU build: one process per GPU.  Every rank passes the SAME edge list;
 * the rank keeps the CSR rows of its vertex slice (degree-ranked round-robin
 * 1D partition) and refreshes the replicated label vector with one RCCL
 * allgather per superstep.  Results are bit-identical to
 * the single-GPU build.  Replaces the Spark shuffle of aggregateMessages (U5).
 * comm_id == NULL with nranks > 1 selects the caller-driven exchange below.  A
 * comm_id with nranks == 1 builds a one-rank job of the same path (the exchange
 * step and its ncclAllGather run every superstep; labels as lpa_graph_create).
 */
int lpa_graph_create_dist(const int32_t* src, const int32_t* dst, int64_t m, int32_t V,
                          int32_t device, uint32_t flags, int32_t rank, int32_t nranks,
                          const uint8_t comm_id[128], lpa_graph** out);

/*
 * In-process loopback collective (SURVEY.md §8(e) "fake backend"): P handles on ONE
 * device, each created with lpa_graph_create_loopback and driven by its OWN host
 * thread (lpa_run / lpa_step concurrently, as P processes would).  The library's
 * exchange runs unchanged -- full/delta switch, host count read, in-place
 * allgather, delta chain -- with the allgather done as stream-ordered D2D copies
 * between the handles instead of ncclAllGather.  lpa_loopback_destroy on a group
 * that still has handles attached aborts it (their collectives fail) and leaves the
 * free to the last handle's lpa_graph_destroy.  lpa_loopback_abort releases every thread waiting in a collective
 * (each then fails with LPA_ERCCL); a rank whose peers never arrive fails the
 * same way after 300 s.
 */
/*
 * Host-staged collective (round 6): the same in-library exchange as the RCCL path --
 * full / delta / giant-compressed forms, the posted delta and its stand-down, the
 * per-rank count triple -- with every allgather handed to the caller's host function:
 *   allgather(send, recv, bytes_per_rank, ctx) gathers every rank's `bytes_per_rank`
 *   bytes from `send` into `recv` in rank order (nranks * bytes_per_rank bytes) and
 *   returns 0 (non-zero: the superstep fails with LPA_ERCCL).
 * Both buffers are pinned host memory owned by the library, valid during the call; the
 * function runs on the thread that called lpa_step / lpa_run, once per allgather, and
 * every rank calls it the same number of times with the same size.  For clusters
 * without RCCL between the ranks: MPI_Allgather, torch.distributed (gloo), a Spark
 * barrier stage moving the bytes through the driver.  PCIe-staged: the RCCL build
 * (lpa_graph_create_dist with a comm id) is the fast path between MI355X GPUs.
 */
typedef int (*lpa_allgather_fn)(const void* send, void* recv, int64_t bytes_per_rank, void* ctx);
int lpa_graph_create_hostcoll(const int32_t* src, const int32_t* dst, int64_t m, int32_t V,
                              int32_t device, uint32_t flags, int32_t rank, int32_t nranks,
                              lpa_allgather_fn allgather, void* ctx, lpa_graph** out);

typedef struct lpa_loopback lpa_loopback;
int lpa_loopback_create(int32_t nranks, lpa_loopback** out);
void lpa_loopback_abort(lpa_loopback* group);
void lpa_loopback_destroy(lpa_loopback* group);
int lpa_graph_create_loopback(const int32_t* src, const int32_t* dst, int64_t m, int32_t V,
                              int32_t device, uint32_t flags, int32_t rank, lpa_loopback* group,
                              lpa_graph** out);

/*
 * Caller-driven label exchange (a handle built by lpa_graph_create_dist with
 * nranks > 1 and comm_id == NULL performs no RCCL collective): after each
 * lpa_step(g, 1) the caller collects every rank's owned slice of the current
 * label vector (lpa_exchange_get: `slice` entries, internal slot order) and
 * writes the concatenation of all slices in rank order back to every rank
 * (lpa_exchange_put: nranks * slice entries).  Used to test the partitioned
 * path with P virtual ranks on one device (SURVEY.md §8(e) fake backend).
 * Host buffers.
 */
int lpa_exchange_get(lpa_graph* g, int32_t* slice_out);
int lpa_exchange_put(lpa_graph* g, const int32_t* full_in);
/*
 * Delta form of the caller-driven exchange (the protocol the in-library RCCL
 * exchange uses in converged supersteps, lpa_exchange.hip): after lpa_step(g, 1)
 * lpa_exchange_get_delta returns this rank's CHANGED owned labels as
 * (local slot << 32 | label) entries (entries_out: room for `slice` entries) and
 * their count; the caller lays every rank's entries out as [nranks][cap]
 * (cap >= every count, cap <= slice / 4) and passes them with the counts to
 * lpa_exchange_put_delta on every rank.  Host buffers.
 */
int lpa_exchange_get_delta(lpa_graph* g, uint64_t* entries_out, int64_t* count_out);
int lpa_exchange_put_delta(lpa_graph* g, const uint64_t* entries, const int64_t* counts, int64_t cap);

/* Profiling control: serial != 0 queues every tally kernel on the handle's main
 * stream (no concurrent bins), so per-kernel times in lpa_stats are standalone
 * durations.  Labels are identical either way. */
int lpa_set_serial(lpa_graph* g, int32_t serial);
/* Frontier (default on; LPA_FRONTIER=0 at create time turns it off): a superstep
 * re-tallies only the rows with a neighbour whose label changed in the previous
 * superstep -- exact, since a row whose neighbourhood labels are unchanged has the
 * same mode (GraphX Pregel's active-set idea applied to LPA).  Off: every row is
 * tallied every superstep.  Labels are identical either way. */
int lpa_set_frontier(lpa_graph* g, int32_t on);
/* P > 1 with a communicator or loopback group: capacity of the posted delta exchange
 * (converged supersteps after a delta exchange: the changed-label entries go out at a
 * capacity fixed before the per-rank counts are read, so the GPU works through the
 * host's read; a count above it makes the queued apply stand down and the host exchange
 * again in the form that fits).  cap < 0: adaptive (default: twice the last largest
 * count, 1024..131072 entries); 0: off (the host reads the counts first); > 0: that
 * fixed capacity (testing: 1 exercises the stand-down path).  The value is this rank's
 * REQUEST: it travels with the next per-rank count exchange and every rank posts the
 * smallest capacity requested by any rank (0 if any rank turned posting off), from the
 * superstep after that exchange on -- so ranks never disagree on the allgather size,
 * whichever ranks call this and when.  Labels are identical either way.  Since ABI 6. */
int lpa_set_posted(lpa_graph* g, int64_t cap);
/* Run on a caller-provided hipStream_t (NULL = the handle's own stream). */
int lpa_set_stream(lpa_graph* g, void* hip_stream);

/* Labels := L0 (every vertex its own id; LabelPropagation.run mapVertices(vid => vid)). */
int lpa_reset(lpa_graph* g);

/* Continue the synchronous BSP loop by n_supersteps (Pregel.apply iterations). */
int lpa_step(lpa_graph* g, int32_t n_supersteps, lpa_stats* stats /* nullable */);

/* Current labels indexed by dense vertex id; out is host memory unless out_is_device. */
int lpa_get_labels(lpa_graph* g, int32_t* labels_out, int32_t out_is_device);

/*
 * labelPropagation(maxIter): reset + max_iter supersteps + labels.
 * max_iter <= 0 -> LPA_EINVAL ("Maximum of steps must be greater than 0", U3 require).
 * Replaces: GraphFrame.labelPropagation -> lib.LabelPropagation.run ->
 * graphx.lib.LabelPropagation.run -> Pregel.apply (Graphframes.py:81).
 */
int lpa_run(lpa_graph* g, int32_t max_iter, int32_t* labels_out, int32_t out_is_device,
            lpa_stats* stats /* nullable */);

/*
 * Outlier stage over `labels` (dense-id indexed; host unless labels_on_device).
 * mode 1 = L1 (top-level community-size threshold), mode 2 = L2 (second LPA of
 * sub_iter supersteps on the intra-community distinct-edge subgraph, threshold
 * per community).  Outputs are host arrays of V entries, each nullable:
 *   size_hist[l]   members of community l              (Graphframes.py:100-104, :120)
 *   incident[l]    distinct directed edges touching l  (Graphframes.py:107-118)
 *   sub_labels[v]  L2 only: second-level label         (Graphframes.py:121-128)
 *   flags[v]       1 = outlier                          (Graphframes.py:130-137)
 * The first call on a handle builds its distinct directed edge set (topology) and a
 * pinned host staging area of 25 bytes per vertex for the host copies; both are kept
 * with the handle and released by lpa_graph_destroy.
 */
int lpa_outlier(lpa_graph* g, const int32_t* labels, int32_t labels_on_device, int32_t mode,
                int32_t sub_iter, int64_t* size_hist, int64_t* incident, int32_t* sub_labels,
                uint8_t* flags, lpa_outlier_summary* summary);

/* The same stage with every array on the device (`device` of the handle): labels in,
 * size_hist / incident (int64[V]), sub_labels (int32[V], L2) and flags (uint8[V]) out,
 * each output nullable; no host staging (the pipeline form: labels straight from
 * lpa_run(..., out_is_device = 1), results consumed on the GPU). */
int lpa_outlier_device(lpa_graph* g, const int32_t* labels, int32_t mode, int32_t sub_iter,
                       int64_t* size_hist, int64_t* incident, int32_t* sub_labels, uint8_t* flags,
                       lpa_outlier_summary* summary);

/* Partition quality of a labelling (dense ids, values in [0, V)) on the handle's
 * symmetrised multigraph, the graph labelPropagation votes on (A = 2m arcs: every
 * input edge both ways, a self-loop as two arcs at its vertex):
 *   modularity = intra_arcs / A - degree_term,  degree_term = sum_c (D_c / A)^2,
 * D_c the degree sum of community c, plus the community count (the distinct-label
 * count of Graphframes.py:85).  Exact integer sums on the device.  North-star
 * "community-count / modularity agreement" report; not a GraphFrames call.
 * On a distributed job (nranks > 1) only rank 0 keeps the edge list this needs; the
 * other ranks return LPA_EINVAL. */
typedef struct lpa_quality_summary {
  int64_t n_communities;
  int64_t intra_arcs;
  int64_t arcs;
  double degree_term;
  double modularity;
} lpa_quality_summary;
int lpa_quality(lpa_graph* g, const int32_t* labels, int32_t labels_on_device, lpa_quality_summary* out);

/*
 * Connected components of the undirected view of the input multigraph (edge direction,
 * duplicate edges and self-loops make no difference; a vertex with no edge is its own
 * component).  comp_out[v], by dense id, is the SMALLEST dense id of v's component:
 * GraphX's "lowest vertex id in the component", and for integral ids the value
 * GraphFrame.connectedComponents returns.  A pure function of (V, edge set): identical
 * across runs, edge orders, handles and devices.  size_out (nullable, V entries):
 * size_out[c] = members of the component whose id is c, 0 at every other index.  Both
 * arrays are host memory unless out_is_device; summary is nullable.  V == 0: success,
 * nothing written.  Concurrent union-find over the kept edge list (one pass); the labels
 * and every other piece of lpa_step's state are neither read nor written, nothing is kept
 * on the handle.  On a distributed job (nranks > 1) only rank 0 keeps the edge list this
 * needs; the other ranks return LPA_EINVAL.  Since ABI 8.
 */
typedef struct lpa_components_summary {
  int64_t n_components;  /* components, single vertices included            */
  int64_t n_singletons;  /* components of exactly one vertex                */
  int64_t largest_size;  /* members of the largest component (0 if V == 0)  */
  int64_t largest_id;    /* its id; the smallest id on a tie; -1 if V == 0  */
} lpa_components_summary;
int lpa_components(lpa_graph* g, int32_t* comp_out, int32_t out_is_device,
                   int64_t* size_out, lpa_components_summary* summary);

/*
 * Triangles per vertex (GraphX TriangleCount / GraphFrame.triangleCount) of the canonical
 * simple undirected graph of the input multigraph: self-loops dropped, direction ignored,
 * duplicates collapsed (a->b, b->a and any number of repeats of either are one edge {a,b}).
 * count_out[v], by dense id (V entries, required), is the number of unordered vertex
 * triples containing v that are pairwise adjacent; its sum is 3 T; a vertex in no triangle,
 * or with no edge, gets 0.  int64: a hub can sit in more than 2^31 triangles.  A pure
 * function of (V, edge set): identical across runs, edge orders, edge directions, handles
 * and devices.  simple_degree_out (nullable, V entries): d(v), the distinct neighbours of v
 * other than v.  Both arrays are host memory unless out_is_device; summary is nullable.
 * V == 0: success, nothing written, summary {0,0,0,0,0,-1}.  The call blocks until the
 * work is done.  Sorted-set intersection over the simple graph oriented by (degree, id)
 * (DESIGN.md "Triangle counting"); all working memory is stream-ordered temporaries, the
 * labels and every other piece of lpa_step's state are neither read nor written, nothing
 * is kept on the handle.  On a distributed job (nranks > 1) only rank 0 keeps the edge
 * list this needs; the other ranks return LPA_EINVAL.  Since ABI 9.
 */
typedef struct lpa_triangle_summary {
  int64_t n_triangles;    /* T = sum(count) / 3                                        */
  int64_t simple_edges;   /* undirected distinct non-loop edges                        */
  int64_t wedges;         /* sum_v d(v) (d(v) - 1) / 2, d = simple degree              */
  int64_t n_in_triangle;  /* vertices with count > 0                                   */
  int64_t max_count;      /* largest count (0 if none)                                 */
  int64_t max_count_id;   /* its dense id, the smallest on a tie; -1 if V == 0         */
} lpa_triangle_summary;   /* 48 bytes */
int lpa_triangle_count(lpa_graph* g, int64_t* count_out, int64_t* simple_degree_out,
                       int32_t out_is_device, lpa_triangle_summary* summary);

/*
 * Static PageRank (GraphX PageRank.runWithOptions / GraphFrame.pageRank(maxIter)) of the
 * DIRECTED input multigraph as given: every kept edge is an edge, a duplicate one more, a
 * self-loop one edge from the vertex to itself.  IEEE binary64 throughout.  With
 * outdeg[u] = the kept edges leaving u, w[u] = 1.0 / outdeg[u] (0.0 for a sink, never
 * read there), a = reset_prob:
 *   start   r[v] = 1.0; with a source (source >= 0, a dense id), 1.0 at the source, else 0.0
 *   step    max_iter times, every read of the previous r:
 *             c[u] = r[u] * w[u];  s[v] = sum of c[u] over the edges u -> v (0.0 with none)
 *             r[v] = a + (1.0 - a) * s[v]; with a source, (v == source ? a : 0.0) + (1.0 - a) * s[v]
 *   finish  S = sum r;  r[v] *= (double)V / S; with a source, r[v] /= S
 * A sink's mass is lost in a step (GraphX's behaviour); the finish makes up for it.  With
 * a = 0 and no source a graph in which every walk dies gives S == 0 and whatever IEEE
 * gives for V / 0.  rank_out (V entries, required) by dense id; out_degree_out and
 * in_degree_out (nullable, V entries, int64, duplicates counted).  The arrays are host
 * memory unless out_is_device; summary is nullable.  V == 0: success, nothing written,
 * summary {0, 0, -1, 0, 0, 0}.  LPA_EINVAL for max_iter <= 0, reset_prob outside [0, 1]
 * or NaN, source outside [-1, V), a null rank_out with V > 0.  The call blocks until the
 * work is done.  A pull over the in-lists of a CSR sorted by (dst, src), without a single
 * floating-point atomic: every sum has a shape fixed by the row's length, the handle's
 * form boundaries and V, so the ranks are bit-identical across runs, handles and input
 * edge orders (DESIGN.md "PageRank"); two implementations of the same max_iter = k differ
 * per vertex by a relative 2 (k (D + 2) + V + 2) 2^-53 at most, D the largest in-degree.
 * All working memory is stream-ordered temporaries, the labels and every other piece of
 * lpa_step's state are neither read nor written, nothing is kept on the handle.  On a
 * distributed job (nranks > 1) only rank 0 keeps the edge list this needs; the other
 * ranks return LPA_EINVAL.  Since ABI 10.
 */
typedef struct lpa_pagerank_summary {
  double  rank_sum;      /* S before normalisation                               */
  double  max_rank;      /* largest normalised rank (0 if V == 0)                */
  int64_t max_rank_id;   /* its dense id, the smallest on a tie; -1 if V == 0    */
  int64_t edges;         /* kept directed edges, duplicates counted              */
  int64_t sinks;         /* vertices with out-degree 0                           */
  int64_t max_in_degree; /* with multiplicity                                    */
} lpa_pagerank_summary;  /* 48 bytes */
int lpa_pagerank(lpa_graph* g, int32_t max_iter, double reset_prob, int32_t source /* -1: none */,
                 double* rank_out, int64_t* out_degree_out, int64_t* in_degree_out,
                 int32_t out_is_device, lpa_pagerank_summary* summary);

/*
 * Parallel personalized PageRank (GraphX PageRank.runParallelPersonalizedPageRank /
 * GraphFrame.parallelPersonalizedPageRank(resetProbability, sourceIds, maxIter)): n_sources
 * personalised ranks of the DIRECTED input multigraph in one call.  Row l of rank_out is
 * exactly what lpa_pagerank specifies for source = sources[l] (the same graph, w, a, start,
 * step and finish, IEEE binary64 without contraction into fused multiply-adds):
 *   start   r_l[v] = (v == sources[l]) ? 1.0 : 0.0
 *   step    max_iter times, every read of the previous r_l:
 *             c_l[u] = r_l[u] * w[u];  s_l[v] = sum of c_l[u] over the edges u -> v
 *             r_l[v] = (v == sources[l] ? a : 0.0) + (1.0 - a) * s_l[v]
 *   finish  S_l = sum_v r_l[v];  r_l[v] /= S_l
 * A source may repeat: its rows are then equal (GraphX keeps only the last of a repeat and
 * returns 0 / 0 for the earlier ones; that accident is not reproduced).  S_l == 0 (a = 0 and
 * a walk that dies) gives whatever IEEE gives.  sources (dense ids) is always host memory;
 * rank_out ([n_sources][V] row-major: rank_out[l * V + v]) is host memory unless
 * out_is_device; rank_sum_out (nullable, n_sources entries: S_l) is always host memory;
 * summary is nullable.  n_sources == 0 or V == 0: success, nothing written, summary all zeros
 * except that edges, sinks and max_in_degree are still filled when V > 0.  LPA_EINVAL for
 * max_iter <= 0, reset_prob outside [0, 1] or NaN, n_sources < 0, a null sources or (with
 * V > 0) rank_out when n_sources > 0, a source outside [0, V).  The call blocks until the
 * work is done.  The in-list CSR of lpa_pagerank is built once per call; the sources then
 * run batch_width to a pass (LPA_PPR_BATCH = 4, 8 or 16 at handle creation; anything else:
 * the default), their c[] and r[] values interleaved so that one gathered in-edge serves
 * the whole pass from 8 batch_width contiguous bytes (DESIGN.md "Parallel personalized
 * PageRank").  No floating-point atomics: every column's sums have a shape fixed by the
 * row's length, the handle's form boundaries, V and the batch width, so row l and S_l are
 * a function of (V, edge multiset, form boundaries, batch width, max_iter, reset_prob,
 * sources[l]) alone: bit-identical across runs, handles, input edge orders, the position of
 * the source in sources and whatever other sources share the call.  They agree with
 * lpa_pagerank's personalised ranks within its bound, 2 (k (D + 2) + V + 2) 2^-53 relative;
 * they need not be bit-equal to them.  The batch width changes bits within that bound, never
 * an integer of the summary.  All working memory is stream-ordered temporaries, the labels
 * and every other piece of lpa_step's state are neither read nor written, nothing is kept on
 * the handle.  On a distributed job (nranks > 1) only rank 0 keeps the edge list this needs;
 * the other ranks return LPA_EINVAL.  Since ABI 13.
 */
typedef struct lpa_ppr_summary {
  int64_t edges, sinks, max_in_degree;   /* as lpa_pagerank_summary                          */
  int64_t batches;       /* passes = ceil(n_sources / batch_width); 0 with none             */
  int64_t batch_width;   /* sources to a pass on this handle                                */
  int64_t nonzero;       /* (source, vertex) pairs with rank > 0                            */
  double  rank_sum_min, rank_sum_max;  /* smallest / largest S_l (0.0 with no source)        */
} lpa_ppr_summary;       /* 64 bytes */
int lpa_parallel_pagerank(lpa_graph* g, int32_t max_iter, double reset_prob,
                          const int32_t* sources /* host, dense ids */, int32_t n_sources,
                          double* rank_out /* [n_sources][V] row-major */, int32_t out_is_device,
                          double* rank_sum_out /* nullable, host, n_sources: S_l */,
                          lpa_ppr_summary* summary /* nullable */);

/*
 * Landmark shortest paths (GraphX lib.ShortestPaths / GraphFrame.shortestPaths(landmarks))
 * of the DIRECTED input graph: dist_out[l * V + v] is the number of edges on a shortest
 * directed path from vertex v to landmarks[l] along src -> dst (GraphX sends its messages
 * from dst to src: distances are TO the landmark), 0 at the landmark itself, -1 where no
 * path exists.  Duplicate edges and self-loops change nothing; an edge with an end outside
 * [0, V) is not an edge.  landmarks (dense ids) is always host memory; a landmark may repeat,
 * its rows are then equal.  dist_out ([n_landmarks][V] row-major int32) is host memory unless
 * out_is_device; summary is nullable.  n_landmarks == 0: success, nothing written, summary
 * {arcs, 0, -1, 0, 0, 0} ({0, 0, -1, 0, 0, 0} with V == 0).  LPA_EINVAL for n_landmarks < 0,
 * a null landmarks or (with V > 0) dist_out when n_landmarks > 0, a landmark outside [0, V).
 * The call blocks until the work is done.  A multi-source breadth-first search over the
 * reversed arcs, 64 landmarks to a pass (one bit each of a 64-bit word per vertex), every
 * level either a push along the frontier's in-lists (64-bit atomic ORs) or a pull over the
 * out-lists of the unfinished vertices (no atomics), chosen per level by Beamer's rule
 * (DESIGN.md "Shortest paths").  OR commutes: the distances and every summary field but
 * push_levels / pull_levels are a function of (V, edge set, landmarks) alone, identical
 * across runs, handles, input edge orders and schedules; push_levels + pull_levels is the
 * sum over the passes of (the pass's largest distance + 1).  All working memory is
 * stream-ordered temporaries, the labels and every other piece of lpa_step's state are
 * neither read nor written, nothing is kept on the handle.  On a distributed job
 * (nranks > 1) only rank 0 keeps the edge list this needs; the other ranks return
 * LPA_EINVAL.  Since ABI 11.
 */
typedef struct lpa_sp_summary {
  int64_t arcs;         /* distinct directed non-loop arcs the search walks              */
  int64_t reached;      /* finite (landmark, vertex) pairs, the landmarks themselves included */
  int64_t max_distance; /* largest finite distance; -1 if n_landmarks == 0 or V == 0     */
  int64_t batches;      /* passes of up to 64 landmarks = ceil(n_landmarks / 64)         */
  int64_t push_levels;  /* levels expanded frontier -> predecessors (all batches)        */
  int64_t pull_levels;  /* levels in which unfinished vertices scanned their out-lists   */
} lpa_sp_summary;       /* 48 bytes */
int lpa_shortest_paths(lpa_graph* g, const int32_t* landmarks /* host, dense ids */,
                       int32_t n_landmarks, int32_t* dist_out /* [n_landmarks][V] row-major */,
                       int32_t out_is_device, lpa_sp_summary* summary /* nullable */);

/*
 * Betweenness centrality (this package's GraphFrame.betweennessCentrality; the definition is
 * networkx.betweenness_centrality's) by Brandes' algorithm from a set S of sources.  The graph
 * is the simple directed graph of the input: the distinct arcs src -> dst with src != dst and
 * both ends in [0, V); duplicate edges and self-loops change nothing.  directed == 0: every arc
 * also counts in the other direction (the simple undirected graph of lpa_triangle_count and
 * lpa_core_numbers).  For every vertex v
 *   raw_out[v] = sum over s in S, s != v, of delta_s(v)
 *   delta_s(v) = sum over the arcs v -> w with level_s(w) == level_s(v) + 1
 *                of sigma_s(v) / sigma_s(w) * (1 + delta_s(w))
 * level_s the breadth-first distance from s, sigma_s the number of shortest paths from s, 0
 * where s does not reach v.  raw_out is UNSCALED: with S = every vertex, raw (directed) and
 * raw / 2 (undirected) are networkx's unnormalised values; with a subset the caller applies
 * V / |S| (the pivot estimate).  sigma is binary64, as in networkx: above 2^53 the path counts
 * are rounded, the result is still deterministic.  sources (distinct dense ids) is always
 * host memory; null means every vertex, 0 ... V - 1 in order, and n_sources is then ignored.
 * raw_out ([V] binary64) is host memory unless out_is_device; summary is nullable.  batch: the
 * sources to a pass, 1, 4, 8 or 16; 0: the handle's (LPA_BC_BATCH = 1, 4, 8 or 16 at handle
 * creation; anything else: the default).  V == 0: success, nothing written, summary {0, 0, 0,
 * 0, 0, -1, 0}.  n_sources == 0 with a non-null sources: raw_out all zeros, max_depth -1.
 * LPA_EINVAL for n_sources < 0, a source outside [0, V), a repeated source, a batch outside
 * {0, 1, 4, 8, 16}, a null raw_out with V > 0.  The call blocks until the work is done.  The
 * out-lists and in-lists of the arcs are built once per call; the sources then run batch_width
 * to a pass in lockstep by level, their level, sigma and delta values interleaved per vertex so
 * that one gathered arc serves the whole pass from one contiguous piece: forward, a level's
 * new vertices are discovered by integer atomic ORs of slot masks along the frontier's out-lists
 * and then pull their sigma over their in-lists; backward, level by level, the vertices of a
 * level pull their delta over their out-lists (DESIGN.md "Betweenness centrality").  If the
 * state of the chosen width cannot be allocated the call falls back to a narrower one before it
 * returns LPA_ENOMEM; batch_width tells.  No floating-point atomics: every sum has a shape
 * fixed by the row's length and form, the same at every batch width and slot, and a pass adds
 * its deltas into raw_out in source order, so raw_out is a function of (V, arc set, sources in
 * their order) alone: bit-identical across runs, handles, input edge orders and batch widths.
 * All working memory is stream-ordered temporaries, the labels and every other piece of
 * lpa_step's state are neither read nor written, nothing is kept on the handle.  On a
 * distributed job (nranks > 1) only rank 0 keeps the edge list this needs; the other ranks
 * return LPA_EINVAL.  Since ABI 22.
 */
typedef struct lpa_bc_summary {
  int64_t arcs;         /* distinct non-loop arcs walked (both orientations when undirected) */
  int64_t sources;      /* |S|                                                              */
  int64_t batches;      /* passes = ceil(|S| / batch_width); 0 with none                    */
  int64_t batch_width;  /* B: sources to a pass in this call                                */
  int64_t reached;      /* sum over sources of the vertices given a level, the source included */
  int64_t max_depth;    /* largest level of any source; -1 if no source or V == 0           */
  int64_t levels;       /* sum over passes of (the pass's largest level + 1)                */
} lpa_bc_summary;       /* 56 bytes */
int lpa_betweenness(lpa_graph* g, const int32_t* sources /* host dense ids; null = every vertex */,
                    int32_t n_sources, int32_t directed, int32_t batch /* 0: the library's */,
                    double* raw_out /* [V], unscaled */, int32_t out_is_device,
                    lpa_bc_summary* summary /* nullable */);

/*
 * Breadth-first search between two vertex sets (GraphFrames lib.BFS / GraphFrame.bfs(fromExpr,
 * toExpr, edgeFilter, maxPathLength)) over the DIRECTED input graph.  F = the vertices with
 * from_mask != 0, T = those with to_mask != 0; the kept edges are the input edges with
 * edge_keep != 0 (null: all of them).  m and the edge order are the handle's input edge list.
 * An edge with an end outside [0, V) is no edge; a self-loop is never on a path.  L = the
 * smallest number of kept, non-loop edges on a directed path src -> dst from a vertex of F to a
 * vertex of T.  With 1 <= L <= max_len the result describes EVERY path of L edges from F to T
 * (GraphFrames' result rows, which the caller enumerates): level_out[v] = i for a vertex that is
 * the i-th of such a path (0 in F, L in T), -1 for every other vertex; on_edge_out[e] = 1 for an
 * input edge e = (a, b) that is kept, no loop, and has level_out[a] >= 0 and level_out[b] ==
 * level_out[a] + 1 (a duplicate edge is marked like its twin: one more path), 0 elsewhere.  The
 * result paths are exactly the walks over marked edges from level 0 to level L.
 *   F or T empty           length = -1, every level -1, no edge marked, reached = 0; no search
 *   F and T share a vertex length = 0, level_out = 0 exactly on their common vertices, no edge
 *                          marked, reached = |F|; no search
 *   max_len == 0           can only give 0 or -1
 *   no path of <= max_len  length = -1, every level -1, no edge marked
 * V == 0: success, nothing written but the summary ({0, 0, 0, -1, 0, 0, 0, 0, 0}).  LPA_EINVAL for
 * max_len < 0, for a null mask or level_out with V > 0, for a null on_edge_out with V > 0 and
 * m > 0.  The three masks and the two outputs are host memory; summary is nullable (arcs is
 * counted only when it is given or a search runs).  The call blocks until the work is done.
 * One bit per vertex (bitmaps of ceil(V / 64) words); every level either a push along the
 * frontier's out-lists (64-bit atomic ORs of one bit) or a pull in which every unseen vertex
 * scans its in-list up to the first frontier vertex, chosen per level by Beamer's rule; the
 * search stops at the first level that holds a vertex of T, at an empty frontier or at max_len;
 * a backward sweep then keeps, level by level, the vertices with an arc to a kept vertex of the
 * next level (DESIGN.md "Breadth-first search").  OR commutes: both outputs and every summary
 * field but push_levels / pull_levels are a function of (V, edge list, masks, max_len) alone,
 * identical across runs, handles and schedules; level_out is also identical across input edge
 * orders and on_edge_out follows its edges through a permutation.  push_levels + pull_levels is
 * L when a path is found, otherwise the levels expanded before the frontier emptied or max_len
 * was reached.  All working memory is stream-ordered temporaries, the labels and every other
 * piece of lpa_step's state are neither read nor written, nothing is kept on the handle.  On a
 * distributed job (nranks > 1) only rank 0 keeps the edge list this needs; the other ranks
 * return LPA_EINVAL.  Since ABI 18.
 */
typedef struct lpa_bfs_summary {
  int64_t arcs;          /* distinct directed non-loop arcs of the kept edges                 */
  int64_t sources;       /* |F|                                                               */
  int64_t targets;       /* |T|                                                               */
  int64_t length;        /* L; 0 if F and T share a vertex; -1 if no path within max_len      */
  int64_t reached;       /* vertices the forward search gave a level, F included              */
  int64_t path_vertices; /* vertices on a result path (F∩T's size when length == 0)           */
  int64_t path_edges;    /* input edges marked in on_edge_out                                 */
  int64_t push_levels;
  int64_t pull_levels;   /* forward levels by form; their sum = levels expanded               */
} lpa_bfs_summary;       /* 72 bytes */
int lpa_bfs(lpa_graph* g,
            const uint8_t* from_mask /* [V] host, nonzero = in F */,
            const uint8_t* to_mask   /* [V] host */,
            const uint8_t* edge_keep /* [m] host, nullable = keep all */,
            int32_t max_len,
            int32_t* level_out  /* [V] host: lev of a path vertex, -1 elsewhere */,
            uint8_t* on_edge_out /* [m] host: 1 for an input edge on a result path */,
            lpa_bfs_summary* summary /* nullable */);

/*
 * Strongly connected components (GraphX lib.StronglyConnectedComponents /
 * GraphFrame.stronglyConnectedComponents(maxIter)) of the DIRECTED input graph.  Duplicate
 * edges change nothing; an edge with an end outside [0, V) is not an edge; a self-loop is kept
 * as a fact about its vertex: it never changes the converged result, but it does change the
 * round in which the vertex leaves.  GraphX's rounds, restated:
 *   state   comp[v] = v, every vertex alive, none marked, rounds = 0
 *   round   while a vertex is alive and rounds < max_iter: ++rounds, then
 *     1. write  every marked v: comp[v] = colour[v], v leaves; none marked
 *     2. trim   to the fixpoint: every alive v without an arc to an alive vertex or without an
 *               arc from one leaves, keeping comp[v] = v (a self-loop counts as both: such a
 *               vertex is never trimmed)
 *     3. only if rounds < max_iter:
 *        colour  colour[v] = the smallest alive u (v included) with a directed path u -> v
 *                inside the alive subgraph
 *        mark    every v with colour[v] == v, and every v that reaches such a root of its own
 *                colour through arcs whose ends both carry that colour: whole SCCs, each
 *                coloured by its smallest member
 * Converged (summary.unresolved == 0): comp_out[v], by dense id, is the SMALLEST dense id of
 * v's SCC, for integral ids the value GraphFrames returns.  Stopped early by max_iter, a
 * vertex whose SCC has not been written yet holds its own id; max_iter = 1 gives the identity
 * (GraphX's behaviour).  Every step is a unique fixpoint: comp_out and every summary field are
 * functions of (V, arc set, loop set, max_iter) alone, identical across runs, handles, input
 * edge orders and kernel schedules.  size_out (nullable, V entries): size_out[c] = the vertices
 * with comp_out == c, 0 at every other index.  Both arrays are host memory unless
 * out_is_device; summary is nullable.  V == 0: success, nothing written, summary
 * {0, 0, 0, -1, 0, 0, 0}.  LPA_EINVAL for max_iter <= 0 and for a null comp_out with V > 0.
 * The call blocks until the work is done.  Counter-driven peeling for the trim, a
 * label-correcting atomicMin propagation for the colours, a backward breadth-first search for
 * the marks (DESIGN.md "Strongly connected components").  All working memory is stream-ordered
 * temporaries, the labels and every other piece of lpa_step's state are neither read nor
 * written, nothing is kept on the handle.  On a distributed job (nranks > 1) only rank 0 keeps
 * the edge list this needs; the other ranks return LPA_EINVAL.  Since ABI 12.
 */
typedef struct lpa_scc_summary {
  int64_t n_components;  /* distinct values of comp_out                                  */
  int64_t n_singletons;  /* values held by exactly one vertex                            */
  int64_t largest_size;  /* 0 if V == 0                                                   */
  int64_t largest_id;    /* smallest id on a tie; -1 if V == 0                            */
  int64_t rounds;        /* rounds entered                                                */
  int64_t trimmed;       /* vertices removed by step 2, all rounds                        */
  int64_t unresolved;    /* vertices still alive at return (0 <=> converged)              */
} lpa_scc_summary;       /* 56 bytes */
int lpa_strongly_connected_components(lpa_graph* g, int32_t max_iter, int32_t* comp_out,
                                      int32_t out_is_device, int64_t* size_out /* nullable, as lpa_components */,
                                      lpa_scc_summary* summary /* nullable */);

/*
 * Louvain community detection on the symmetrised multigraph lpa_step votes on and lpa_quality
 * scores: a synchronous, deterministic Louvain (the Lu-Halappanavar-Kalyanaraman singleton rule
 * plus a monotone acceptance test), defined in exact integer arithmetic.  This is the package's
 * own call (GraphFrames has none); its labels go wherever lpa_run's go (lpa_outlier, lpa_quality).
 *
 * Graph.  Every kept input edge u -> v (both ends in [0, V)) gives the arcs u -> v and v -> u; a
 *   self-loop gives two arcs at its vertex; duplicates count.  A = total arcs.  At any level a
 *   vertex u has a self weight s[u] (arcs u -> u), off-diagonal weights w(u,v) = w(v,u) for
 *   u != v, and a degree k[u] = s[u] + sum_v w(u,v); sum k = A at every level.  Level 0:
 *   s[u] = 2 x (self-loops at u), w(u,v) = the input edges between u and v in either direction.
 * State of a level with n vertices: c[u] = u, D[c] = sum of k over the members, size[c] = the
 *   members.  The score numerator is N = A x I - sum_c D[c]^2, where
 *   I = sum_u (s[u] + sum_{v != u, c[v] = c[u]} w(u,v)).  Modularity is N / A^2.
 * A round.  All reads are of the state at the start of the round.  For every u, with own
 *   community a = c[u] and K(u,x) = sum_{v != u, c[v] = x} w(u,v):
 *     score(x) = A x K(u,x) - k[u] x (D[x] - (x == a ? k[u] : 0)).
 *     The candidates are the x != a with K(u,x) > 0; the best b has the largest score, ties to
 *     the smallest x.  u proposes a move to b iff score(b) > score(a), and not
 *     (size[a] == 1 and size[b] == 1 and b > a).  A blocked or failed best is not replaced by
 *     the second best.
 *   No proposals: the phase ends and the round is not counted.  Otherwise rounds += 1; apply all
 *   proposals; if the new N is greater than the old N, the round is accepted.  If not, apply
 *   only the proposals with b < a; if there is at least one and N rises, the round is accepted
 *   and counted in damped_rounds.  Otherwise the labels stay as they were and the phase ends.
 *   The phase also ends when its rounds == max_rounds.  N rises strictly with every accepted
 *   round, so a phase always terminates.
 * A level.  A phase with no accepted move ends the algorithm, and that level is not counted.
 *   Otherwise aggregate: the surviving community ids, in ascending order, become vertices
 *   0, 1, ... of the next level; w'(i,j) is the summed w between members of i and of j, i != j;
 *   s'(i) = sum of s over the members + sum of w(u,v) over ordered pairs u != v inside i.
 *   levels += 1; stop at max_levels.
 * Result.  comm_out[v], by dense id, is the SMALLEST original dense id in v's final community
 *   (the convention of lpa_components).  V == 0 or A == 0: the identity, 0 levels, modularity
 *   0.0.  Vertices without off-diagonal arcs never move.
 * A path or a cycle is the slow case of any synchronous min-label scheme: about n / 2 rounds in
 * the first level; max_rounds is the caller's bound.
 * Limits.  A <= 3,037,000,499, so that A^2 < 2^63: every score, N and D^2 fit int64; above
 * that the call returns LPA_EINVAL with a message.  LPA_EINVAL for max_levels <= 0, for
 * max_rounds <= 0 and for a null comm_out with V > 0.
 * comm_out and every integer of the level rows and the summary are functions of (V, the edge
 * multiset as undirected pairs, max_levels, max_rounds) alone: identical across runs, handles,
 * input edge orders and directions, and kernel schedules.  size_out (nullable, V entries):
 * size_out[c] = the vertices with comm_out == c, 0 at every other index.  Both arrays are host
 * memory unless out_is_device.  levels_out (nullable, host, levels_cap rows): row l describes
 * counted level l; the levels past levels_cap are run and summed in the summary, not written.
 * The call blocks until the work is done.  Degree-binned move kernels with LDS tally tables and
 * an exact global spill table (DESIGN.md "Louvain").  All working memory is stream-ordered
 * temporaries, the labels and every other piece of lpa_step's state are neither read nor
 * written, nothing is kept on the handle.  On a distributed job (nranks > 1) only rank 0 keeps
 * the edge list this needs; the other ranks return LPA_EINVAL.  Since ABI 14.
 */
typedef struct lpa_louvain_level {
  int64_t vertices;       /* vertices of the level                                        */
  int64_t communities;    /* communities it ends with = vertices of the next level        */
  int64_t rounds;         /* rounds with at least one proposal (a rejected last one too)  */
  int64_t damped_rounds;  /* accepted rounds that applied only the moves to a smaller id  */
  int64_t moves;          /* moves applied by the accepted rounds                         */
  int64_t numerator;      /* N at the end of the level                                    */
} lpa_louvain_level;      /* 48 bytes */
typedef struct lpa_louvain_summary {
  int64_t n_communities;  /* distinct values of comm_out                                  */
  int64_t n_singletons;   /* values held by exactly one vertex                            */
  int64_t largest_size;   /* 0 if V == 0                                                  */
  int64_t largest_id;     /* smallest id on a tie; -1 if V == 0                           */
  int64_t levels;         /* counted levels                                               */
  int64_t rounds;         /* sums over the counted levels ...                             */
  int64_t damped_rounds;
  int64_t moves;
  int64_t arcs;           /* A                                                            */
  int64_t intra_arcs;     /* I of the result                                              */
  int64_t numerator;      /* N of the result                                              */
  double modularity;      /* (double)numerator / ((double)arcs * arcs), 0.0 if arcs == 0  */
} lpa_louvain_summary;    /* 96 bytes */
int lpa_louvain(lpa_graph* g, int32_t max_levels, int32_t max_rounds, int32_t* comm_out, int32_t out_is_device,
                int64_t* size_out /* nullable, [V], where comm_out is */,
                lpa_louvain_level* levels_out /* nullable, host */, int32_t levels_cap,
                lpa_louvain_summary* summary /* nullable */);

/*
 * k-core decomposition (core numbers) of the canonical simple undirected graph of the input
 * multigraph, exactly lpa_triangle_count's: self-loops dropped, direction ignored, duplicates
 * collapsed, an edge with an end outside [0, V) is no edge.  This is the package's own call
 * (GraphFrames has none).  core_out[v], by dense id (V entries, required), is the largest k such
 * that v belongs to a subgraph in which every vertex has at least k neighbours; an isolated
 * vertex, or one with only self-loops, gets 0.  The result is unique: a pure function of
 * (V, edge set, max_k), identical across runs, edge orders, edge directions, handles, devices
 * and kernel schedules.
 * max_k >= 0 caps it (INT32_MAX: no cap): the result is min(core[v], max_k); the peeling stops
 * before level max_k and every vertex still alive gets max_k.  max_k = 0 does only the build and
 * writes zeros.  With a cap, degeneracy and main_core_size describe the CAPPED values: the
 * largest value written and the vertices that hold it.
 * simple_degree_out (nullable, V entries, int32): d(v), the distinct neighbours of v other than
 * v.  Both arrays are host memory unless out_is_device; summary is nullable.  V == 0: success,
 * nothing written, the summary all zeros.  LPA_EINVAL for a null handle, for max_k < 0 and for
 * a null core_out with V > 0.  The call blocks until the work is done.
 * Level-by-level peeling with an atomic live count per vertex: a vertex leaves at level k when
 * its count falls from k + 1 to k (DESIGN.md "k-core decomposition"); the removal queue holds
 * every vertex once, and a call whose queue tails do not sum to the vertices peeled returns
 * LPA_EOVERFLOW.  All working memory is stream-ordered temporaries, the labels and every other
 * piece of lpa_step's state are neither read nor written, nothing is kept on the handle.  On a
 * distributed job (nranks > 1) only rank 0 keeps the edge list this needs; the other ranks
 * return LPA_EINVAL.  Since ABI 16.
 */
typedef struct lpa_core_summary {
  int64_t degeneracy;      /* largest value of core_out (0 if V == 0)                         */
  int64_t main_core_size;  /* vertices with core_out == degeneracy                            */
  int64_t levels;          /* distinct values of the uncapped core among the peeled vertices,
                              + 1 if the cap left a vertex alive                               */
  int64_t simple_edges;    /* as lpa_triangle_summary                                         */
  int64_t max_degree;      /* largest simple degree                                           */
  int64_t n_core0;         /* vertices of simple degree 0                                     */
  int64_t passes;          /* host round trips of the peel: the schedule, NOT a function of
                              the graph (it depends on LPA_KC_BLOCK)                          */
} lpa_core_summary;        /* 56 bytes */
int lpa_core_numbers(lpa_graph* g, int32_t max_k /* INT32_MAX: no cap */, int32_t* core_out,
                     int32_t* simple_degree_out /* nullable */, int32_t out_is_device,
                     lpa_core_summary* summary /* nullable */);

/*
 * SCAN structural clustering (Xu, Yuruk, Feng, Schweiger: "SCAN: A Structural Clustering
 * Algorithm for Networks", KDD 2007): clusters, and the two kinds of vertex that belong to none,
 * hubs and outliers.  This is the package's own call (GraphFrames has none).  It works on the
 * canonical simple undirected graph of the input multigraph, exactly lpa_triangle_count's and
 * lpa_core_numbers': self-loops dropped, direction ignored, duplicates collapsed, an edge with an
 * end outside [0, V) is no edge.
 *   d[v]      the simple degree; c(u,v) the number of common neighbours of an edge {u,v}.  With
 *             closed neighbourhoods the structural similarity is
 *             sigma(u,v) = (c + 2) / sqrt((d[u] + 1) (d[v] + 1)).
 *   similar   an edge is similar iff, in IEEE binary64, evaluated exactly as written, every
 *             product rounded once, no fused multiply-add:
 *               (double)(c+2) * (double)(c+2) >= (eps * eps) * ((double)(d[u]+1) * (double)(d[v]+1))
 *             (sigma >= eps without the root and the division; numpy performs the same
 *             operations, so the decision is reproducible bit for bit, equality included).
 *   core      nsim[v] is the number of similar edges at v; v is a core iff nsim[v] + 1 >= mu
 *             (the vertex counts itself, as in the paper).
 *   cluster   cores are joined over similar edges whose two ends are both cores; a cluster's
 *             label is the smallest dense id among its CORES.
 *   border    a non-core with at least one similar edge to a core; it takes the SMALLEST label
 *             among those cores' clusters (the deterministic replacement for the paper's visit
 *             order).
 *   the rest  are non-members and keep label[v] = v (no collision: a cluster label is a core's
 *             id).  A non-member is a hub iff its neighbours, over all simple edges, carry at
 *             least two different cluster labels among the members; otherwise an outlier.
 *   role[v]   0 outlier, 1 hub, 2 border, 3 core.
 * label_out (int32) and role_out (uint8), V entries each, are required; nsim_out (int32, V
 * entries) is nullable.  common_out (nullable, int32, m entries: one per INPUT EDGE ROW i) is
 * c of row i's edge, or -1 where the row is a self-loop or has an end outside [0, V).  All are
 * host memory unless out_is_device; summary is nullable.  The result is a function of
 * (V, edge set, eps, mu) alone: identical across runs, edge orders, edge directions, handles,
 * devices and kernel schedules (every accumulation is an integer atomic; the only
 * floating-point work is the three products of the similarity test).
 * LPA_EINVAL for a null handle, for eps NaN or outside (0, 1], for mu < 1 and for a null
 * label_out or role_out with V > 0.  V == 0: success, nothing written, the summary all zeros
 * (largest_cluster_label -1).  The call blocks until the work is done.  All working memory is
 * stream-ordered temporaries, the labels and every other piece of lpa_step's state are neither
 * read nor written, nothing is kept on the handle.  The LPA_TC_* boundaries of
 * lpa_triangle_count choose the row forms of the common-neighbour pass.  On a distributed job
 * (nranks > 1) only rank 0 keeps the edge list this needs; the other ranks return LPA_EINVAL.
 * Since ABI 23.
 */
typedef struct lpa_scan_summary {
  int64_t simple_edges;          /* as lpa_triangle_summary                                   */
  int64_t triangles;             /* as lpa_triangle_summary.n_triangles                       */
  int64_t similar_edges;         /* simple edges that pass the test                           */
  int64_t n_clusters;
  int64_t n_cores;
  int64_t n_borders;
  int64_t n_hubs;
  int64_t n_outliers;
  int64_t largest_cluster;       /* members (cores and borders) of the largest cluster; 0 if none */
  int64_t largest_cluster_label; /* its label, the smallest among equals; -1 if none          */
} lpa_scan_summary;              /* 80 bytes */
int lpa_scan(lpa_graph* g, double eps, int32_t mu, int32_t* label_out, uint8_t* role_out,
             int32_t* nsim_out /* nullable */, int32_t* common_out /* nullable, m entries */,
             int32_t out_is_device, lpa_scan_summary* summary /* nullable */);

/*
 * Motif finding (GraphFrames GraphFrame.find(pattern)) over the DIRECTED input MULTIGRAPH.  The
 * caller has parsed the pattern into n_vars vertex variables and n_terms terms; a term is an
 * edge src_var -> dst_var, negated or not.  A result row is one assignment of vertices to the
 * vertex variables that positive terms bind, and of input edge rows to the positive terms, such
 * that every positive term's edge row goes from its src variable's vertex to its dst
 * variable's vertex, and no input edge row goes from a negated term's src vertex to its dst
 * vertex.  One row per assignment: duplicate edge rows and variables that are not in the output
 * multiply rows, variables need not be distinct (a self-loop matches a -> b with a == b), rows
 * are never deduplicated.  An edge with an end outside [0, V) is no edge; self-loops and
 * duplicates are edges.
 * The terms run in the order given.  The first term must be positive (it seeds the table with
 * every valid edge row, in edge-row order; with src_var == dst_var, the self-loops); every later
 * positive term must share a variable with the positive terms before it (an extension along the
 * out-lists or in-lists, or, with both ends bound, a close: the row times the number of
 * parallel edges); a negated term must have both variables bound by earlier positive terms.
 * var_out[v] != 0 asks for variable v's column (nullable: none), want_edge for a positive term's
 * edge-row column.  max_rows > 0 bounds EVERY table, intermediate or final: it is checked from
 * the scan's total before the table is allocated, and a step that needs more returns
 * LPA_EOVERFLOW with overflow_step / overflow_rows set in the summary (the summary is written
 * on that path too) and nothing allocated left behind; max_rows <= 0: no cap.  count_only != 0
 * runs every step but never fills the last table: rows is exact, result_out must be null.
 * Otherwise *result_out receives a result object that owns the final table (one plain device
 * allocation on the handle's device, which the last fill wrote) and nothing of the handle: it
 * stays valid after later calls and after lpa_graph_destroy, until lpa_motif_result_destroy.
 * lpa_motif_vertex_column / lpa_motif_edge_column copy a column to the host (dense vertex ids,
 * int32; input edge rows, int64; `rows` entries) and return LPA_EINVAL for a column that was
 * not asked for.  V == 0 or m == 0: success, zero rows, a valid empty result.
 * LPA_EINVAL for a null handle, n_vars outside [1, 32], n_terms outside [1, 16] or more than 8
 * positive or 8 negated terms, a variable index out of range, a negated first term, a positive
 * term that shares no variable with the earlier positive ones, a negated term with an unbound
 * variable, var_out naming a variable no positive term binds, result_out null without
 * count_only or the reverse.  LPA_ENOMEM when a table cannot be allocated (the temporaries are
 * released).  The call blocks until the work is done; one host synchronisation per term.
 * Every step is counts, an int64 exclusive scan and a fill that writes the children of a row in
 * list order and the rows in their order (DESIGN.md "Motif finding"): the final table, row for
 * row, and every summary field are a function of (V, edge list, terms) alone, identical across
 * runs and handles.  table_rows[t] is the table after term t; a table without rows ends the
 * call (steps = the terms run so far, the later entries 0).  All working memory is
 * stream-ordered temporaries, the labels and every other piece of lpa_step's state are neither
 * read nor written, nothing is kept on the handle.  On a distributed job (nranks > 1) only rank
 * 0 keeps the edge list this needs; the other ranks return LPA_EINVAL.  Since ABI 19.
 */
typedef struct lpa_motif_term {
  int32_t src_var, dst_var, negated, want_edge;
} lpa_motif_term;
typedef struct lpa_motif_summary {
  int64_t rows;            /* rows of the final table                                         */
  int64_t edges;           /* valid input edge rows                                           */
  int64_t self_loops;      /* self-loops among them                                           */
  int64_t steps;           /* terms executed                                                  */
  int64_t peak_rows;       /* largest table of the call                                       */
  int64_t overflow_step;   /* term index that exceeded max_rows, else -1                      */
  int64_t overflow_rows;   /* rows that step needed                                           */
  int64_t table_rows[16];  /* rows after each term, in execution order                        */
} lpa_motif_summary;       /* 184 bytes */
typedef struct lpa_motif_result lpa_motif_result;
int lpa_motif(lpa_graph* g, int32_t n_vars, const uint8_t* var_out /* [n_vars], nullable */,
              const lpa_motif_term* terms, int32_t n_terms, int64_t max_rows,
              int32_t count_only, lpa_motif_result** result_out /* null iff count_only */,
              lpa_motif_summary* summary /* nullable */);
int64_t lpa_motif_rows(const lpa_motif_result* r);
int lpa_motif_vertex_column(const lpa_motif_result* r, int32_t var, int32_t* out /* host [rows] */);
int lpa_motif_edge_column(const lpa_motif_result* r, int32_t term, int64_t* out /* host [rows] */);
void lpa_motif_result_destroy(lpa_motif_result* r);   /* null: no-op */

/*
 * Message aggregation (GraphFrames GraphFrame.aggregateMessages) over the DIRECTED input
 * MULTIGRAPH.  Every kept edge row src -> dst evaluates a message program: to_dst's value goes
 * to dst, to_src's to src (either may be null, not both).  Every vertex reduces the messages it
 * receives to their count, sum, min and max, in IEEE binary64.  Duplicates are edges of their own
 * (they send again), a self-loop with both programs delivers both messages to its vertex, an edge
 * with an end outside [0, V) is no edge.
 * A program is postfix code over an operand stack of at most LPA_AM_MAX_STACK values: op word =
 * opcode | argument << 16.  CONST k pushes consts[k]; SRC c / DST c push vcols[c][src] /
 * vcols[c][dst]; EDGE c pushes ecols[c][edge row]; ADD SUB MUL DIV, the comparisons EQ NE LT LE GT
 * GE (1.0 or 0.0) and AND OR (operands != 0.0 are true) pop b, then a, and push a op b; NEG ABS NOT
 * replace the top; WHEN pops value, then condition, and pushes the value where the condition is
 * true; WHEN_ELSE pops otherwise, value, condition.  A value may be null: an operator with a null
 * operand gives null (AND and OR too: no three-valued logic), x / 0 gives null, a WHEN whose
 * condition is false or null gives null, a WHEN_ELSE whose condition is false or null gives its
 * otherwise operand.  Both branches of a conditional are evaluated.  A null message is not
 * delivered.  The program must leave exactly one value.
 * vcols: host [n_vcols][V]; ecols: host [n_ecols][m], in the handle's input edge order.  The
 * outputs are host arrays of V entries, each nullable (only the wanted ones are written):
 * count_out (0 for a vertex that received nothing), sum_out (0.0 there), min_out and max_out (NaN
 * there).  summary (nullable) holds integers only: nulls = the messages evaluated and not
 * delivered; receivers = vertices with count > 0; rows_* = the vertices by kernel form; max_row =
 * the longest message list (in-degree if to_dst, plus out-degree if to_src).
 * LPA_EINVAL, with a lpa_last_error() text, for both programs null; a malformed program (n_ops
 * outside [1, LPA_AM_MAX_OPS], n_consts outside [0, LPA_AM_MAX_CONSTS], an unknown opcode, a
 * constant or column index out of range, stack underflow, a stack deeper than LPA_AM_MAX_STACK,
 * an end depth other than 1); a null handle; n_vcols or n_ecols outside [0, LPA_AM_MAX_COLUMNS];
 * a null column pointer when a column is read.  The programs are validated on the host, before
 * the handle is looked at and before anything is launched; the kernels trust them.  V == 0 or no
 * valid edge: success, the outputs at their empty values.
 * A vertex's message list is its in-list rows, sorted by (src, edge row), then its out-list rows,
 * sorted by (dst, edge row).  Rows of up to LPA_AM_SHORT entries (default 32) take 8 lanes each,
 * up to LPA_AM_WAVE (default 1024) a wave, longer ones a block of 1024 (both read at create time;
 * 0, or LPA_AM_WAVE <= LPA_AM_SHORT: no row takes that form, except that an empty row is always a
 * short one).  Every lane accumulates its strided share in list order, then an xor-shuffle tree,
 * then, in the block form, the wave partials in order; no floating-point atomics, no fused
 * multiply-adds (DESIGN.md "Message aggregation").  Hence count, min, max and every summary
 * integer except rows_* are a function of the inputs alone (min prefers -0.0 to +0.0, max the
 * reverse); sum is bit-identical across calls and handles with the same boundaries, and across
 * input edge orders whenever parallel edges carry equal messages (any program that reads no edge
 * column).  With finite columns a NaN message can only come from overflow; min and max are then
 * unspecified.  All working memory is stream-ordered temporaries, the labels and every other
 * piece of lpa_step's state are neither read nor written, nothing is kept on the handle.  On a
 * distributed job (nranks > 1) only rank 0 keeps the edge list this needs; the other ranks return
 * LPA_EINVAL.  Since ABI 20.
 */
#define LPA_AM_MAX_OPS 64
#define LPA_AM_MAX_STACK 8
#define LPA_AM_MAX_CONSTS 16
#define LPA_AM_MAX_COLUMNS 8   /* vertex columns, and edge columns, of one call */
enum {
  LPA_AM_CONST = 0, LPA_AM_SRC = 1, LPA_AM_DST = 2, LPA_AM_EDGE = 3,
  LPA_AM_ADD = 4, LPA_AM_SUB = 5, LPA_AM_MUL = 6, LPA_AM_DIV = 7,
  LPA_AM_NEG = 8, LPA_AM_ABS = 9,
  LPA_AM_EQ = 10, LPA_AM_NE = 11, LPA_AM_LT = 12, LPA_AM_LE = 13, LPA_AM_GT = 14, LPA_AM_GE = 15,
  LPA_AM_AND = 16, LPA_AM_OR = 17, LPA_AM_NOT = 18,
  LPA_AM_WHEN = 19, LPA_AM_WHEN_ELSE = 20,
  LPA_AM_NOPS = 21
};
typedef struct lpa_am_program {
  int32_t n_ops, n_consts;
  uint32_t ops[LPA_AM_MAX_OPS];       /* opcode | argument << 16                               */
  double consts[LPA_AM_MAX_CONSTS];
} lpa_am_program;          /* 392 bytes */
typedef struct lpa_am_summary {
  int64_t edges;             /* valid input edge rows                                         */
  int64_t messages_to_src;   /* delivered (non-null) messages, by direction                   */
  int64_t messages_to_dst;
  int64_t nulls;             /* evaluated and not delivered                                   */
  int64_t receivers;         /* vertices with count > 0                                       */
  int64_t rows_short, rows_wave, rows_block;   /* vertices by kernel form                     */
  int64_t max_row;           /* the longest message list                                      */
} lpa_am_summary;          /* 72 bytes */
int lpa_aggregate_messages(lpa_graph* g, const lpa_am_program* to_src /* nullable */,
                           const lpa_am_program* to_dst /* nullable */,
                           const double* vcols /* host [n_vcols][V] */, int32_t n_vcols,
                           const double* ecols /* host [n_ecols][m] */, int32_t n_ecols,
                           int64_t* count_out /* host [V], nullable */, double* sum_out /* nullable */,
                           double* min_out /* nullable */, double* max_out /* nullable */,
                           lpa_am_summary* summary /* nullable */);

/*
 * Pregel (graphframes.lib.Pregel.run of GraphFrames 0.8) over the DIRECTED input MULTIGRAPH:
 * vertex columns that live across max_iter iterations on the device, messages along the edges,
 * one aggregate, one update program per column.  Duplicates are edges of their own, a self-loop
 * is an edge, an edge with an end outside [0, V) is no edge.  IEEE binary64, no fused
 * multiply-adds; the null rules are those of lpa_aggregate_messages (AND and OR with a null
 * operand give null).
 * Columns.  The n_vcols static columns (vcols, host [n_vcols][V]) have the indices [0, n_vcols),
 * the n_pcols Pregel columns (1 to LPA_PG_MAX_COLUMNS) the indices n_vcols + j; together at most
 * LPA_AM_MAX_COLUMNS.  ecols: host [n_ecols][m], in the handle's input edge order.
 * Start.  Pregel column j = init[j] per vertex.  An init program reads static columns and
 * constants only.
 * One iteration, max_iter times, no early stop; every read is of the state before the iteration
 * and all Pregel columns change at once (a' = b, b' = a swaps):
 *   1. every kept edge row s -> d evaluates the n_to_dst programs to_dst[] for d and the n_to_src
 *      programs to_src[] for s (0 to LPA_PG_MAX_MESSAGES each, at least one in all): message
 *      programs as lpa_aggregate_messages takes them, SRC c / DST c reading column c, static or
 *      Pregel, of that end.  A null message is not delivered;
 *   2. every vertex aggregates what was delivered to it with agg: LPA_PG_SUM, MIN, MAX, AVG (sum /
 *      count, on the device) or COUNT.  That is msg; it is NULL for a vertex that received
 *      nothing, for COUNT too;
 *   3. Pregel column j becomes update[j] over the vertex's own columns (old values) and msg.
 * init[] and update[] are vertex programs: postfix code with the stack discipline and the limits
 * of a message program and opcodes of their own (LPA_VP_*).  CONST k pushes consts[k], COL c
 * column c of this vertex, MSG the aggregate; the arithmetic, comparison, logic and conditional
 * ops are those of the message programs; COALESCE pops b, then a, and pushes a where a is not
 * null, else b; ISNULL replaces the top by 1.0 where it is null, else 0.0, and is never null.
 * A null value of an init or update program is an error: the kernels record the smallest
 * (iteration, column, vertex) -- iteration 0 is the start -- in one 64-bit atomic minimum, store
 * NaN and go on; the call looks once, at its end, returns LPA_EINVAL with a lpa_last_error() text
 * that names the iteration, the Pregel column and the dense id, and writes nothing to cols_out
 * (summary then holds the three in null_iteration, null_column, null_vertex and nothing else of
 * meaning; they are -1 after a success).
 * cols_out: host [n_pcols][V], the columns after max_iter iterations.  summary (nullable) holds
 * integers only, the message counts summed over the iterations: nulls = evaluated and not
 * delivered; rows_* = the vertices by kernel form; max_row = the longest message list in rows.
 * LPA_EINVAL, with a lpa_last_error() text naming the program, for a malformed program (as for
 * lpa_aggregate_messages; also an init program that reads a Pregel column or MSG), max_iter <= 0,
 * an unknown agg, n_pcols outside [1, LPA_PG_MAX_COLUMNS], n_to_src or n_to_dst outside
 * [0, LPA_PG_MAX_MESSAGES] or both 0, n_vcols < 0 or n_vcols + n_pcols > LPA_AM_MAX_COLUMNS,
 * n_ecols outside [0, LPA_AM_MAX_COLUMNS], a null pointer where something is read or written; all
 * of it is checked on the host before the handle is looked at, and the kernels trust it.  Then a
 * null handle.  V == 0: success, nothing written.  No kept edge: the iterations run, every msg is
 * null.  LPA_EINVAL also where one direction's programs times m exceed 2^32 - 1: a vertex counts
 * the messages of a direction in 32 bits.
 * A vertex's message list is its in-list rows, sorted by (src, edge row), then its out-list rows,
 * sorted by (dst, edge row); the entries are ROWS: a lane takes its strided share of rows in list
 * order and, within a row, that direction's programs in the order given; then the xor-shuffle
 * tree, then, in the block form, the 16 wave partials in order.  The row forms and their
 * boundaries are those of lpa_aggregate_messages (LPA_AM_SHORT, LPA_AM_WAVE), by rows.  One fused
 * launch per row form and iteration reduces a vertex's messages and applies its update programs:
 * no per-edge message array, no per-vertex aggregate array, no host synchronisation between the
 * iterations, no floating-point atomics (DESIGN.md "Pregel").  Hence with MIN, MAX or COUNT every
 * column is a function of the inputs alone; with SUM or AVG the columns are bit-identical across
 * calls and handles with the same boundaries, and across input edge orders for programs that read
 * no edge column; with one program per direction, iteration 1's aggregate has the bits
 * lpa_aggregate_messages returns for those programs over the initial columns.  The labels and
 * every other piece of lpa_step's state are neither read nor written, nothing is kept on the
 * handle.  On a distributed job only rank 0 keeps the edge list; the other ranks return
 * LPA_EINVAL.  Since ABI 21.
 */
#define LPA_PG_MAX_COLUMNS 4    /* Pregel columns of one call          */
#define LPA_PG_MAX_MESSAGES 4   /* message programs of one direction   */
enum { LPA_PG_SUM = 0, LPA_PG_MIN = 1, LPA_PG_MAX = 2, LPA_PG_AVG = 3, LPA_PG_COUNT = 4, LPA_PG_NAGGS = 5 };
enum {
  LPA_VP_CONST = 0, LPA_VP_COL = 1, LPA_VP_MSG = 2,
  LPA_VP_ADD = 3, LPA_VP_SUB = 4, LPA_VP_MUL = 5, LPA_VP_DIV = 6,
  LPA_VP_NEG = 7, LPA_VP_ABS = 8,
  LPA_VP_EQ = 9, LPA_VP_NE = 10, LPA_VP_LT = 11, LPA_VP_LE = 12, LPA_VP_GT = 13, LPA_VP_GE = 14,
  LPA_VP_AND = 15, LPA_VP_OR = 16, LPA_VP_NOT = 17,
  LPA_VP_WHEN = 18, LPA_VP_WHEN_ELSE = 19,
  LPA_VP_COALESCE = 20, LPA_VP_ISNULL = 21,
  LPA_VP_NOPS = 22
};
typedef struct lpa_vp_program {
  int32_t n_ops, n_consts;
  uint32_t ops[LPA_AM_MAX_OPS];       /* opcode | argument << 16                               */
  double consts[LPA_AM_MAX_CONSTS];
} lpa_vp_program;          /* 392 bytes */
typedef struct lpa_pregel_summary {
  int64_t edges;             /* valid input edge rows                                         */
  int64_t messages_to_src;   /* delivered (non-null) messages, by direction, all iterations   */
  int64_t messages_to_dst;
  int64_t nulls;             /* evaluated and not delivered, all iterations                   */
  int64_t rows_short, rows_wave, rows_block;   /* vertices by kernel form                     */
  int64_t max_row;           /* the longest message list, in rows                             */
  int64_t iterations;        /* iterations run                                                */
  int64_t null_iteration, null_column, null_vertex;   /* the first null value, or -1          */
} lpa_pregel_summary;      /* 96 bytes */
int lpa_pregel(lpa_graph* g, int32_t max_iter, int32_t agg,
               const lpa_am_program* to_src /* [n_to_src] */, int32_t n_to_src,
               const lpa_am_program* to_dst /* [n_to_dst] */, int32_t n_to_dst,
               const lpa_vp_program* init /* [n_pcols] */, const lpa_vp_program* update /* [n_pcols] */,
               int32_t n_pcols,
               const double* vcols /* host [n_vcols][V] */, int32_t n_vcols,
               const double* ecols /* host [n_ecols][m] */, int32_t n_ecols,
               double* cols_out /* host [n_pcols][V] */, lpa_pregel_summary* summary /* nullable */);

/* Symmetrised degree of every vertex (dense ids), host output. */
int lpa_degrees(lpa_graph* g, int32_t* deg_out);

/* lpa_graph_info has grown across header versions (it carries no size field of its
 * own; fields are only ever appended).  lpa_graph_get_info is frozen at the ABI-5
 * struct: it writes the fields up to blocked_pieces, never more, so a caller built
 * against that header is not overrun.  lpa_graph_get_info_sized(g, info, sizeof *info)
 * writes min(info_size, sizeof) bytes of this header's struct and zeroes the rest of a
 * larger caller struct: use it for the later fields.  lpa_abi_version() returns the
 * library's LPA_ABI_VERSION, so a binding can check the header it was built for.
 * ABI 7: lpa_graph_create_hostcoll, host_allgathers, the frozen unsized get_info.
 * ABI 8: lpa_components.
 * ABI 9: lpa_triangle_count.
 * ABI 10: lpa_pagerank.
 * ABI 11: lpa_shortest_paths.
 * ABI 12: lpa_strongly_connected_components.
 * ABI 13: lpa_parallel_pagerank.
 * ABI 14: lpa_louvain.
 * ABI 15: sparse_refreshes.
 * ABI 16: lpa_core_numbers.
 * ABI 17: fill_refreshes.
 * ABI 18: lpa_bfs.
 * ABI 19: lpa_motif, lpa_motif_rows, lpa_motif_vertex_column, lpa_motif_edge_column,
 *         lpa_motif_result_destroy.
 * ABI 20: lpa_aggregate_messages.
 * ABI 21: lpa_pregel.
 * ABI 22: lpa_betweenness.
 * ABI 23: lpa_scan. */
#define LPA_ABI_VERSION 23
int lpa_abi_version(void);
int lpa_graph_get_info(const lpa_graph* g, lpa_graph_info* info);
int lpa_graph_get_info_sized(const lpa_graph* g, lpa_graph_info* info, int64_t info_size);
void lpa_graph_destroy(lpa_graph* g);
const char* lpa_last_error(void);

/* ---- synthetic inputs; device outputs, caller-allocated ---- */
/* R-MAT, Graph500 A/B/C/D = .57/.19/.19/.05, m edges over 2^scale vertices,
 * duplicates and self-loops kept, optional seeded bijective id scramble. */
int lpa_gen_rmat(int32_t scale, int64_t m, uint64_t seed, int32_t scramble, int32_t* d_src,
                 int32_t* d_dst, int32_t device, void* hip_stream);
/* planted-partition SBM: V vertices in `blocks` equal blocks, p_in as a Q32 fraction. */
int lpa_gen_sbm(int32_t V, int32_t blocks, int64_t m, uint32_t p_in_q32, uint64_t seed,
                int32_t* d_src, int32_t* d_dst, int32_t device, void* hip_stream);
/* Chung-Lu power-law (config C5: "Twitter-shaped", heavy hubs): both endpoints drawn
 * with P(i) ~ (i + i0)^(-1/(gamma-1)), i0 chosen so the expected maximum degree is
 * max_deg (<= 0: i0 = 1), ranks mapped to ids by a seeded affine permutation mod V;
 * duplicates and self-loops kept.  Builds a (V+1) x 8 B weight table on the host. */
int lpa_gen_chunglu(int32_t V, int64_t m, double gamma, double max_deg, uint64_t seed,
                    int32_t* d_src, int32_t* d_dst, int32_t device, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LPA_H_ */
