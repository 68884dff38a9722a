// The phases of the superstep schedule: every test of lpa_graph::since_reset (supersteps
// run since the labels were last L0) that launch_tally, launch_refresh, run_supersteps,
// the hub combine and the exchange branch on, by name.  Superstep k runs while
// since_reset == k - 1.
//
//   superstep  what is special about it
//   1          from L0: column runs instead of hash tallies (first_runs_now); label-dense
//              (block mode, dense refresh, forked hub combine); its refresh may take the
//              giant codes; gather mode starts here
//   2          label-dense too; the giant word G is offered to the tallies from here on;
//              in block mode the hub rows are decided by giant counts first; settles from
//              the giant codes when the refresh of superstep 1 took them (code_tally_now);
//              its refresh may take them as well; captured per (superstep, cur, par)
//   3          rows settled from the arc giant bits of superstep 2's rebuild (settle3_now)
//              or from the giant codes of superstep 2's refresh (code_tally3_now); its
//              scatter keeps the arc giant bits (keep_bits_now), or its refresh takes the
//              fill-scatter form and leaves exact ones (fill_step3_now); captured like superstep 2
//   4          rows below the hubs settled from a fresh abits pass while every hub unit
//              is re-tallied (settle4_now); the last one that is offered G, that queues
//              the units last and whose row bins peel once; launched eagerly
//   5+         converged (converged_now): frontier lists, fused bins, captured graphs per
//              (cur, par); gather mode ends after superstep kGatherSteps
#pragma once

#include "lpa_internal.h"

namespace lpa {

// Gather mode (lpa_build: small label vector, no row above 128 arcs -- C2) for the first
// kGatherSteps supersteps: their tallies read L[col[i]] (arc_vote), no al[] is written
// (the scatter only marks the frontier), and the last of them rebuilds al once, for the
// later supersteps, whose cheaper tallies beat the gathers (C2, same box: label-dense
// supersteps 0.42-0.49 -> 0.34-0.37 ms gathering, converged ones 0.16-0.22 ms from al[]
// against 0.25-0.30 gathering; LPA_GATHER_STEPS=99, every superstep gathering, re-measured:
// supersteps 2-10 2.84 against 2.65 ms)
#ifndef LPA_GATHER_STEPS
#define LPA_GATHER_STEPS 6
#endif
constexpr int kGatherSteps = LPA_GATHER_STEPS;
inline bool gather_now(const lpa_graph* g) { return g->gather && g->since_reset < kGatherSteps; }
// the last gather-mode superstep, when the handle is in gather mode (its refresh rebuilds al)
inline bool gather_last_step(const lpa_graph* g) { return g->since_reset == kGatherSteps - 1; }

// no superstep ran since L0
inline bool at_l0(const lpa_graph* g) { return g->since_reset == 0; }

// superstep 1 from L0 by column runs (k_first_runs); the caller's refresh diffs
inline bool first_runs_now(const lpa_graph* g) {
  return g->first_runs && g->cols_sorted && g->first_best && g->rstart && g->since_reset == 0 && g->arcs > 0 &&
         !g->serial;
}

// the label-dense supersteps (1 and 2): few peel rounds, no row-bin peel, forked hub combine
// (the same test as dense_refresh below, kept apart: change one, look at the other)
inline bool label_dense_now(const lpa_graph* g) { return g->since_reset < kDenseSupersteps; }
// the label-dense supersteps tally the rows [hub_lane_begin, n_hub) with k_lpa_block
// and skip their units; the superstep after them tallies every row (their units'
// staged words are stale)
inline bool block_mode_now(const lpa_graph* g) { return g->since_reset < kDenseSupersteps && g->hub_lane_begin < g->n_hub; }
inline bool last_block_mode_now(const lpa_graph* g) {
  return block_mode_now(g) && g->since_reset + 1 == kDenseSupersteps;
}
inline int64_t block_rows_begin(const lpa_graph* g) { return g->hub_block2_begin; }  // first row of the block tiers
// label-dense superstep: its diff only counts the changed slots, and its refresh
// rebuilds al[] unless few changed (k_dense_decide).  P > 1: the count runs after the
// exchange over the whole replicated vector (launch_refresh), P = 1 per stream inside
// the tally
inline bool dense_refresh(const lpa_graph* g) { return g->since_reset < kDenseSupersteps; }

// the refresh after superstep 1 or 2 may take the giant codes (after superstep 1 on
// R-MAT, after superstep 2 on Chung-Lu: the first label vector whose giant carries the
// hubs without holding half the hot slots).  Round 6: on every rank of a partitioned job
// too -- the refresh follows the exchange, so it codes the replicated vector, and G (picked
// from it) is the same on every rank; each rank codes and settles its own rows
inline bool code_refresh_now(const lpa_graph* g) { return g->code_ok && g->since_reset <= 1; }
// ... and superstep 2 (block mode) or 3 then settles from them
inline bool code_tally_now(const lpa_graph* g) { return g->code_ok && g->since_reset == 1; }
inline bool code_tally3_now(const lpa_graph* g) { return g->code_ok && g->since_reset == 2 && g->code3; }
// before superstep 3 on a code-capable handle the host reads whether the refresh after
// superstep 2 took the giant codes (lpa_graph::code3)
inline bool code3_read_now(const lpa_graph* g) { return g->code_ok && g->since_reset == 2; }

// supersteps 2-4 (the label-dense ones after the column-run superstep 1): the giant word
// is offered to the tallies (giant_decide)
inline bool giant_offered_now(const lpa_graph* g) { return g->since_reset >= 1 && g->since_reset <= 3; }
// superstep 3 with arc giant bits: its rows may settle from them (k_settle_*)
inline bool settle3_now(const lpa_graph* g) { return g->since_reset == 2 && g->abits; }
// superstep 4: the settle of the rows below the hubs (its abits come from al)
inline bool settle4_now(const lpa_graph* g) { return g->since_reset == 3 && g->abits != nullptr && !gather_now(g); }
// supersteps 2-4 of the concurrent schedule queue the main stream's unit work after the bins
inline bool units_last_now(const lpa_graph* g) { return !g->serial && g->since_reset >= 1 && g->since_reset <= 3; }
// supersteps up to 4: the row bins peel at most once before a chunk is hashed
inline bool rows_peel_once_now(const lpa_graph* g) { return g->since_reset <= 3; }
// superstep 3's refresh keeps the arc giant bits of superstep 2's bits-mode rebuild
// (k_al_scatter; superstep 4's row settle reads them)
inline bool keep_bits_now(const lpa_graph* g) {
  return g->since_reset == 2 && g->abits != nullptr && g->gbits != nullptr && !gather_now(g) && g->keep_bits;
}
// superstep 3's refresh may take the fill-scatter form in place of its scatter (one GPU, sparse
// al[], outside gather mode, LPA_FILL_STEP3; the decision itself is taken on the device).  The
// form writes no frontier marks and syncs no label: superstep 4 tallies or settles every row
// (settle3_now sets force_all_next whenever abits exists, whatever the other switches)
inline bool fill_step3_now(const lpa_graph* g) {
  return g->since_reset == 2 && g->sparse_al && g->fill_scatter != 0 && g->fill_step3 != 0 && g->nranks == 1 &&
         !g->gather && !g->no_scatter && g->rebuild_hot && g->cptr && g->cpos && g->abits && g->gbits &&
         g->gbits_next && g->fill_part;
}

// from superstep kDenseSupersteps + 3 on a superstep is converged: frontier lists, captured
// graphs per (cur, par); the supersteps before it are launched stream-ordered or from the
// early graphs (their schedule differs from the one a converged graph bakes)
inline bool converged_now(const lpa_graph* g) { return g->since_reset >= kDenseSupersteps + 2; }
// the converged supersteps' bins as one k_bins_fused launch per stream (launch_tally)
inline bool fused_now(const lpa_graph* g) {
  return g->fused_bins && g->frontier && converged_now(g) && !gather_now(g);
}
// supersteps 2 and 3 have captured graphs of their own (not 4: its settle chain on aux0
// stops overlapping the hub units inside a graph, 0.67 -> 0.75 ms at C3) ...
inline bool early_graph_window(const lpa_graph* g) { return g->since_reset >= 1 && g->since_reset <= 2; }
// ... numbered 0 and 1 in the graph keys
inline int early_graph_index(const lpa_graph* g) { return (int)(g->since_reset - 1); }

// the vote source of a tally launch: p = g->al (or the column array in gather mode, whose
// refreshes never leave al[] sparse)
inline ArcSrc arc_src(const lpa_graph* g, const int32_t* p) {
  ArcSrc a;
  a.p = p;
  a.bits = reinterpret_cast<const uint32_t*>(g->abits);
  a.gword = g->gword;
  a.last = (uint32_t)(2 * ((g->arcs + 63) / 64 + 1) - 1);
  return a;
}
inline ArcSrc arc_src(const lpa_graph* g) { return arc_src(g, g->al); }

}  // namespace lpa
