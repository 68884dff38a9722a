"""MI355X-native label propagation + outlier scoring (drop-in for the
GraphFrames ``labelPropagation`` path of
/root/reference/CommunityDetection/Graphframes.py).

Importable as ``graphframes_amd`` (see the shim at the repository root).  The
compute runs in liblpa_hip.so (hand-written HIP for gfx950, C ABI in
include/lpa.h); importing this package does not load it -- the first call does,
and fails loudly if it has not been built.
"""
from .graph import Graph, Loopback, PregelNullError, comm_unique_id, gen_chunglu, gen_rmat, gen_sbm, run_ranks
from .graphframe import (AggregateMessages, CompiledMessage, CompiledVertexProgram, GraphFrame, IndexedGraph,
                         MessageAggregate, MessageExpr,
                         MotifTerm, OutlierResult, ParsedMotif, Pregel, aggregate_messages, betweenness_centrality, bfs,
                         compile_message,
                         compile_vertex_program,
                         connected_components, core_number, count_paths, enumerate_paths, find, index_graph,
                         k_core, label_propagation, louvain, motif_count, outlier_scores, page_rank,
                         parallel_personalized_page_rank, parse_motif, plan_motif, scan, shortest_paths,
                         strongly_connected_components, structural_similarity, triangle_count)
from . import ingest

__all__ = ["Graph", "Loopback", "run_ranks", "GraphFrame", "IndexedGraph", "OutlierResult", "comm_unique_id", "gen_chunglu", "gen_rmat",
           "gen_sbm", "betweenness_centrality", "bfs", "connected_components", "core_number", "count_paths", "enumerate_paths", "index_graph", "ingest", "k_core",
           "label_propagation", "louvain",
           "outlier_scores", "page_rank", "parallel_personalized_page_rank", "shortest_paths", "strongly_connected_components",
           "triangle_count", "find", "motif_count", "parse_motif", "plan_motif", "MotifTerm", "ParsedMotif",
           "AggregateMessages", "aggregate_messages", "compile_message", "CompiledMessage", "MessageExpr", "MessageAggregate",
           "Pregel", "PregelNullError", "compile_vertex_program", "CompiledVertexProgram", "scan",
           "structural_similarity"]
