"""Parallel personalized PageRank, the part that needs no GPU: the C-ABI boundary of
lpa_parallel_pagerank, the exported names, the argument checks of
GraphFrame.parallelPersonalizedPageRank (they run before any device work), and the all-columns
reference of tests/ppr_ref.py checked per column against the per-source pr_ref.pagerank within
pr_ref.bound and against closed forms."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import ppr_ref
import pr_ref
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph
from ppr_ref import degree_mix_sources, tournament_sources

KS = (1, 5, 20)


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_parallel_pagerank(None, 5, 0.15, None, 0, None, 0, None, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_parallel_pagerank():
    assert _lib.load().lpa_abi_version() >= 13


def test_summary_struct_layout():
    s = _lib.LpaPprSummary(1, 2, 3, 4, 5, 6, 0.5, 1.5)
    assert s.to_dict() == dict(edges=1, sinks=2, max_in_degree=3, batches=4, batch_width=5, nonzero=6,
                               rank_sum_min=0.5, rank_sum_max=1.5)
    assert list(s.to_dict()) == ["edges", "sinks", "max_in_degree", "batches", "batch_width", "nonzero",
                                 "rank_sum_min", "rank_sum_max"]
    assert ctypes.sizeof(_lib.LpaPprSummary) == 64


def test_names_exported():
    assert "parallel_personalized_page_rank" in gfa.__all__
    assert callable(gfa.parallel_personalized_page_rank)
    assert callable(gfa.GraphFrame.parallelPersonalizedPageRank) and callable(gfa.Graph.parallel_pagerank)
    assert "lpa_parallel_pagerank" in _lib.SIGNATURES


# ---- argument checks: none of them reaches the device ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": np.array([30, 10, 20], np.int64)})
    e = pd.DataFrame({"src": np.array([10, 20], np.int64), "dst": np.array([20, 30], np.int64)})
    f = gfa.GraphFrame(v, e)
    yield f
    assert f._graph is None   # no handle was ever built


@pytest.mark.parametrize("ids", [None, [], (), np.empty(0, np.int64)])
def test_source_ids_required(gf, ids):
    with pytest.raises(ValueError, match="sourceIds"):
        gf.parallelPersonalizedPageRank(sourceIds=ids, maxIter=5)
    with pytest.raises(ValueError, match="sourceIds"):
        gfa.parallel_personalized_page_rank(gf.vertices, gf.edges, ids, 5)


def test_source_ids_default_is_missing(gf):
    with pytest.raises(ValueError, match="sourceIds"):
        gf.parallelPersonalizedPageRank(maxIter=5)


def test_max_iter_required(gf):
    with pytest.raises(ValueError, match="maxIter"):
        gf.parallelPersonalizedPageRank(sourceIds=[10])
    with pytest.raises(ValueError, match="maxIter"):
        gfa.parallel_personalized_page_rank(gf.vertices, gf.edges, [10], None)


@pytest.mark.parametrize("n", [0, -3])
def test_max_iter_positive(gf, n):
    with pytest.raises(ValueError, match=rf"^requirement failed: Number of iterations must be greater than 0, but got {n}$"):
        gf.parallelPersonalizedPageRank(sourceIds=[10], maxIter=n)


@pytest.mark.parametrize("bad", [2.0, "5", True])
def test_max_iter_type(gf, bad):
    with pytest.raises(TypeError, match="maxIter"):
        gf.parallelPersonalizedPageRank(sourceIds=[10], maxIter=bad)


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan")])
def test_reset_probability_range(gf, p):
    with pytest.raises(ValueError, match=r"^requirement failed: Random reset probability must belong to \[0, 1\], but got "):
        gf.parallelPersonalizedPageRank(resetProbability=p, sourceIds=[10], maxIter=5)


@pytest.mark.parametrize("ids", [10, "10", {10, 20}, np.array([[10, 20]]), iter([10])])
def test_source_ids_type(gf, ids):
    with pytest.raises(TypeError, match="sourceIds"):
        gf.parallelPersonalizedPageRank(sourceIds=ids, maxIter=5)


@pytest.mark.parametrize("sid", [99, 15, "10", None])
def test_source_id_must_be_a_vertex(gf, sid):
    with pytest.raises(ValueError, match="sourceIds") as ei:
        gf.parallelPersonalizedPageRank(sourceIds=[10, sid, 20], maxIter=5)
    assert repr(sid) in str(ei.value)


def test_graph_method_argument_types():
    with pytest.raises(TypeError, match="max_iter"):
        gfa.Graph.parallel_pagerank(None, [0], 2.5)
    with pytest.raises(TypeError, match="source"):
        gfa.Graph.parallel_pagerank(None, [0, "a"], 2)
    with pytest.raises(TypeError, match="source"):
        gfa.Graph.parallel_pagerank(None, [True], 2)


# ---- the two references, column by column ----
def _both(V, s, d, sources, k, a=0.15):
    R, S = ppr_ref.parallel(V, s, d, sources, k, a)
    assert R.dtype == np.float64 and R.shape == (len(sources), V) and S.shape == (len(sources),)
    _, indeg = pr_ref.degrees(V, s, d)
    b = pr_ref.bound(k, int(indeg.max()) if V else 0, V)
    worst = 0.0
    for l, x in enumerate(sources):
        r1, _, _, S1 = pr_ref.pagerank(V, s, d, k, a, int(x))
        err = np.abs(R[l] - r1)
        worst = max(worst, float(np.max(err / np.where(r1 > 0, r1, 1.0))))
        assert (err <= b * r1).all(), (l, x, worst, b)
        assert np.array_equal(R[l] == 0.0, r1 == 0.0)
        assert abs(S[l] - S1) <= b * S1
        assert abs(float(R[l].sum()) - 1.0) <= V * 2.0 ** -52
    print(f"V={V} k={k} n={len(sources)} bound={b:.3e} worst relative difference={worst:.3e}")
    return R, S


@pytest.mark.parametrize("k", KS)
def test_references_agree_on_tournament(k):
    n = 1026
    s, d = np.triu_indices(n, 1)
    _both(n, s, d, tournament_sources(), k)


@pytest.mark.parametrize("k", KS)
def test_references_agree_on_degree_mix(k):
    V, s, d = degree_mix()
    _both(V, s, d, degree_mix_sources(V, s, d), k)


@pytest.mark.parametrize("k", KS)
def test_references_agree_on_random_multigraph(k):
    V, s, d = random_multigraph(2000, 60000, 7)
    _both(V, s, d, list(range(0, 2000, 59)), k)   # 34 sources


# ---- closed forms ----
def test_sink_source_keeps_everything():
    """A sink's mass is lost in the first superstep: r = a at the source, 0.0 elsewhere, S = a."""
    V, s, d = random_multigraph(300, 600, 2)
    outdeg, _ = pr_ref.degrees(V, s, d)
    sink = int(np.flatnonzero(outdeg == 0)[0])
    for k in KS:
        R, S = _both(V, s, d, [sink, 3], k, 0.25)
        assert R[0, sink] == 1.0 and np.count_nonzero(R[0]) == 1 and S[0] == 0.25


def test_repeated_source_columns_are_equal():
    V, s, d = random_multigraph(300, 2000, 1)
    R, S = _both(V, s, d, [4, 9, 4], 5)
    assert np.array_equal(R[0], R[2]) and S[0] == S[2] and not np.array_equal(R[0], R[1])


def test_path_by_hand():
    """0 -> 1 -> 2 from 0 and from 1, a = 0.15, k = 2: raw (0.15, 0.1275, 0.7225) and
    (0, 0.15, 0.85 * 0.15) -- the step from 1 into the sink 2 is the last mass that survives."""
    R, S = _both(3, [0, 1], [1, 2], [0, 1], 2)
    assert S == pytest.approx([1.0, 0.2775], rel=1e-15)
    assert R[0] == pytest.approx([0.15, 0.1275, 0.7225], rel=1e-15)
    assert R[1] == pytest.approx([0.0, 0.15 / 0.2775, 0.1275 / 0.2775], rel=1e-15) and R[1, 0] == 0.0


def test_nonzero_counts_walks_of_at_most_k_edges():
    V, s, d = random_multigraph(2000, 3000, 11)
    sources = [0, 5, 1999, 5]
    for k in (1, 3):
        R, _ = ppr_ref.parallel(V, s, d, sources, k)
        assert int((R > 0).sum()) == ppr_ref.reachable_pairs(V, s, d, sources, k)


def test_no_sources_and_no_vertices():
    e = np.empty(0, np.int32)
    R, S = ppr_ref.parallel(5, e, e, [], 3)
    assert R.shape == (0, 5) and S.shape == (0,)
    R, S = ppr_ref.parallel(0, e, e, [], 3)
    assert R.shape == (0, 0) and S.shape == (0,)
