"""Static PageRank, the part that needs no GPU: the C-ABI boundary of lpa_pagerank, the
exported names, the argument checks of GraphFrame.pageRank (they run before any device
work), and the two CPU references of tests/pr_ref.py (np.bincount per superstep; a scipy CSR
product) checked against each other within pr_ref.bound and against closed forms."""
import ctypes
import math

import numpy as np
import pandas as pd
import pytest

import pr_ref
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph

KS = (1, 5, 20)


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_pagerank(None, 5, 0.15, -1, None, None, None, 0, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_pagerank():
    assert _lib.load().lpa_abi_version() >= 10


def test_summary_struct_layout():
    s = _lib.LpaPagerankSummary(1.5, 2.5, 3, 4, 5, 6)
    assert s.to_dict() == dict(rank_sum=1.5, max_rank=2.5, max_rank_id=3, edges=4, sinks=5, max_in_degree=6)
    assert ctypes.sizeof(_lib.LpaPagerankSummary) == 48


def test_function_form_exported():
    assert "page_rank" in gfa.__all__
    assert callable(gfa.page_rank)
    assert callable(gfa.GraphFrame.pageRank) and callable(gfa.Graph.pagerank)
    assert callable(gfa.GraphFrame.inDegrees) and callable(gfa.GraphFrame.outDegrees)


# ---- argument checks: none of them reaches the device ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": np.array([30, 10, 20], np.int64)})
    e = pd.DataFrame({"src": np.array([10, 20], np.int64), "dst": np.array([20, 30], np.int64)})
    f = gfa.GraphFrame(v, e)
    yield f
    assert f._graph is None   # no handle was ever built


def test_max_iter_and_tol(gf):
    with pytest.raises(ValueError, match=r"^Exactly one of maxIter or tol should be set\.$"):
        gf.pageRank()
    with pytest.raises(ValueError, match=r"^Exactly one of maxIter or tol should be set\.$"):
        gf.pageRank(maxIter=5, tol=0.01)
    with pytest.raises(NotImplementedError, match="maxIter"):
        gf.pageRank(tol=0.01)


@pytest.mark.parametrize("n", [0, -3])
def test_max_iter_positive(gf, n):
    with pytest.raises(ValueError, match=rf"^requirement failed: Number of iterations must be greater than 0, but got {n}$"):
        gf.pageRank(maxIter=n)
    with pytest.raises(ValueError, match="Number of iterations must be greater than 0"):
        gfa.page_rank(gf.vertices, gf.edges, n)


@pytest.mark.parametrize("bad", [2.0, "5", True, None])
def test_max_iter_type(gf, bad):
    if bad is None:   # the function form has no tol: a missing maxIter is the both-or-neither error
        with pytest.raises(ValueError, match="Exactly one"):
            gfa.page_rank(gf.vertices, gf.edges, None)
        return
    with pytest.raises(TypeError, match="maxIter"):
        gf.pageRank(maxIter=bad)


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan")])
def test_reset_probability_range(gf, p):
    with pytest.raises(ValueError, match=r"^requirement failed: Random reset probability must belong to \[0, 1\], but got "):
        gf.pageRank(resetProbability=p, maxIter=5)
    if not math.isnan(p):
        with pytest.raises(ValueError, match=rf"but got {p}$"):
            gf.pageRank(resetProbability=p, maxIter=5)


@pytest.mark.parametrize("sid", [99, 15, "10"])
def test_source_id_must_be_a_vertex(gf, sid):
    with pytest.raises(ValueError, match="sourceId"):
        gf.pageRank(maxIter=5, sourceId=sid)


def test_graph_method_argument_types():
    with pytest.raises(TypeError, match="max_iter"):
        gfa.Graph.pagerank(None, 2.5)
    with pytest.raises(TypeError, match="source"):
        gfa.Graph.pagerank(None, 2, source="a")


# ---- the two reference forms ----
def _both(V, s, d, k, a=0.15, source=None):
    r1, o1, i1, S1 = pr_ref.pagerank(V, s, d, k, a, source)
    r2, o2, i2, S2 = pr_ref.pagerank_csr(V, s, d, k, a, source)
    assert r1.dtype == np.float64 and r1.shape == (V,)
    assert np.array_equal(o1, o2) and np.array_equal(i1, i2)
    b = pr_ref.bound(k, int(i1.max()) if V else 0, V)
    assert (np.abs(r1 - r2) <= b * r1).all(), float(np.max(np.abs(r1 - r2) / np.where(r1 > 0, r1, 1.0)))
    assert np.array_equal(r1 == 0.0, r2 == 0.0)
    assert abs(S1 - S2) <= b * S1
    total = V if source is None else 1.0
    assert abs(float(r1.sum()) - total) <= V * 2.0 ** -52
    return r1, o1, i1, S1


@pytest.mark.parametrize("k", KS)
def test_references_agree_on_r9(golden, k):
    V = int(golden["ids"].size)
    _, outdeg, indeg, _ = _both(V, golden["src"], golden["dst"], k)
    assert int((outdeg == 0).sum()) == 3917 and int(indeg.max()) == 1223
    _both(V, golden["src"], golden["dst"], k, source=int(np.argmax(outdeg)))


@pytest.mark.parametrize("k", KS)
def test_references_agree_on_degree_mix(k):
    V, s, d = degree_mix()
    _both(V, s, d, k)
    _both(V, s, d, k, source=int(s[0]))


@pytest.mark.parametrize("k", KS)
def test_references_agree_on_random_multigraph(k):
    V, s, d = random_multigraph(2000, 60000, 7)
    _both(V, s, d, k)
    _both(V, s, d, k, source=17)


# ---- closed forms ----
def test_directed_cycle_is_uniform():
    n = 1000
    i = np.arange(n)
    for k in KS:
        r, outdeg, indeg, S = _both(n, i, (i + 1) % n, k)
        assert (r == 1.0).all() and S == n and (outdeg == 1).all() and (indeg == 1).all()


def test_complete_digraph_is_uniform():
    n = 70
    a, b = np.nonzero(~np.eye(n, dtype=bool))
    for k in KS:
        r, _, indeg, _ = _both(n, a, b, k)
        assert (indeg == n - 1).all()
        assert (np.abs(r - 1.0) <= pr_ref.bound(k, n - 1, n)).all()


def test_two_vertices_one_edge():
    """0 -> 1, a = 0.15.  Superstep 1 reads r = (1, 1): raw (0.15, 0.15 + 0.85 * 1).  Every
    later one reads r[0] = 0.15: raw (0.15, 0.15 + 0.85 * 0.15) = (0.15, 0.2775), normalised
    by 2 / 0.4275.  Vertex 1 is a sink: its mass never comes back."""
    r, outdeg, indeg, S = _both(2, [0], [1], 1)
    assert outdeg.tolist() == [1, 0] and indeg.tolist() == [0, 1]
    assert S == pytest.approx(1.15, rel=1e-15) and r == pytest.approx([0.3 / 1.15, 2.0 / 1.15], rel=1e-15)
    for k in (2, 3, 5, 20):
        r, _, _, S = _both(2, [0], [1], k)
        assert S == pytest.approx(0.4275, rel=1e-15)
        assert r == pytest.approx([0.15 * 2 / 0.4275, 0.2775 * 2 / 0.4275], rel=1e-15)


def test_repeated_edge_to_the_only_target():
    for k in KS:
        once, _, _, _ = _both(3, [0, 1], [1, 2], k)
        thrice, outdeg, indeg, _ = _both(3, [0, 0, 0, 1], [1, 1, 1, 2], k)
        assert outdeg.tolist() == [3, 1, 0] and indeg.tolist() == [0, 3, 1]
        assert (np.abs(once - thrice) <= pr_ref.bound(k, 3, 3) * once).all()


def test_self_loops():
    """A vertex whose only edge is its self-loop: r <- a + (1 - a) r.  With a second edge
    0 -> 1 the loop carries half: r0 <- a + (1 - a) r0 / 2, r1 <- a + (1 - a) r0 / 2."""
    a = 0.25
    for k in KS:
        raw, _, _, S = pr_ref.pagerank(2, [0], [0], k, a)
        x = 1.0
        for _ in range(k):
            x = a + (1 - a) * x
        assert S == pytest.approx(x + a, rel=1e-15) and raw == pytest.approx([2 * x / (x + a), 2 * a / (x + a)], rel=1e-14)
        _both(2, [0], [0], k, a)
        r, outdeg, indeg, S = _both(2, [0, 0], [0, 1], k, a)
        assert outdeg.tolist() == [2, 0] and indeg.tolist() == [1, 1]
        x = 1.0
        for _ in range(k):
            x = a + (1 - a) * (x * 0.5)
        assert S == pytest.approx(2 * x, rel=1e-15) and r == pytest.approx([1.0, 1.0], rel=1e-14)


def test_reset_probability_one():
    V, s, d = random_multigraph(300, 2000, 1)
    for k in KS:
        r, _, _, S = _both(V, s, d, k, 1.0)
        assert (r == 1.0).all() and S == V
        r, _, _, S = _both(V, s, d, k, 1.0, source=4)
        assert r[4] == 1.0 and S == 1.0 and np.count_nonzero(r) == 1


def test_personalised_path_by_hand():
    """0 -> 1 -> 2 from 0, a = 0.15 (w = (1, 1, 0)):
    k = 1  r = (0.15, 0.85, 0)                          S = 1
    k = 2  r = (0.15, 0.85 * 0.15, 0.85 * 0.85)         S = 1
    k = 3  r = (0.15, 0.1275, 0.85 * 0.1275)            S = 0.385875"""
    s, d = [0, 1], [1, 2]
    want = {1: ([0.15, 0.85, 0.0], 1.0), 2: ([0.15, 0.1275, 0.7225], 1.0), 3: ([0.15, 0.1275, 0.108375], 0.385875)}
    for k, (raw, S) in want.items():
        r, _, _, got_S = _both(3, s, d, k, 0.15, source=0)
        assert got_S == pytest.approx(S, rel=1e-15)
        assert r == pytest.approx([x / S for x in raw], rel=1e-15)
        assert (r == 0.0).tolist() == [x == 0.0 for x in raw]


def test_no_vertices():
    e = np.empty(0, np.int32)
    for f in (pr_ref.pagerank, pr_ref.pagerank_csr):
        r, outdeg, indeg, S = f(0, e, e, 3)
        assert r.size == 0 and outdeg.size == 0 and indeg.size == 0 and S == 0.0
        assert pr_ref.summary(r, outdeg, indeg, S) == dict(rank_sum=0.0, max_rank=0.0, max_rank_id=-1, edges=0,
                                                           sinks=0, max_in_degree=0)


def test_edgeless_and_dropped_edges():
    r, outdeg, indeg, S = _both(4, [0, 7, -1], [9, 1, 2], 5)   # no edge has both ends in [0, 4)
    assert (r == 1.0).all() and not outdeg.any() and not indeg.any() and S == pytest.approx(0.6, rel=1e-15)
    assert pr_ref.summary(r, outdeg, indeg, S)["sinks"] == 4
