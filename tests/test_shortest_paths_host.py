"""Landmark shortest paths, the part that needs no GPU: the C-ABI boundary of
lpa_shortest_paths, the exported names, the argument checks of GraphFrame.shortestPaths and
Graph.shortest_paths (they run before any device work), and the two CPU references of
tests/sp_ref.py (a numpy BFS per landmark; scipy's csgraph on the pattern matrix) checked
against each other exactly and against closed forms."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import sp_ref
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph


def test_null_handle_is_einval():
    lib = _lib.load()
    lm = (ctypes.c_int32 * 1)(0)
    assert lib.lpa_shortest_paths(None, lm, 1, None, 0, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_shortest_paths():
    assert _lib.load().lpa_abi_version() >= 11


def test_summary_struct_layout():
    s = _lib.LpaSpSummary(1, 2, 3, 4, 5, 6)
    assert s.to_dict() == dict(arcs=1, reached=2, max_distance=3, batches=4, push_levels=5, pull_levels=6)
    assert ctypes.sizeof(_lib.LpaSpSummary) == 48


def test_function_form_exported():
    assert "shortest_paths" in gfa.__all__
    assert callable(gfa.shortest_paths)
    assert callable(gfa.GraphFrame.shortestPaths) and callable(gfa.Graph.shortest_paths)


# ---- argument checks: none of them reaches the device ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": np.array([30, 10, 20], np.int64), "name": ["c", "a", "b"]})
    e = pd.DataFrame({"src": np.array([10, 20], np.int64), "dst": np.array([20, 30], np.int64)})
    f = gfa.GraphFrame(v, e)
    yield f
    assert f._graph is None   # no handle was ever built


@pytest.mark.parametrize("bad", ["10", b"10", 10, 10.0, None, {10}, {10: 1}, np.array([[10, 20]])])
def test_landmarks_must_be_a_sequence(gf, bad):
    with pytest.raises(TypeError, match="landmarks"):
        gf.shortestPaths(bad)
    with pytest.raises(TypeError, match="landmarks"):
        gfa.shortest_paths(gf.vertices, gf.edges, bad)


@pytest.mark.parametrize("lms", [[99], [10, 15], ["10"], (20, None), np.array([10, 31]), [10, 10, -1]])
def test_landmark_must_be_a_vertex(gf, lms):
    with pytest.raises(ValueError, match=r"landmark .* is not a vertex id"):
        gf.shortestPaths(lms)
    with pytest.raises(ValueError, match=r"landmark .* is not a vertex id"):
        gfa.shortest_paths(gf.vertices, gf.edges, lms)


def test_landmark_must_be_a_vertex_string_ids():
    v = pd.DataFrame({"id": ["b", "a", "c"]})
    e = pd.DataFrame({"src": ["a"], "dst": ["b"]})
    f = gfa.GraphFrame(v, e)
    for lms in (["a", "zz"], [0], ["a", 1.5]):
        with pytest.raises(ValueError, match=r"landmark .* is not a vertex id"):
            f.shortestPaths(lms)
    assert f._graph is None


@pytest.mark.parametrize("empty", [[], (), np.empty(0, np.int64)])
def test_no_landmarks_needs_no_handle(gf, empty):
    out = gf.shortestPaths(empty)
    assert list(out.columns) == ["id", "name", "distances"] and out["distances"].dtype == object
    assert out["id"].tolist() == [10, 20, 30] and out["name"].tolist() == ["a", "b", "c"]
    assert out["distances"].tolist() == [{}, {}, {}]
    assert out.equals(gfa.shortest_paths(gf.vertices, gf.edges, empty))


def test_graph_method_argument_types():
    for bad in (["a"], [1.0], [True], [None], [0, np.float64(1)], [np.bool_(False)]):
        with pytest.raises(TypeError, match="landmark"):
            gfa.Graph.shortest_paths(None, bad)

    class _G:
        num_vertices = 5

    for bad in ([5], [-1], [0, 4, 7], np.array([2, 5], np.int64)):
        with pytest.raises(ValueError, match=r"landmark -?\d+ is not a vertex of \[0, 5\)"):
            gfa.Graph.shortest_paths(_G(), bad)


# ---- the two reference forms ----
def _both(V, s, d, lms):
    a = sp_ref.shortest_paths(V, s, d, lms)
    b = sp_ref.shortest_paths_csr(V, s, d, lms)
    assert a.dtype == np.int32 and a.shape == (len(lms), V) and b.dtype == np.int32
    assert np.array_equal(a, b)
    assert all(a[i, int(l)] == 0 for i, l in enumerate(lms))
    return a


def test_references_agree_on_r9(golden):
    V = int(golden["ids"].size)
    lms = sp_ref.top_in_degree(V, golden["src"], golden["dst"], 70)
    dist = _both(V, golden["src"], golden["dst"], lms)
    per_landmark = (dist >= 0).sum(axis=1)
    assert int(per_landmark.min()) == 2 and int(per_landmark.max()) == 569 and int(dist.max()) == 6
    summ = sp_ref.summary(V, golden["src"], golden["dst"], dist)
    assert summ["batches"] == 2 and summ["max_distance"] == 6 and summ["reached"] == int(per_landmark.sum())


def test_references_agree_on_degree_mix():
    V, s, d = degree_mix()
    lms = sp_ref.evenly_spaced(V, 130)
    dist = _both(V, s, d, lms)
    per_landmark = (dist >= 0).sum(axis=1)
    assert int(per_landmark.min()) == 1 and int(per_landmark.max()) == 3001 and int(dist.max()) == 7
    assert sp_ref.summary(V, s, d, dist)["batches"] == 3


def test_references_agree_on_random_multigraph():
    V, s, d = random_multigraph(2000, 60000, 7)
    dist = _both(V, s, d, np.arange(0, V, 29))
    assert (dist >= 0).all()   # 30 out-edges a vertex: strongly connected
    repeated, once = _both(V, s, d, [5, 5, 9, 5]), _both(V, s, d, [5])[0]
    assert all(np.array_equal(repeated[i], once) for i in (0, 1, 3)) and not np.array_equal(repeated[2], once)


# ---- closed forms ----
def test_directed_path():
    n = 2000
    V, s, d = sp_ref.path(n)
    dist = _both(V, s, d, [n - 1, 0])
    assert np.array_equal(dist[0], n - 1 - np.arange(n))
    assert dist[1, 0] == 0 and (dist[1, 1:] == -1).all()
    assert sp_ref.summary(V, s, d, dist) == dict(arcs=n - 1, reached=n + 1, max_distance=n - 1, batches=1, levels=n)


def test_directed_cycle():
    n = 1000
    V, s, d = sp_ref.cycle(n)
    lms = [0, 1, 499, 999]
    dist = _both(V, s, d, lms)
    for row, l in zip(dist, lms):
        assert np.array_equal(row, (l - np.arange(n)) % n)


def test_one_edge_both_directions():
    dist = _both(2, [0], [1], [1, 0])
    assert dist.tolist() == [[1, 0], [0, -1]]   # 0 reaches 1 in one step; 1 never reaches 0


def test_duplicates_loops_and_dropped_edges_change_nothing():
    V, s, d = random_multigraph(300, 900, 3)
    lms = [0, 17, 299]
    want = _both(V, s, d, lms)
    s2 = np.concatenate([s, s[:200], np.arange(50), [-1, 300, 4]]).astype(np.int32)
    d2 = np.concatenate([d, d[:200], np.arange(50), [3, 5, 300]]).astype(np.int32)
    assert np.array_equal(_both(V, s2, d2, lms), want)
    assert sp_ref.summary(V, s2, d2, want) == sp_ref.summary(V, s, d, want)


def test_no_vertices_and_no_landmarks():
    e = np.empty(0, np.int32)
    for f in (sp_ref.shortest_paths, sp_ref.shortest_paths_csr):
        assert f(0, e, e, []).shape == (0, 0)
        assert f(7, [0], [1], []).shape == (0, 7)
    assert sp_ref.summary(0, e, e, np.empty((0, 0), np.int32)) == dict(arcs=0, reached=0, max_distance=-1, batches=0,
                                                                        levels=0)
    assert sp_ref.summary(7, [0, 0, 3], [1, 1, 3], np.empty((0, 7), np.int32)) == dict(
        arcs=1, reached=0, max_distance=-1, batches=0, levels=0)
