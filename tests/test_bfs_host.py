"""Host-side checks of the breadth-first search (no GPU): the ABI version and the symbol, the
summary's size, the two CPU references against each other on a seeded random family,
enumerate_paths against the literal join loop (path set and row order), the argument checks of
GraphFrame.bfs / Graph.bfs (they run before any device work) and the two shortcuts that never
touch the GPU."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import bfs_ref
import graphframes_amd as gfa
from graphframes_amd import _lib


def test_abi_version_has_bfs():
    assert _lib.load().lpa_abi_version() >= 18


def test_symbol_and_summary_size():
    lib = _lib.load()
    assert "lpa_bfs" in _lib.SIGNATURES
    assert lib.lpa_bfs(None, None, None, None, 1, None, None, None) == _lib.LPA_EINVAL   # null handle
    assert ctypes.sizeof(_lib.LpaBfsSummary) == 72
    assert list(_lib.LpaBfsSummary().to_dict()) == ["arcs", "sources", "targets", "length", "reached",
                                                    "path_vertices", "path_edges", "push_levels", "pull_levels"]


def test_exports():
    for name in ("bfs", "enumerate_paths", "count_paths"):
        assert name in gfa.__all__ and callable(getattr(gfa, name))
    assert callable(gfa.GraphFrame.bfs) and callable(gfa.Graph.bfs)


# ---- the references ----
@pytest.fixture(scope="module")
def family():
    """(case, literal result, levels_dag result) of 1500 seeded random cases."""
    rng = np.random.default_rng(20180)
    out = []
    for _ in range(1500):
        case = bfs_ref.random_case(rng)
        out.append((case, bfs_ref.literal(*case), bfs_ref.levels_dag(*case)))
    return out


def test_references_agree(family):
    found = 0
    for (V, s, d, F, T, keep, max_len), (length, paths), dag in family:
        assert dag["length"] == length
        level, on_edge = dag["level"], dag["on_edge"]
        if length > 0:
            found += 1
            verts, edges = gfa.enumerate_paths(level, s, d, np.flatnonzero(on_edge), length)
            assert sorted(bfs_ref.path_tuples(verts, edges)) == paths
            on_v = sorted({v for p in paths for v in p[0::2]})
            assert np.flatnonzero(level >= 0).tolist() == on_v
            assert np.flatnonzero(on_edge).tolist() == sorted({e for p in paths for e in p[1::2]})
            for p in paths:
                assert [int(level[v]) for v in p[0::2]] == list(range(length + 1))
        elif length == 0:
            assert np.flatnonzero(level == 0).tolist() == [p[0] for p in paths] and not on_edge.any()
            assert (level <= 0).all()
        else:
            assert (level == -1).all() and not on_edge.any()
    assert found >= 200, found   # the family does exercise the search


def test_enumerate_paths_row_order(family):
    for (V, s, d, F, T, keep, max_len), (length, paths), dag in family:
        if length <= 0:
            continue
        eidx = np.flatnonzero(dag["on_edge"])
        verts, edges = gfa.enumerate_paths(dag["level"], s, d, eidx, length)
        assert verts.dtype == np.int32 and verts.shape == (len(paths), length + 1)
        assert edges.dtype == np.int64 and edges.shape == (len(paths), length)
        keys = [tuple(r) for r in edges.tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert gfa.count_paths(dag["level"], s, d, eidx, length) == len(paths)
        for j in range(length):   # every row is a walk over its edges
            assert np.array_equal(s[edges[:, j]], verts[:, j]) and np.array_equal(d[edges[:, j]], verts[:, j + 1])


def test_lattice_has_27_paths():
    V, s, d = bfs_ref.lattice(4, 3)
    F, T = np.arange(V) < 3, np.arange(V) == V - 1      # the first layer to one vertex of the last
    assert len(bfs_ref.literal(V, s, d, F, T)[1]) == 27
    F, T = np.arange(V) == 0, np.arange(V) >= 9         # one vertex of the first layer to the last
    length, paths = bfs_ref.literal(V, s, d, F, T)
    dag = bfs_ref.levels_dag(V, s, d, F, T)
    assert length == dag["length"] == 3 and len(paths) == 27
    verts, edges = gfa.enumerate_paths(dag["level"], s, d, np.flatnonzero(dag["on_edge"]), 3)
    assert bfs_ref.path_tuples(verts, edges) == paths     # the promised order is literal()'s sorted order here
    assert gfa.count_paths(dag["level"], s, d, np.flatnonzero(dag["on_edge"]), 3) == 27
    assert dag["summary"]["path_edges"] == 3 + 9 + 9 and dag["summary"]["path_vertices"] == 1 + 3 + 3 + 3


def test_enumerate_paths_degenerate():
    verts, edges = gfa.enumerate_paths(np.full(5, -1, np.int32), np.empty(0, np.int32), np.empty(0, np.int32),
                                       np.empty(0, np.int64), -1)
    assert verts.shape[0] == 0 and edges.shape[0] == 0
    assert gfa.count_paths(np.zeros(3, np.int32), [], [], [], 0) == 0


# ---- argument checks: all before any device work (no GPU here) ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": ["a", "b", "c", "d"], "age": [1, 2, 3, 4]})
    e = pd.DataFrame({"src": ["a", "b", "c"], "dst": ["b", "c", "d"], "rel": ["x", "y", "x"]})
    return gfa.GraphFrame(v, e)


def test_max_path_length_checks(gf):
    msg = "requirement failed: BFS maxPathLength must be >= 0, but was set to -1"
    with pytest.raises(ValueError) as ei:
        gf.bfs("id == 'a'", "id == 'd'", maxPathLength=-1)
    assert str(ei.value) == msg
    with pytest.raises(ValueError) as ei:
        gfa.bfs(gf.vertices, gf.edges, "id == 'a'", "id == 'd'", maxPathLength=-1)
    assert str(ei.value) == msg
    for bad in (2.0, True, "3", None):
        with pytest.raises(TypeError, match="maxPathLength"):
            gf.bfs("id == 'a'", "id == 'd'", maxPathLength=bad)
        with pytest.raises(TypeError, match="maxPathLength"):
            gfa.bfs(gf.vertices, gf.edges, "id == 'a'", "id == 'd'", maxPathLength=bad)


def test_expression_checks(gf):
    ok = "id == 'd'"
    for bad in (3, None, ["a"], [True, False, False, False]):
        with pytest.raises(TypeError, match="fromExpr"):
            gf.bfs(bad, ok)
        with pytest.raises(TypeError, match="toExpr"):
            gf.bfs(ok, bad)
    with pytest.raises(TypeError, match="edgeFilter"):
        gf.bfs("id == 'a'", ok, edgeFilter=7)
    with pytest.raises(ValueError, match="fromExpr must yield 4 entries, got 3"):    # wrong length
        gf.bfs(np.array([True, False, False]), ok)
    with pytest.raises(ValueError, match="edgeFilter must yield 3 entries, got 4"):
        gf.bfs("id == 'a'", ok, edgeFilter=np.ones(4, bool))
    with pytest.raises(TypeError, match="boolean"):                                  # wrong dtype
        gf.bfs(np.array([1, 0, 0, 0]), ok)
    with pytest.raises(TypeError, match="boolean"):
        gf.bfs("age + 1", ok)
    with pytest.raises(TypeError, match="boolean"):
        gf.bfs(lambda v: v["age"], ok)
    with pytest.raises(TypeError, match="dimensions"):
        gf.bfs(np.zeros((4, 1), bool), ok)
    with pytest.raises(ValueError, match="toExpr: cannot evaluate"):                 # unknown column
        gf.bfs("id == 'a'", "nosuch == 1")
    with pytest.raises(ValueError, match="edgeFilter: cannot evaluate"):
        gf.bfs("id == 'a'", ok, edgeFilter="age > 1")    # a vertex column is no edge column
    for bad in (1.5, True, "2"):
        with pytest.raises(TypeError, match="maxPaths"):
            gf.bfs("id == 'a'", ok, maxPaths=bad)
    with pytest.raises(ValueError, match="maxPaths"):
        gf.bfs("id == 'a'", ok, maxPaths=-1)


def test_graph_bfs_checks():
    class _G:
        num_vertices, num_edges = 4, 3
        _mask = staticmethod(gfa.Graph._mask)

    ok = np.zeros(4, bool)
    for bad in (1.0, True, None):
        with pytest.raises(TypeError, match="max_path_length"):
            gfa.Graph.bfs(_G(), ok, ok, max_path_length=bad)
    with pytest.raises(ValueError, match="negative"):
        gfa.Graph.bfs(_G(), ok, ok, max_path_length=-1)
    with pytest.raises(ValueError, match="from_mask must have 4 entries, got 5"):
        gfa.Graph.bfs(_G(), np.zeros(5, bool), ok)
    with pytest.raises(ValueError, match="edge_keep must have 3 entries, got 4"):
        gfa.Graph.bfs(_G(), ok, ok, edge_keep=np.zeros(4, np.uint8))
    with pytest.raises(TypeError, match="to_mask"):
        gfa.Graph.bfs(_G(), ok, np.zeros(4, np.int32))
    with pytest.raises(TypeError, match="dimensions"):
        gfa.Graph.bfs(_G(), np.zeros((2, 2), bool), ok)


# ---- the shortcuts: no search, no GPU ----
def test_empty_set_gives_empty_vertex_frame(gf):
    for a, b in (("id == 'zz'", "id == 'd'"), ("id == 'a'", "age > 99"), ("age < 0", "age < 0")):
        out = gf.bfs(a, b)
        assert list(out.columns) == ["id", "age"] and len(out) == 0
        assert out.dtypes.tolist() == gf.vertices.dtypes.tolist()
        assert out.attrs == {"length": -1, "paths": 0}
    assert gf._graph is None   # no handle was ever built
    out = gfa.bfs(gf.vertices, gf.edges, np.zeros(4, bool), lambda v: v["age"] > 0)
    assert len(out) == 0 and out.attrs["length"] == -1


def test_shared_vertices_come_back_as_from_and_to():
    v = pd.DataFrame({"id": [30, 10, 20, 10, 40], "name": ["c", "a", "b", "a-again", "d"]})
    e = pd.DataFrame({"src": [10, 20], "dst": [20, 30]})
    gf = gfa.GraphFrame(v, e)
    out = gf.bfs("id >= 20", "id <= 30", maxPathLength=0)
    assert out.columns.tolist() == [("from", "id"), ("from", "name"), ("to", "id"), ("to", "name")]
    assert out["from"]["id"].tolist() == [20, 30] and out["to"]["name"].tolist() == ["b", "c"]
    assert out["from"].equals(out["to"]) and out.attrs == {"length": 0, "paths": 2}
    # a repeated id: its first row stands for the vertex (row 3 says True, row 1 says False)
    out = gf.bfs(np.array([False, False, False, True, False]), "id == 10")
    assert len(out) == 0 and out.attrs["length"] == -1
    out = gf.bfs(np.array([False, True, False, False, False]), "id == 10")
    assert out["from"]["name"].tolist() == ["a"] and out.attrs["length"] == 0
    assert gf._graph is None


# ---- GraphFrame.bfs's host side on a handle answered by the reference ----
class _RefGraph:
    """Graph.bfs answered by levels_dag, so the frame assembly and maxPaths run without a GPU."""

    def __init__(self, ig):
        self.ig = ig

    def bfs(self, F, T, keep=None, max_path_length=10, stats=False):
        r = bfs_ref.levels_dag(self.ig.num_vertices, self.ig.src, self.ig.dst, F, T, keep, max_path_length)
        return r["length"], r["level"], np.flatnonzero(r["on_edge"]).astype(np.int64)


def test_max_paths_and_frame_assembly(monkeypatch):
    V, s, d = bfs_ref.lattice(4, 3)
    v = pd.DataFrame({"id": np.arange(V, dtype=np.int64)[::-1], "layer": np.arange(V)[::-1] // 3})
    e = pd.DataFrame({"src": np.append(s, 5).astype(np.int64), "dst": np.append(d, 99).astype(np.int64),
                      "n": np.arange(s.size + 1)})     # the last edge dangles
    gf = gfa.GraphFrame(v, e)
    monkeypatch.setattr(gf, "_gpu_graph", lambda: _RefGraph(gf._indexed()))
    out = gf.bfs("id == 0", "layer == 3")
    assert len(out) == 27 and out.attrs == {"length": 3, "paths": 27}
    assert out.columns.tolist() == [(g, c) for g, cols in (("from", ("id", "layer")), ("e0", ("src", "dst", "n")),
                                                           ("v1", ("id", "layer")), ("e1", ("src", "dst", "n")),
                                                           ("v2", ("id", "layer")), ("e2", ("src", "dst", "n")),
                                                           ("to", ("id", "layer"))) for c in cols]
    rows = list(zip(out["e0"]["n"], out["e1"]["n"], out["e2"]["n"]))
    assert rows == sorted(rows) and len(set(rows)) == 27
    assert out["e0"]["dst"].equals(out["v1"]["id"]) and out["e2"]["dst"].equals(out["to"]["id"])
    assert (out["v2"]["layer"] == 2).all() and sorted(set(out["to"]["id"])) == [9, 10, 11]
    with pytest.raises(ValueError, match="27 paths of 3 edges, more than maxPaths = 26"):
        gf.bfs("id == 0", "layer == 3", maxPaths=26)
    assert len(gf.bfs("id == 0", "layer == 3", maxPaths=27)) == 27
    assert len(gf.bfs("id == 0", "layer == 3", edgeFilter="n != 0", maxPaths=18)) == 18
    none = gf.bfs("id == 0", "layer == 3", maxPathLength=2)
    assert len(none) == 0 and list(none.columns) == ["id", "layer"] and none.attrs == {"length": -1, "paths": 0}
