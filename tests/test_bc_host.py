"""Host-side checks of the betweenness centrality (no GPU): the ABI version, the symbol and the
summary's size, the two CPU references of tests/bc_ref.py against each other (and against the
closed forms of the fixtures), the scaling table, the documented pivot draw and the argument
checks of GraphFrame.betweennessCentrality / Graph.betweenness, which run before any device
work."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import bc_ref
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import random_multigraph


def test_abi_version_has_betweenness():
    assert _lib.load().lpa_abi_version() >= 22


def test_symbol_and_summary_size():
    lib = _lib.load()
    assert "lpa_betweenness" in _lib.SIGNATURES
    assert lib.lpa_betweenness(None, None, 0, 1, 0, None, 0, None) == _lib.LPA_EINVAL   # null handle
    assert ctypes.sizeof(_lib.LpaBcSummary) == 56
    assert list(_lib.LpaBcSummary().to_dict()) == ["arcs", "sources", "batches", "batch_width", "reached",
                                                   "max_depth", "levels"]


def test_exports():
    assert "betweenness_centrality" in gfa.__all__ and callable(gfa.betweenness_centrality)
    assert callable(gfa.GraphFrame.betweennessCentrality) and callable(gfa.Graph.betweenness)
    assert "binary64" in gfa.GraphFrame.betweennessCentrality.__doc__
    assert "2^53" in gfa.GraphFrame.betweennessCentrality.__doc__


# ---- the references ----
def _close(a, b):
    assert np.array_equal(a == 0, b == 0)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


@pytest.mark.parametrize("directed", [True, False], ids=["directed", "undirected"])
def test_references_agree(directed):
    rng = np.random.default_rng(2207)
    for case in range(12):
        V = int(rng.integers(1, 60))
        V, s, d = random_multigraph(V, int(rng.integers(0, 4 * V)), 100 + case)
        r = bc_ref.brandes(V, s, d, None, directed)
        for normalized in (True, False):
            _close(bc_ref.scale(r["raw"], V, V, directed, normalized), bc_ref.networkx_bc(V, s, d, directed, normalized))


def test_subset_is_networkx_subset_with_k_scaling():
    import networkx as nx

    V, s, d = random_multigraph(80, 300, 5)
    S = bc_ref.pivots(V, 13, 1)
    for directed in (True, False):
        G = nx.DiGraph() if directed else nx.Graph()
        G.add_nodes_from(range(V))
        G.add_edges_from(bc_ref.simple_arcs(V, s, d))
        sub = nx.betweenness_centrality_subset(G, S.tolist(), list(range(V)), normalized=False)
        want = np.asarray([sub[v] for v in range(V)]) * (V / S.size)   # the subset call halves undirected itself
        got = bc_ref.scale(bc_ref.brandes(V, s, d, S, directed)["raw"], V, S.size, directed, normalized=False)
        _close(got, want)


def test_fixture_closed_forms():
    V, s, d = bc_ref.path(300)
    r = bc_ref.brandes(V, s, d)
    i = np.arange(300.0)
    assert np.array_equal(r["raw"], i * (299 - i)) and r["max_depth"] == 299 and r["max_list"] == 1
    V, s, d = bc_ref.diamond_chain(40)
    r = bc_ref.brandes(V, s, d)
    assert V == 161 and r["max_depth"] == 80 and r["arcs"] == 240
    _close(r["raw"], bc_ref.networkx_bc(V, s, d, True, False))
    V, s, d, centres = bc_ref.form_stars()
    n = centres.size // 2
    lengths = [0, 1, 8, 9, 32, 33, 1024, 1025]
    arcs = np.asarray(bc_ref.simple_arcs(V, s, d))
    assert np.bincount(arcs[:, 0], minlength=V)[centres[:n]].tolist() == lengths
    assert np.bincount(arcs[:, 1], minlength=V)[centres[n:]].tolist() == lengths


def test_scaling_table():
    raw = np.array([0.0, 6.0, 2.0, 0.0])
    assert np.array_equal(bc_ref.scale(raw, 4, 4, True, False), raw)
    assert np.array_equal(bc_ref.scale(raw, 4, 4, False, False), raw / 2)
    assert np.array_equal(bc_ref.scale(raw, 4, 2, True, True), raw * 2 / 6)
    assert np.array_equal(bc_ref.scale(raw, 4, 2, False, True), raw * 2 / 6)
    assert np.array_equal(bc_ref.scale(raw[:2], 2, 2, True, True), np.zeros(2))


# ---- argument checks: all before any device work (no GPU here) ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": ["a", "b", "c", "d"], "age": [1, 2, 3, 4]})
    e = pd.DataFrame({"src": ["a", "b", "c"], "dst": ["b", "c", "d"]})
    return gfa.GraphFrame(v, e)


def test_pivot_draw_is_the_documented_one(gf):
    for V, k, seed in ((4, 2, 0), (4, 4, 9), (4, 1, 3)):
        want = np.sort(np.random.default_rng(seed).choice(V, size=k, replace=False))
        got = gf._bc_sources(None, k, seed)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert np.array_equal(bc_ref.pivots(V, k, seed), want)
    assert gf._bc_sources(None, None, 0) is None
    assert gf._bc_sources(["c", "a"], None, 0).tolist() == [2, 0]
    assert gf._bc_sources(np.array(["d"]), None, 0).tolist() == [3]
    assert gf._graph is None   # nothing touched the device


@pytest.mark.parametrize("kwargs, match", [
    (dict(sources=["a", "zz"]), "source 'zz' is not a vertex id"),
    (dict(sources=[None]), "is not a vertex id"),
    (dict(sources=[1]), "is not a vertex id"),
    (dict(sources=["a", "b", "a"]), "a source is repeated"),
    (dict(sources=[]), "sources is empty"),
    (dict(sources=()), "sources is empty"),
    (dict(sources=np.array([], dtype=object)), "sources is empty"),
    (dict(sources=["a"], k=1), "sources or k, not both"),
    (dict(k=0), r"k must belong to \[1, 4\]"),
    (dict(k=5), r"k must belong to \[1, 4\]"),
    (dict(k=-1), r"k must belong to \[1, 4\]"),
])
def test_value_errors_before_device_work(gf, kwargs, match):
    with pytest.raises(ValueError, match=match):
        gf.betweennessCentrality(**kwargs)
    with pytest.raises(ValueError, match=match):
        gfa.betweenness_centrality(gf.vertices, gf.edges, **kwargs)
    assert gf._graph is None


@pytest.mark.parametrize("kwargs", [dict(sources="a"), dict(sources=7), dict(sources=np.array([["a"]])),
                                    dict(k=1.5), dict(k=True), dict(k=2, seed="x")])
def test_type_errors_before_device_work(gf, kwargs):
    with pytest.raises(TypeError):
        gf.betweennessCentrality(**kwargs)
    assert gf._graph is None


def test_graph_betweenness_checks_before_the_handle():
    """Graph.betweenness validates on the host first: on an object whose handle is closed (a call
    that got as far as the library would raise "graph handle is closed")."""
    g = object.__new__(gfa.Graph)
    g._lib, g._h, g.num_vertices, g.device = _lib.load(), ctypes.c_void_p(), 5, 0
    with pytest.raises(ValueError, match="graph handle is closed"):
        g.betweenness([0, 1])
    for bad in (2, 3, 32, -1):
        with pytest.raises(ValueError, match="batch must be 0, 1, 4, 8 or 16"):
            g.betweenness(batch=bad)
    with pytest.raises(TypeError):
        g.betweenness(batch=True)
    with pytest.raises(ValueError, match="source 5 is not a vertex"):
        g.betweenness([0, 5])
    with pytest.raises(ValueError, match="source -1 is not a vertex"):
        g.betweenness([-1])
    with pytest.raises(ValueError, match="repeated"):
        g.betweenness([1, 2, 1])
    with pytest.raises(TypeError):
        g.betweenness([1.0])
    with pytest.raises(ValueError, match="float64 device tensor"):
        g.betweenness(out=np.zeros(5))
