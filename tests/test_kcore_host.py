"""k-core decomposition, the part that needs no GPU: the C-ABI boundary of lpa_core_numbers, the
exported names, the argument checks of Graph.core_numbers, GraphFrame.kCore and the function forms
(they run before any device work), and the two CPU restatements of tests/kcore_ref.py (a
vectorised peel; the h-index fixpoint) checked against each other, against networkx, against the
closed forms of the specification and against the definition of a k-core."""
import ctypes
import functools
import os

import numpy as np
import pandas as pd
import pytest

import kcore_ref as kc
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph, star, two_cliques


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_core_numbers(None, 3, None, None, 0, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_core_numbers():
    assert _lib.load().lpa_abi_version() >= 16


def test_struct_layout():
    s = _lib.LpaCoreSummary(1, 2, 3, 4, 5, 6, 7)
    assert tuple(s.to_dict()) == kc.SUMMARY_KEYS
    assert list(s.to_dict().values()) == [1, 2, 3, 4, 5, 6, 7]
    assert ctypes.sizeof(_lib.LpaCoreSummary) == 56


def test_exported():
    for name in ("core_number", "k_core"):
        assert name in gfa.__all__ and callable(getattr(gfa, name))
    assert callable(gfa.GraphFrame.coreNumber) and callable(gfa.GraphFrame.kCore)
    assert callable(gfa.Graph.core_numbers)
    assert "lpa_core_numbers" in _lib.SIGNATURES


# ---- argument checks: none of them reaches the device ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": np.array([30, 10, 20], np.int64), "name": ["c", "a", "b"]})
    e = pd.DataFrame({"src": np.array([10, 20], np.int64), "dst": np.array([20, 30], np.int64)})
    f = gfa.GraphFrame(v, e)
    yield f
    assert f._graph is None   # no handle was ever built


@pytest.mark.parametrize("bad", [2.5, True, "3", None, np.float64(4), np.bool_(True), [1]])
def test_k_must_be_an_int(gf, bad):
    with pytest.raises(TypeError, match="k must be an int"):
        gf.kCore(bad)
    with pytest.raises(TypeError, match="k must be an int"):
        gfa.k_core(gf.vertices, gf.edges, bad)
    if bad is not None:   # None is Graph.core_numbers' "no cap"
        with pytest.raises(TypeError, match="max_k must be an int"):
            gfa.Graph.core_numbers(None, bad)
        with pytest.raises(TypeError, match="max_k must be an int"):
            gfa.Graph.core_numbers(None, max_k=bad)


@pytest.mark.parametrize("bad", [-1, -7, np.int64(-2)])
def test_k_must_not_be_negative(gf, bad):
    with pytest.raises(ValueError, match=f"k must not be negative, but got {bad}"):
        gf.kCore(bad)
    with pytest.raises(ValueError, match="k must not be negative"):
        gfa.k_core(gf.vertices, gf.edges, bad)
    with pytest.raises(ValueError, match="max_k must not be negative"):
        gfa.Graph.core_numbers(None, bad)


def test_reference_checks_its_cap():
    for fn in (kc.core_numbers, kc.core_numbers_literal):
        with pytest.raises(ValueError):
            fn(2, [0], [1], max_k=-1)
        with pytest.raises(TypeError):
            fn(2, [0], [1], max_k=1.5)


# ---- the two reference forms ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r9_golden.npz")


def _r9():
    z = np.load(GOLDEN, allow_pickle=False)
    return int(z["ids"].size), z["src"], z["dst"]


def _heavy_triangle():
    a, b = np.array([0, 1, 2, 1, 2, 0]), np.array([1, 2, 0, 0, 1, 2])
    return (3, np.concatenate([np.tile(a, 100), [0, 1, 2, 2]]).astype(np.int32),
            np.concatenate([np.tile(b, 100), [0, 1, 2, 2]]).astype(np.int32))


CASES = {
    "empty": lambda: (0, np.empty(0, np.int32), np.empty(0, np.int32)),
    "one_vertex": lambda: (1, np.empty(0, np.int32), np.empty(0, np.int32)),
    "edgeless": lambda: (70, np.empty(0, np.int32), np.empty(0, np.int32)),
    "loops": lambda: (100, np.array([3, 3, 0, 99, 64], np.int32), np.array([3, 3, 0, 99, 64], np.int32)),
    "edge_x1000": lambda: (9, np.full(1000, 6, np.int32), np.full(1000, 2, np.int32)),
    "heavy_triangle": _heavy_triangle,
    "two_cliques": lambda: two_cliques(5),
    "star": lambda: star(500),
    "k3_500": lambda: kc.complete_bipartite(3, 500),
    "clique_leaves": lambda: kc.clique_with_leaves(40, 100),
    "overshoot": lambda: kc.overshoot(50),
    "k70": lambda: (70,) + kc.clique(70),
    "clique_chain": lambda: kc.clique_chain(3, 12),
    "grid": lambda: kc.grid(40, 40),
    "circulant": lambda: kc.circulant(1000, (1, 2)),
    "tree": lambda: kc.binary_tree(4095),
    "path300": lambda: kc.path(300),
    "r9": _r9,
    "degree_mix": degree_mix,
    "rm2000": lambda: random_multigraph(2000, 30000, 1),
}


@functools.lru_cache(maxsize=None)
def _both(name):
    """The case's graph and its uncapped reference, the two forms checked against each other once."""
    V, s, d = CASES[name]()
    core, deg = kc.core_numbers(V, s, d)
    lcore, ldeg = kc.core_numbers_literal(V, s, d)
    assert core.dtype == np.int32 and core.shape == (V,) and deg.dtype == np.int32 and deg.shape == (V,)
    assert np.array_equal(core, lcore) and np.array_equal(deg, ldeg)
    for a in (core, deg):
        a.setflags(write=False)
    return V, s, d, core, deg


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_agree(name):
    _both(name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_against_networkx(name):
    nx = pytest.importorskip("networkx")
    V, s, d, core, deg = _both(name)
    G = nx.Graph()
    G.add_nodes_from(range(V))
    G.add_edges_from((int(a), int(b)) for a, b in zip(s, d) if a != b)
    want = nx.core_number(G)
    assert core.tolist() == [want[v] for v in range(V)]
    assert deg.tolist() == [G.degree(v) for v in range(V)]


def _hist(core):
    return np.bincount(core).tolist()


def test_closed_forms():
    """The values the specification states."""
    V, s, d, core, deg = _both("two_cliques")
    summ = kc.summary_of(core, deg)
    assert summ["degeneracy"] == 5 and summ["main_core_size"] == 6
    assert _hist(_both("r9")[3]) == [0, 3430, 450, 202, 148, 164, 92, 73, 12, 42]
    assert _hist(_both("degree_mix")[3]) == [7, 40, 13, 26, 47, 78, 115, 167, 250, 560, 1751]
    assert (_both("star")[3] == 1).all()
    assert (_both("k3_500")[3] == 3).all()
    core = _both("clique_leaves")[3]
    assert (core[:40] == 39).all() and (core[40:] == 1).all()
    assert kc.summary_of(core, _both("clique_leaves")[4])["levels"] == 2
    core = _both("overshoot")[3]
    assert core.tolist() == [1, 2, 2, 2] + [1] * 50
    assert (_both("k70")[3] == 69).all()
    V, s, d, core, deg = _both("clique_chain")
    assert _hist(core) == [0, 0] + list(range(3, 13)) and kc.summary_of(core, deg)["levels"] == 10
    assert (_both("grid")[3] == 2).all() and (_both("circulant")[3] == 4).all()
    assert (_both("tree")[3] == 1).all() and (_both("path300")[3] == 1).all()
    assert _both("heavy_triangle")[3].tolist() == [2, 2, 2] and _both("edge_x1000")[3].sum() == 2
    assert not _both("loops")[3].any() and not _both("edgeless")[3].any()


def test_summary_fields():
    V, s, d, core, deg = _both("degree_mix")
    summ = kc.summary(V, s, d)
    assert tuple(summ) == kc.PURE_KEYS
    assert summ == dict(degeneracy=10, main_core_size=1751, levels=11, simple_edges=int(deg.sum()) // 2,
                        max_degree=int(deg.max()), n_core0=7)
    capped = kc.summary(V, s, d, max_k=4)
    assert capped["degeneracy"] == 4 and capped["main_core_size"] == int((core >= 4).sum()) and capped["levels"] == 5
    assert kc.summary(V, s, d, max_k=0)["levels"] == 1 and kc.summary(V, s, d, max_k=0)["main_core_size"] == V
    assert kc.summary(*CASES["empty"]()) == dict.fromkeys(kc.PURE_KEYS, 0)


# ---- invariants ----
INVARIANT_CASES = ("two_cliques", "r9", "degree_mix", "rm2000", "overshoot", "clique_chain")


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_max_k_is_a_cap(name):
    V, s, d, core, deg = _both(name)
    top = int(core.max())
    for max_k in (0, 1, 3, top, top + 5):
        for fn in (kc.core_numbers, kc.core_numbers_literal) if name != "rm2000" else (kc.core_numbers,):
            got, gdeg = fn(V, s, d, max_k=max_k)
            assert np.array_equal(got, np.minimum(core, max_k)) and np.array_equal(gdeg, deg)


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_invariances(name):
    V, s, d, core, deg = _both(name)
    rng = np.random.default_rng(5)
    order = rng.permutation(s.size)
    assert np.array_equal(kc.core_numbers(V, s[order], d[order])[0], core)
    assert np.array_equal(kc.core_numbers(V, d, s)[0], core)
    assert np.array_equal(kc.core_numbers(V, np.concatenate([s, s, d]), np.concatenate([d, d, s]))[0], core)
    loops = rng.integers(0, V, size=50)
    assert np.array_equal(kc.core_numbers(V, np.concatenate([s, loops]), np.concatenate([d, loops]))[0], core)
    perm = rng.permutation(V)
    pcore, pdeg = kc.core_numbers(V, perm[s], perm[d])
    assert np.array_equal(pcore[perm], core) and np.array_equal(pdeg[perm], deg)


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_k_core_property(name):
    """In the subgraph induced by core >= k every vertex has at least k neighbours, for every k; and the
    (k + 1)-core is maximal: no vertex of core k keeps k + 1 neighbours among core >= k ... that are
    themselves enough to survive, which the peel and the fixpoint agreeing already says."""
    V, s, d, core, deg = _both(name)
    off, col, _ = kc.simple_graph(V, s, d)
    row = np.repeat(np.arange(V), np.diff(off))
    for k in range(int(core.max()) + 1):
        inside = core >= k
        both = inside[row] & inside[col]
        inner = np.bincount(row[both], minlength=V)
        assert (inner[inside] >= k).all(), f"a vertex of the {k}-core has fewer than {k} neighbours in it"
