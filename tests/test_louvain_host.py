"""Louvain, the part that needs no GPU: the C-ABI boundary of lpa_louvain, the exported names,
the argument checks of GraphFrame.louvain and Graph.louvain (they run before any device work),
and the two CPU restatements of tests/louvain_ref.py (vectorised; literal) checked against each
other, against the closed forms of the specification and against the quality the detector is
there for."""
import ctypes
import functools
import os

import numpy as np
import pandas as pd
import pytest

import louvain_ref as lv
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph, star, two_cliques


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_louvain(None, 64, 1000, None, 0, None, None, 0, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_louvain():
    assert _lib.load().lpa_abi_version() >= 14


def test_struct_layouts():
    row = _lib.LpaLouvainLevel(1, 2, 3, 4, 5, 6)
    assert row.to_dict() == dict(vertices=1, communities=2, rounds=3, damped_rounds=4, moves=5, numerator=6)
    assert tuple(row.to_dict()) == lv.LEVEL_KEYS
    assert ctypes.sizeof(_lib.LpaLouvainLevel) == 48
    s = _lib.LpaLouvainSummary(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0.5)
    assert tuple(s.to_dict()) == lv.SUMMARY_KEYS
    assert list(s.to_dict().values()) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0.5]
    assert ctypes.sizeof(_lib.LpaLouvainSummary) == 96


def test_exported():
    assert "louvain" in gfa.__all__
    assert callable(gfa.louvain) and callable(gfa.GraphFrame.louvain) and callable(gfa.Graph.louvain)


# ---- argument checks: none of them reaches the device ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": np.array([30, 10, 20], np.int64), "name": ["c", "a", "b"]})
    e = pd.DataFrame({"src": np.array([10, 20], np.int64), "dst": np.array([20, 30], np.int64)})
    f = gfa.GraphFrame(v, e)
    yield f
    assert f._graph is None   # no handle was ever built


@pytest.mark.parametrize("bad", [0, -3])
def test_bounds_must_be_positive(gf, bad):
    for kw, name in (("maxLevels", "maxLevels"), ("maxRounds", "maxRounds")):
        with pytest.raises(ValueError, match=f"{name} must be greater than 0, but got {bad}"):
            gf.louvain(**{kw: bad})
        with pytest.raises(ValueError, match=f"{name} must be greater than 0"):
            gfa.louvain(gf.vertices, gf.edges, **{kw: bad})
    with pytest.raises(ValueError, match="max_levels must be greater than 0"):
        gfa.Graph.louvain(None, bad)
    with pytest.raises(ValueError, match="max_rounds must be greater than 0"):
        gfa.Graph.louvain(None, 3, bad)


@pytest.mark.parametrize("bad", [2.5, True, "3", None, np.float64(4), np.bool_(True)])
def test_bounds_must_be_ints(gf, bad):
    with pytest.raises(TypeError, match="maxLevels"):
        gf.louvain(bad)
    with pytest.raises(TypeError, match="maxRounds"):
        gf.louvain(3, bad)
    with pytest.raises(TypeError, match="maxRounds"):
        gfa.louvain(gf.vertices, gf.edges, maxRounds=bad)
    with pytest.raises(TypeError, match="max_levels"):
        gfa.Graph.louvain(None, bad)
    with pytest.raises(TypeError, match="max_rounds"):
        gfa.Graph.louvain(None, 3, bad)


def test_reference_checks_its_bounds():
    for fn in (lv.louvain, lv.louvain_literal):
        with pytest.raises(ValueError):
            fn(2, [0], [1], max_levels=0)
        with pytest.raises(ValueError):
            fn(2, [0], [1], max_rounds=0)


# ---- the two reference forms ----
def _rows(levels):
    return [(r["rounds"], r["moves"], r["communities"]) for r in levels]


def _check_result(V, s, d, comm, levels, summ):
    """What any result must satisfy, recomputed from comm in plain numpy."""
    assert comm.dtype == np.int32 and comm.shape == (V,)
    assert np.array_equal(comm[comm], comm) and (comm <= np.arange(V)).all()
    numer, intra, arcs, ncomm = lv.modularity_np(V, s, d, comm)
    assert (summ["numerator"], summ["intra_arcs"], summ["arcs"], summ["n_communities"]) == (numer, intra, arcs, ncomm)
    assert summ["modularity"] == (numer / (float(arcs) * float(arcs)) if arcs else 0.0)
    sizes = np.bincount(comm, minlength=V) if V else np.zeros(0, np.int64)
    assert summ["n_singletons"] == int((sizes == 1).sum())
    assert summ["largest_size"] == (int(sizes.max()) if V else 0)
    assert summ["largest_id"] == (int(np.argmax(sizes)) if V else -1)
    assert summ["levels"] == len(levels)
    for key in ("rounds", "damped_rounds", "moves"):
        assert summ[key] == sum(r[key] for r in levels)
    if levels:
        assert levels[0]["vertices"] == V and levels[-1]["communities"] == ncomm
        assert levels[-1]["numerator"] == numer
        for a, b in zip(levels, levels[1:]):
            assert b["vertices"] == a["communities"] and b["numerator"] > a["numerator"]
    for r in levels:
        assert r["moves"] >= r["rounds"] - 1 >= 0 and r["communities"] < r["vertices"]
        assert 0 <= r["damped_rounds"] <= r["rounds"]


@functools.lru_cache(maxsize=None)
def _both_cached(name):
    V, s, d = CASES[name]()
    got = lv.louvain(V, s, d)
    lit = lv.louvain_literal(V, s, d)
    assert np.array_equal(got[0], lit[0]) and got[1] == lit[1] and got[2] == lit[2]
    _check_result(V, np.asarray(s), np.asarray(d), *got)
    return (V, s, d) + got


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r9_golden.npz")


def _r9():
    z = np.load(GOLDEN, allow_pickle=False)
    return int(z["ids"].size), z["src"], z["dst"]


CASES = {
    "edge": lambda: (2, np.array([0], np.int32), np.array([1], np.int32)),
    "path4": lambda: lv.path(4),
    "two_cliques": lambda: two_cliques(5),
    "star5000": lambda: star(5000),
    "ring": lambda: lv.ring_of_cliques(30, 5),
    "path200": lambda: lv.path(200),
    "cycle1000": lambda: lv.cycle(1000),
    "r9": _r9,
    "degree_mix": degree_mix,
    "rm300": lambda: random_multigraph(300, 2000, 1),
    "rm2000": lambda: random_multigraph(2000, 60000, 7),
    "loops": lambda: (4, np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32)),
    "edgeless": lambda: (70, np.empty(0, np.int32), np.empty(0, np.int32)),
    "empty": lambda: (0, np.empty(0, np.int32), np.empty(0, np.int32)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_agree(name):
    _both_cached(name)


def test_closed_forms():
    """The rows of the specification's table."""
    _, _, _, comm, levels, summ = _both_cached("edge")
    assert comm.tolist() == [0, 0] and _rows(levels) == [(1, 1, 1)]
    _, _, _, comm, levels, summ = _both_cached("path4")
    assert comm.tolist() == [0, 0, 2, 2] and _rows(levels) == [(1, 2, 2)]
    _, _, _, comm, levels, summ = _both_cached("two_cliques")
    assert comm.tolist() == [0] * 5 + [5] * 6 and _rows(levels) == [(2, 9, 2)]
    V, _, _, comm, levels, summ = _both_cached("star5000")
    assert (comm == 0).all() and summ["numerator"] == 0 and summ["modularity"] == 0.0
    assert _rows(levels) == [(1, V - 1, 1)] and V - 1 == 5000
    _, _, _, comm, levels, summ = _both_cached("ring")
    assert np.array_equal(comm, 5 * (np.arange(150) // 5)) and _rows(levels) == [(2, 120, 30)]
    assert round(summ["modularity"], 6) == 0.875758
    _, _, _, comm, levels, summ = _both_cached("path200")
    assert summ["n_communities"] == 13
    assert _rows(levels) == [(99, 9802, 100), (49, 2402, 50), (24, 577, 25), (11, 133, 13)]
    _, _, _, comm, levels, summ = _both_cached("cycle1000")
    assert summ["n_communities"] == 31 and _rows(levels)[0] == (500, 249999, 500)
    _, _, _, comm, levels, summ = _both_cached("r9")
    assert summ["n_communities"] == 123 and [r["rounds"] for r in levels] == [12, 9, 2]
    assert abs(summ["modularity"] - 0.8261) < 5e-5


@pytest.mark.parametrize("name", ["loops", "edgeless", "empty"])
def test_nothing_to_move_is_the_identity(name):
    V, _, _, comm, levels, summ = _both_cached(name)
    assert np.array_equal(comm, np.arange(V)) and levels == [] and summ["levels"] == 0
    assert summ["n_communities"] == V and summ["largest_id"] == (0 if V else -1)
    if name != "loops":
        assert summ["arcs"] == 0 and summ["modularity"] == 0.0


@pytest.mark.parametrize("name", ["r9", "path200", "rm300"])
def test_max_levels_prefixes(name):
    V, s, d, comm, levels, summ = _both_cached(name)
    assert len(levels) >= 3
    trace = []
    lv.louvain(V, s, d, trace=trace)
    assert len(trace) == len(levels)
    for cut in range(1, len(levels) + 2):
        c2, l2, s2 = lv.louvain(V, s, d, max_levels=cut)
        assert l2 == levels[:cut] and s2["levels"] == min(cut, len(levels))
        tc, tl, ts = trace[min(cut, len(levels)) - 1]
        assert np.array_equal(c2, tc) and l2 == tl and s2 == ts
        _check_result(V, s, d, c2, l2, s2)
        if cut >= len(levels):
            assert np.array_equal(c2, comm) and s2 == summ
        else:
            assert s2["n_communities"] == levels[cut - 1]["communities"]
            assert np.array_equal(comm[c2], comm)      # a coarser partition of the same hierarchy


def test_max_rounds_one_on_the_path():
    """The one-round state.  Every interior vertex ties between its two singleton neighbours and
    takes the smaller; 0 and 198 prefer an end of degree 1 with a larger id and are blocked by the
    singleton rule; 199 joins 198.  The 198 proposals are a chain of shifts c[u] = u - 1: vertex 1
    joins 0, every u in 2 .. 197 sits alone in community u - 1, 197 is left empty.  I = 4 ordered
    arcs, D = 3, 3 and 196 twos: N = 398 x 4 - 802 = 790 > -794, accepted."""
    V, s, d = lv.path(200)
    want = np.arange(V)
    want[1], want[199] = 0, 198
    for fn in (lv.louvain, lv.louvain_literal):
        comm, levels, summ = fn(V, s, d, max_levels=1, max_rounds=1)
        assert np.array_equal(comm, want)
        assert levels == [dict(vertices=200, communities=198, rounds=1, damped_rounds=0, moves=198, numerator=790)]
        assert summ["intra_arcs"] == 4 and summ["n_singletons"] == 196
    # max_rounds bounds every level's phase: one round a level from there on
    comm, levels, summ = lv.louvain(V, s, d, max_levels=5, max_rounds=1)
    assert [r["rounds"] for r in levels] == [1] * 5 and summ["rounds"] == 5
    assert levels == lv.louvain_literal(V, s, d, max_levels=5, max_rounds=1)[1]


def test_edge_order_and_direction_do_not_matter():
    V, s, d, comm, levels, summ = _both_cached("rm300")
    perm = np.random.default_rng(5).permutation(s.size)
    for s2, d2 in ((s[perm], d[perm]), (d, s), (s[::-1], d[::-1])):
        c2, l2, m2 = lv.louvain(V, s2, d2)
        assert np.array_equal(c2, comm) and l2 == levels and m2 == summ


def test_dropped_edges_are_not_edges():
    V, s, d = two_cliques(5)
    s2 = np.concatenate([s, [3, -1, V]]).astype(np.int32)
    d2 = np.concatenate([d, [V, 2, 0]]).astype(np.int32)
    a, b = lv.louvain(V, s, d), lv.louvain(V, s2, d2)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


# ---- quality: what the detector is for ----
def test_r9_beats_every_golden_lpa_superstep(golden):
    V, s, d, comm, levels, summ = _both_cached("r9")
    for lab in golden["labels_iter"]:
        numer, _, arcs, _ = lv.modularity_np(V, s, d, lab)
        assert summ["modularity"] > numer / float(arcs) ** 2
    assert summ["modularity"] > 0.8


def test_planted_partition_is_recovered():
    V, s, d, block = lv.planted(V=2000, blocks=20, m=30000, p_in=0.8, seed=11)
    comm, levels, summ = lv.louvain(V, s, d)
    assert summ["n_communities"] == 20 == np.unique(block).size
    assert len(set(zip(comm.tolist(), block.tolist()))) == 20   # a bijection of communities and blocks


def test_r9_close_to_networkx_louvain():
    nx = pytest.importorskip("networkx")
    V, s, d, comm, levels, summ = _both_cached("r9")
    G = nx.MultiGraph()
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(s.tolist(), d.tolist()))
    best = max(nx.community.modularity(G, nx.community.louvain_communities(G, seed=seed)) for seed in range(3))
    print(f"louvain {summ['modularity']:.4f} networkx best of 3 {best:.4f}")
    assert summ["modularity"] >= 0.95 * best
