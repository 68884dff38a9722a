"""Breadth-first search on the GPU (lpa_bfs, csrc/lpa_bfs.hip) against the CPU references of
tests/bfs_ref.py: exact integer equality of the length, every level, every marked edge and every
summary field that does not depend on the schedule; push_levels + pull_levels against the
reference's level count; on the small cases the path set against the literal join loop.  The same
result under the push-only and pull-only overrides, across calls, handles and edge orders.
Drop-in calls: GraphFrame.bfs, bfs."""
import numpy as np
import pandas as pd
import pytest

import bfs_ref
from bfs_ref import one_hot
from graphs import degree_mix, random_multigraph

pytestmark = pytest.mark.gpu

# the create-time overrides of the push / pull switch (DESIGN.md "Breadth-first search")
BFS_OVERRIDES = [{}, {"LPA_BFS_ALPHA": "0"}, {"LPA_BFS_PULL": "1"}]
BFS_IDS = ["defaults", "push-only", "pull-only"]


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _compare(got, V, s, d, F, T, keep=None, max_len=10, ref=None, literal=False):
    """One stats=True result against levels_dag (and the literal join loop); returns the reference."""
    length, level, eidx, summ = got
    if ref is None:
        ref = bfs_ref.levels_dag(V, s, d, F, T, keep, max_len)
    print(f"V={V} m={len(s)} max_len={max_len} summary={summ} levels={ref['levels']}")
    assert length == ref["length"] == summ["length"]
    assert level.dtype == np.int32 and level.shape == (V,)
    assert np.array_equal(level, ref["level"]), f"{int((level != ref['level']).sum())} of {V} levels differ"
    assert eidx.dtype == np.int64 and np.array_equal(eidx, np.flatnonzero(ref["on_edge"]))
    for key, val in ref["summary"].items():
        assert summ[key] == val, key
    assert summ["push_levels"] >= 0 and summ["pull_levels"] >= 0
    assert summ["push_levels"] + summ["pull_levels"] == ref["levels"]
    if literal:
        import graphframes_amd as gfa

        want_len, want = bfs_ref.literal(V, s, d, F, T, keep, max_len)
        assert length == want_len
        if length > 0:
            verts, edges = gfa.enumerate_paths(level, s, d, eidx, length)
            assert bfs_ref.path_tuples(verts, edges) == sorted(want, key=lambda p: p[1::2])
        elif length == 0:
            assert [(int(v),) for v in np.flatnonzero(level == 0)] == want
    return ref


def _check(gfa, V, s, d, F, T, keep=None, max_len=10, g=None, ref=None, literal=False):
    """bfs() plain and with stats (of a fresh handle unless g is given) against the references."""
    s = np.asarray(s, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    own = g is None
    if own:
        g = gfa.Graph(s, d, V)
    try:
        plain = g.bfs(F, T, keep, max_len)
        got = g.bfs(F, T, keep, max_len, stats=True)
    finally:
        if own:
            g.close()
    assert plain[0] == got[0] and np.array_equal(plain[1], got[1]) and np.array_equal(plain[2], got[2])
    _compare(got, V, s, d, F, T, keep, max_len, ref, literal)
    return got


def _with_env(gfa, monkeypatch, env, V, s, d):
    """A handle created under the overrides (they are read when the handle is created)."""
    with monkeypatch.context() as mp:
        for key, val in env.items():
            mp.setenv(key, val)
        return gfa.Graph(np.asarray(s, np.int32), np.asarray(d, np.int32), V)


# ---- 1. degenerate ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    none = np.empty(0, bool)
    with gfa.Graph(e, e, 0) as g:
        length, level, eidx, summ = g.bfs(none, none, stats=True)
    assert length == -1 and level.shape == (0,) and eidx.shape == (0,)
    assert summ == dict(arcs=0, sources=0, targets=0, length=-1, reached=0, path_vertices=0, path_edges=0,
                        push_levels=0, pull_levels=0)


def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    yes, no = np.ones(1, bool), np.zeros(1, bool)
    assert _check(gfa, 1, e, e, yes, yes, literal=True)[0] == 0
    assert _check(gfa, 1, e, e, yes, no, literal=True)[0] == -1
    loop = np.zeros(3, np.int32)
    assert _check(gfa, 1, loop, loop, yes, yes, literal=True)[0] == 0


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    length, level, eidx, summ = _check(gfa, 70, e, e, one_hot(70, 0, 64), one_hot(70, 69), literal=True)
    assert length == -1 and summ["arcs"] == 0 and summ["reached"] == 2


def test_only_self_loops(gfa):
    v = np.array([3, 3, 0, 99, 64, 64, 64], np.int32)
    length, _, eidx, summ = _check(gfa, 100, v, v, one_hot(100, 3, 64), one_hot(100, 0, 99), literal=True)
    assert length == -1 and summ["arcs"] == 0 and eidx.size == 0


def test_empty_sets_shared_vertices_and_zero_length(gfa):
    V, s, d = random_multigraph(100, 400, 2)
    none = np.zeros(V, bool)
    some, other = one_hot(V, 5, 70), one_hot(V, 70, 71, 99)
    with gfa.Graph(s, d, V) as g:
        for F, T in ((none, some), (some, none), (none, none)):
            length, level, eidx, summ = _check(gfa, V, s, d, F, T, g=g, literal=True)
            assert length == -1 and (level == -1).all() and eidx.size == 0 and summ["reached"] == 0
            assert 0 < summ["arcs"] <= 400
        length, level, eidx, summ = _check(gfa, V, s, d, some, other, g=g, literal=True)
        assert length == 0 and np.flatnonzero(level == 0).tolist() == [70] and eidx.size == 0
        assert summ["path_vertices"] == 1 and summ["reached"] == 2 and summ["push_levels"] + summ["pull_levels"] == 0
        # max_len = 0 can only give 0 or -1
        assert _check(gfa, V, s, d, some, other, max_len=0, g=g, literal=True)[0] == 0
        length, level, _, summ = _check(gfa, V, s, d, one_hot(V, 5), one_hot(V, 71), max_len=0, g=g, literal=True)
        assert length == -1 and (level == -1).all() and summ["reached"] == 1
        keep = np.ones(s.size, bool)
        lib, u8 = g._lib, gfa._lib._u8p
        lv, on = np.empty(V, np.int32), np.empty(s.size, np.uint8)
        args = [some.view(np.uint8).ctypes.data_as(u8), other.view(np.uint8).ctypes.data_as(u8),
                keep.view(np.uint8).ctypes.data_as(u8), 3, lv.ctypes.data_as(gfa._lib._i32p), on.ctypes.data_as(u8), None]
        assert lib.lpa_bfs(g._handle(), *args) == gfa._lib.LPA_OK   # a null summary
        assert np.flatnonzero(lv == 0).tolist() == [70] and not on.any()
        for i, val in ((0, None), (1, None), (4, None), (5, None), (3, -1)):   # the C ABI's own argument checks
            bad = list(args)
            bad[i] = val
            assert lib.lpa_bfs(g._handle(), *bad) == gfa._lib.LPA_EINVAL


# ---- 2. bitmap word edges ----
@pytest.mark.parametrize("env", BFS_OVERRIDES[1:], ids=BFS_IDS[1:])
@pytest.mark.parametrize("V", [63, 64, 65, 129])
def test_directed_path_across_words(gfa, monkeypatch, V, env):
    _, s, d = bfs_ref.path(V)
    F, T = one_hot(V, 0), one_hot(V, V - 1)
    g = _with_env(gfa, monkeypatch, env, V, s, d)
    try:
        length, level, eidx, summ = _check(gfa, V, s, d, F, T, max_len=V - 1, g=g)
        assert length == V - 1 and np.array_equal(level, np.arange(V)) and eidx.size == V - 1
        assert summ[("pull" if "LPA_BFS_ALPHA" in env else "push") + "_levels"] == 0
        length, level, eidx, summ = _check(gfa, V, s, d, F, T, max_len=V - 2, g=g)
        assert length == -1 and (level == -1).all() and eidx.size == 0 and summ["reached"] == V - 1
    finally:
        g.close()


# ---- 3. row forms ----
@pytest.mark.parametrize("k", [32, 33, 1024, 1025, 3000])
def test_row_forms(gfa, monkeypatch, k):
    """A source with k distinct out-arcs (the push's short / wave / block lists) and, mirrored, a
    target with k in-arcs (the pull's); the next hop hangs behind exactly one of the arcs."""
    for behind in (0, k // 2, k - 1):
        V, s, d, t = bfs_ref.fan(k, behind)
        for fwd in (True, False):
            a, b, F, T = (s, d, one_hot(V, 0), one_hot(V, t)) if fwd else (d, s, one_hot(V, t), one_hot(V, 0))
            ref = bfs_ref.levels_dag(V, a, b, F, T)
            assert ref["length"] == 2 and ref["summary"]["path_edges"] == 2
            for env in BFS_OVERRIDES:
                g = _with_env(gfa, monkeypatch, env, V, a, b)
                try:
                    got = g.bfs(F, T, stats=True)
                finally:
                    g.close()
                _compare(got, V, a, b, F, T, ref=ref)
                assert np.flatnonzero(got[1] >= 0).tolist() == sorted([0, 1 + behind, t])


# ---- 4. schedule independence ----
def _far_case(V, s, d, source):
    """F = one vertex, T = the (at most three) smallest vertices at the largest finite distance."""
    F = one_hot(V, source)
    dist = bfs_ref.distances(V, s, d, F)
    far = np.flatnonzero(dist == dist.max())[:3]
    assert dist.max() >= 3
    return F, one_hot(V, *far)


@pytest.fixture(scope="module")
def rnd():
    V, s, d = random_multigraph(2000, 16000, 7)
    F, T = _far_case(V, s, d, int(s[0]))
    ref = bfs_ref.levels_dag(V, s, d, F, T)
    for a in (ref["level"], ref["on_edge"]):
        a.setflags(write=False)
    return V, s, d, F, T, ref


@pytest.fixture(scope="module")
def mix():
    V, s, d = degree_mix()
    F, T = _far_case(V, s, d, int(s[0]))    # s[0] is a hub: a block row in the first push
    ref = bfs_ref.levels_dag(V, s, d, F, T)
    for a in (ref["level"], ref["on_edge"]):
        a.setflags(write=False)
    return V, s, d, F, T, ref


def _under_overrides(gfa, monkeypatch, V, s, d, F, T, ref):
    got = []
    for env in BFS_OVERRIDES:
        g = _with_env(gfa, monkeypatch, env, V, s, d)
        try:
            got.append(g.bfs(F, T, stats=True))
        finally:
            g.close()
    for res in got:
        _compare(res, V, s, d, F, T, ref=ref)
    (_, _, _, dflt), (_, _, _, push), (_, _, _, pull) = got
    assert push["pull_levels"] == 0 and pull["push_levels"] == 0
    assert dflt["push_levels"] + dflt["pull_levels"] == ref["length"]


def test_schedules_agree_on_random_multigraph(gfa, monkeypatch, rnd):
    _under_overrides(gfa, monkeypatch, *rnd)


def test_schedules_agree_on_degree_mix(gfa, monkeypatch, mix):
    _under_overrides(gfa, monkeypatch, *mix)


@pytest.mark.parametrize("which", ["rnd", "mix"])
def test_calls_handles_and_edge_order(gfa, request, which):
    V, s, d, F, T, ref = request.getfixturevalue(which)
    with gfa.Graph(s, d, V) as g:
        a = g.bfs(F, T, stats=True)
        b = g.bfs(F, T, stats=True)
    with gfa.Graph(s, d, V) as g:
        c = g.bfs(F, T, stats=True)
    for res in (a, b, c):
        _compare(res, V, s, d, F, T, ref=ref)
    assert a[3] == b[3] == c[3]
    perm = np.random.default_rng(9).permutation(s.size)
    with gfa.Graph(s[perm], d[perm], V) as g:
        length, level, eidx, summ = g.bfs(F, T, stats=True)
    assert length == ref["length"] and np.array_equal(level, ref["level"])
    assert np.array_equal(np.sort(perm[eidx]), np.flatnonzero(ref["on_edge"]))   # on_edge follows its edges
    assert {k: summ[k] for k in ref["summary"]} == ref["summary"]


def test_does_not_disturb_lpa(gfa, mix):
    V, s, d, F, T, ref = mix
    with gfa.Graph(s, d, V) as g:
        want = g.run(5)
        before = g.info()["device_bytes"]
        _compare(g.bfs(F, T, stats=True), V, s, d, F, T, ref=ref)
        assert g.info()["device_bytes"] == before
        assert np.array_equal(g.labels(), want) and np.array_equal(g.run(5), want)


def test_two_loopback_ranks(gfa, rnd):
    V, s, d, F, T, ref = rnd
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        _compare(ranks[0].bfs(F, T, stats=True), V, s, d, F, T, ref=ref)
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].bfs(F, T)
    finally:
        for g in ranks:
            g.close()
        lb.close()


# ---- 5. sets ----
def test_source_and_target_sets(gfa):
    """0 -> 2 -> 4 and 1 -> 3 -> 5 -> 8, 4 -> 6 -> 7, 0 -> 3: from {0, 1} the targets 4 and 5 are
    both two edges away (paths from more than one pair), 7 and 8 farther."""
    s = np.array([0, 2, 1, 3, 4, 6, 0, 5], np.int32)
    d = np.array([2, 4, 3, 5, 6, 7, 3, 8], np.int32)
    V = 9
    F = one_hot(V, 0, 1)
    length, level, eidx, _ = _check(gfa, V, s, d, F, one_hot(V, 4, 5, 7, 8), literal=True)
    assert length == 2 and eidx.tolist() == [0, 1, 2, 3, 6] and level.tolist() == [0, 0, 1, 1, 2, 2, -1, -1, -1]
    # a nearer target shadows the farther ones
    length, level, eidx, _ = _check(gfa, V, s, d, F, one_hot(V, 2, 4, 5, 7), literal=True)
    assert length == 1 and eidx.tolist() == [0] and np.flatnonzero(level >= 0).tolist() == [0, 2]
    # uint8 masks: any nonzero byte is a member
    F8, T8 = np.array([0x80, 7, 0, 0, 0, 0, 0, 0, 0], np.uint8), np.array([0, 0, 0, 0, 255, 1, 0, 2, 0x40], np.uint8)
    length, level, eidx, summ = _check(gfa, V, s, d, F8, T8, literal=True)
    assert length == 2 and eidx.tolist() == [0, 1, 2, 3, 6] and summ["sources"] == 2 and summ["targets"] == 4
    # a target at level L that is reached, and a vertex at level L that is no target
    length, level, eidx, _ = _check(gfa, V, s, d, F, one_hot(V, 5), literal=True)
    assert length == 2 and eidx.tolist() == [2, 3, 6] and level[4] == -1 and level[2] == -1


# ---- 6. edge filter ----
def test_edge_filter(gfa):
    """0 -> 1 -> 3 and 0 -> 2 -> 4 -> 3."""
    s = np.array([0, 1, 0, 2, 4], np.int32)
    d = np.array([1, 3, 2, 4, 3], np.int32)
    V, F, T = 5, one_hot(5, 0), one_hot(5, 3)
    with gfa.Graph(s, d, V) as g:
        assert _check(gfa, V, s, d, F, T, g=g, literal=True)[2].tolist() == [0, 1]
        keep = np.array([1, 0, 1, 1, 1], np.uint8)     # the only shortest path goes: L grows
        length, _, eidx, summ = _check(gfa, V, s, d, F, T, keep, g=g, literal=True)
        assert length == 3 and eidx.tolist() == [2, 3, 4] and summ["arcs"] == 4
        keep = np.array([True, False, True, True, False])   # every path goes
        length, _, eidx, summ = _check(gfa, V, s, d, F, T, keep, g=g, literal=True)
        assert length == -1 and eidx.size == 0 and summ["reached"] == 4
        length, _, _, summ = _check(gfa, V, s, d, F, T, np.zeros(5, bool), g=g, literal=True)
        assert length == -1 and summ["arcs"] == 0 and summ["reached"] == 1
        assert _check(gfa, V, s, d, F, T, np.ones(5, bool), g=g, literal=True)[0] == 2


def test_edge_filter_on_random_multigraph(gfa, rnd):
    V, s, d, F, T, ref = rnd
    keep = np.random.default_rng(3).random(s.size) < 0.6
    got = _check(gfa, V, s, d, F, T, keep, max_len=20)
    assert got[3]["arcs"] < ref["summary"]["arcs"] and (got[0] == -1 or got[0] >= ref["length"])


# ---- 7. path multiplicity ----
def test_duplicates_and_self_loops(gfa, rnd):
    V, s, d, F, T, ref = rnd
    s2 = np.concatenate([s, s[:50], np.arange(9, dtype=np.int32)])
    d2 = np.concatenate([d, d[:50], np.arange(9, dtype=np.int32)])
    with gfa.Graph(s2, d2, V) as g:
        length, level, eidx, summ = _check(gfa, V, s2, d2, F, T, g=g)
        # the levels and the marks of the first copies are the plain graph's; no loop is marked
        assert length == ref["length"] and np.array_equal(level, ref["level"])
        assert np.array_equal(eidx[eidx < s.size], np.flatnonzero(ref["on_edge"]))
        twins = eidx[eidx >= s.size] - s.size
        assert (twins < 50).all() and np.array_equal(twins, np.flatnonzero(ref["on_edge"][:50]))
        assert summ["arcs"] == ref["summary"]["arcs"]
        # edge 0 alone joins its ends in the plain graph: its twin doubles the paths through it
        a, b = int(s[0]), int(d[0])
        assert a != b and int(((s == a) & (d == b)).sum()) == 1
        one = _check(gfa, V, s2, d2, one_hot(V, a), one_hot(V, b), g=g, literal=True)
        assert one[0] == 1 and one[2].tolist() == [0, s.size]
        assert gfa.count_paths(one[1], s2, d2, one[2], 1) == 2
    n_plain = gfa.count_paths(ref["level"], s, d, np.flatnonzero(ref["on_edge"]), ref["length"])
    assert gfa.count_paths(level, s2, d2, eidx, length) >= n_plain


def _lattice_frames():
    V, s, d = bfs_ref.lattice(4, 3)
    v = pd.DataFrame({"id": np.arange(V, dtype=np.int64), "layer": np.arange(V) // 3})
    e = pd.DataFrame({"src": s.astype(np.int64), "dst": d.astype(np.int64), "n": np.arange(s.size)})
    return v, e


def test_lattice_gives_27_rows(gfa):
    v, e = _lattice_frames()
    out = gfa.bfs(v, e, "id == 0", "layer == 3")
    assert len(out) == 27 and out.attrs == {"length": 3, "paths": 27}
    assert list(out.columns.get_level_values(0).unique()) == ["from", "e0", "v1", "e1", "v2", "e2", "to"]
    assert (out["from"]["id"] == 0).all() and sorted(set(out["to"]["id"])) == [9, 10, 11]
    assert out["v1"]["layer"].eq(1).all() and out["v2"]["layer"].eq(2).all()
    rows = list(zip(out["e0"]["n"], out["e1"]["n"], out["e2"]["n"]))
    assert rows == sorted(rows) and len(set(rows)) == 27
    with pytest.raises(ValueError, match="27 paths"):
        gfa.bfs(v, e, "id == 0", "layer == 3", maxPaths=26)
    assert len(gfa.bfs(v, e, "id == 0", "layer == 3", maxPaths=27)) == 27
    assert len(gfa.bfs(v, e, "layer == 0", "id == 11")) == 27
    assert len(gfa.bfs(v, e, "id == 0", "layer == 3", maxPathLength=2)) == 0


# ---- 8. drop-in ----
def test_graphframe_string_ids(gfa):
    """a -> b -> d, a -> c -> d twice, d -> e, a self-loop at a, and a dangling b -> zz in the
    middle of the edge rows (the rows after it keep their row numbers)."""
    v = pd.DataFrame({"id": ["d", "a", "c", "b", "e"], "age": [4, 1, 3, 2, 5]})
    e = pd.DataFrame({"src": ["a", "a", "b", "a", "b", "c", "c", "d"],
                      "dst": ["a", "b", "zz", "c", "d", "d", "d", "e"],
                      "rel": ["loop", "x", "gone", "y", "x", "y", "y2", "x"]})
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.bfs("id == 'a'", "id == 'd'")
        far = gf.bfs("id == 'a'", "age >= 4", edgeFilter="rel != 'y2'", maxPathLength=2)
        only_x = gf.bfs("id == 'a'", "id == 'e'", edgeFilter=lambda df: df["rel"] == "x")
        short = gf.bfs("id == 'a'", "id == 'e'", maxPathLength=2)
        by_array = gf.bfs(v["age"].to_numpy() == 1, v["id"] == "d")
    finally:
        gf.close()
    assert out.columns.tolist() == [("from", "id"), ("from", "age"), ("e0", "src"), ("e0", "dst"), ("e0", "rel"),
                                    ("v1", "id"), ("v1", "age"), ("e1", "src"), ("e1", "dst"), ("e1", "rel"),
                                    ("to", "id"), ("to", "age")]
    assert out.attrs == {"length": 2, "paths": 3}
    # rows sorted by the input-edge row numbers (1, 4), (3, 5), (3, 6)
    assert out["e0"]["rel"].tolist() == ["x", "y", "y"] and out["e1"]["rel"].tolist() == ["x", "y", "y2"]
    assert out["v1"]["id"].tolist() == ["b", "c", "c"] and out["v1"]["age"].tolist() == [2, 3, 3]
    assert out["from"]["age"].tolist() == [1, 1, 1] and out["to"]["id"].tolist() == ["d", "d", "d"]
    assert out["e1"]["src"].tolist() == out["v1"]["id"].tolist()
    assert far["e1"]["rel"].tolist() == ["x", "y"] and far.attrs == {"length": 2, "paths": 2}
    assert only_x.attrs == {"length": 3, "paths": 1} and only_x["v2"]["id"].tolist() == ["d"]
    assert only_x.columns.get_level_values(0).unique().tolist() == ["from", "e0", "v1", "e1", "v2", "e2", "to"]
    assert len(short) == 0 and list(short.columns) == ["id", "age"] and short.attrs == {"length": -1, "paths": 0}
    assert by_array.equals(out)
    assert out.equals(gfa.bfs(v, e, "id == 'a'", "id == 'd'"))


def test_graphframe_integral_ids(gfa):
    """10 -> 20 -> 30 -> 10, 40 -> 10, 50 alone, and a dangling 40 -> 99."""
    v = pd.DataFrame({"id": np.array([30, 10, 50, 20, 40], np.int64), "name": ["c", "a", "e", "b", "d"]})
    e = pd.DataFrame({"src": np.array([10, 20, 40, 30, 40], np.int64), "dst": np.array([20, 30, 99, 10, 10], np.int64)})
    out = gfa.bfs(v, e, "id == 40", "name == 'c'")
    assert out.attrs == {"length": 3, "paths": 1}
    assert [out[k]["id"].item() for k in ("from", "v1", "v2", "to")] == [40, 10, 20, 30]
    assert [out[k]["name"].item() for k in ("from", "v1", "v2", "to")] == ["d", "a", "b", "c"]
    assert [(out[k]["src"].item(), out[k]["dst"].item()) for k in ("e0", "e1", "e2")] == [(40, 10), (10, 20), (20, 30)]
    assert len(gfa.bfs(v, e, "id == 10", "id == 50")) == 0
    assert len(gfa.bfs(v, e, "id == 10", "id == 40")) == 0        # 40 has no in-edge


def test_sample_graph_path_between_two_domains(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    V = ig.num_vertices
    source = int(np.argmax(np.bincount(ig.src, minlength=V)))
    dist = bfs_ref.distances(V, ig.src, ig.dst, one_hot(V, source))
    target = int(np.flatnonzero(dist == dist.max())[0])
    assert dist.max() >= 2
    ref = bfs_ref.levels_dag(V, ig.src, ig.dst, one_hot(V, source), one_hot(V, target))
    a, b = str(ig.ids[source]), str(ig.ids[target])
    out = gfa.bfs(v, e, f"id == '{a}'", f"id == '{b}'")
    L = ref["length"]
    assert out.attrs["length"] == L == int(dist.max())
    eidx = np.flatnonzero(ref["on_edge"])
    assert len(out) == gfa.count_paths(ref["level"], ig.src, ig.dst, eidx, L)
    assert (out["from"]["id"] == a).all() and (out["to"]["id"] == b).all()
    on_path = {str(ig.ids[i]) for i in np.flatnonzero(ref["level"] >= 0)}
    names = ["from"] + [f"v{j}" for j in range(1, L)] + ["to"]
    assert set(np.concatenate([out[k]["id"].to_numpy() for k in names])) == on_path
    for j, k in enumerate(names):   # every vertex column holds vertices of its own level
        assert (ref["level"][np.searchsorted(ig.ids, out[k]["id"].to_numpy())] == j).all()
