"""Landmark shortest paths on the GPU (lpa_shortest_paths, csrc/lpa_sp.hip) against the numpy
reference tests/sp_ref.py: exact integer equality of every distance and of every summary field
that does not depend on the schedule; push_levels + pull_levels against the reference's level
count; identical distances under the push-only and pull-only overrides, across edge orders,
calls and handles.  Drop-in calls: GraphFrame.shortestPaths, shortest_paths."""
import numpy as np
import pandas as pd
import pytest

import sp_ref
from graphs import degree_mix, random_multigraph, star, two_cliques

pytestmark = pytest.mark.gpu

# the create-time overrides of the push / pull switch (DESIGN.md "Shortest paths")
SP_OVERRIDES = [{}, {"LPA_SP_ALPHA": "0"}, {"LPA_SP_PULL": "1"}]
SP_IDS = ["defaults", "push-only", "pull-only"]


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _compare(got, V, s, d, lms, ref=None):
    """One stats=True result against the reference; returns the reference distances."""
    dist, summ = got
    if ref is None:
        ref = sp_ref.shortest_paths(V, s, d, lms)
    assert dist.dtype == np.int32 and dist.shape == (len(lms), V)
    assert np.array_equal(dist, ref), f"{int((dist != ref).sum())} of {dist.size} distances differ"
    want = sp_ref.summary(V, s, d, ref)
    levels = want.pop("levels")
    print(f"V={V} landmarks={len(lms)} summary={summ} levels={levels}")
    for key, val in want.items():
        assert summ[key] == val, key
    assert summ["push_levels"] >= 0 and summ["pull_levels"] >= 0
    assert summ["push_levels"] + summ["pull_levels"] == levels
    return ref


def _check(gfa, V, s, d, lms, g=None, ref=None):
    """shortest_paths() plain and with stats (of a fresh handle unless g is given) against the reference."""
    s = np.asarray(s, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    own = g is None
    if own:
        g = gfa.Graph(s, d, V)
    try:
        dist = g.shortest_paths(lms)
        got = g.shortest_paths(lms, stats=True)
    finally:
        if own:
            g.close()
    assert np.array_equal(dist, got[0])
    _compare(got, V, s, d, lms, ref)
    return got


# ---- 1. degenerate ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        assert g.shortest_paths([]).shape == (0, 0)
        dist, summ = g.shortest_paths([], stats=True)
        with pytest.raises(ValueError, match="landmark 0"):
            g.shortest_paths([0])
    assert dist.shape == (0, 0)
    assert summ == dict(arcs=0, reached=0, max_distance=-1, batches=0, push_levels=0, pull_levels=0)


def test_no_landmarks(gfa):
    V, s, d = random_multigraph(100, 400, 2)
    s2 = np.concatenate([s, s[:50], np.arange(9, dtype=np.int32)])
    d2 = np.concatenate([d, d[:50], np.arange(9, dtype=np.int32)])
    with gfa.Graph(s2, d2, V) as g:
        assert g.shortest_paths([]).shape == (0, V)
        dist, summ = g.shortest_paths([], stats=True)
    assert dist.shape == (0, V)
    arcs = sp_ref.summary(V, s, d, dist)["arcs"]
    assert 0 < arcs <= 400
    assert summ == dict(arcs=arcs, reached=0, max_distance=-1, batches=0, push_levels=0, pull_levels=0)


def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    dist, summ = _check(gfa, 1, e, e, [0])
    assert dist.tolist() == [[0]]
    assert {k: summ[k] for k in ("arcs", "reached", "max_distance", "batches")} == dict(arcs=0, reached=1,
                                                                                       max_distance=0, batches=1)


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    lms = np.arange(70, dtype=np.int32)
    dist, summ = _check(gfa, 70, e, e, lms)
    assert np.array_equal(dist, np.where(np.eye(70, dtype=bool), 0, -1))
    assert summ["arcs"] == 0 and summ["reached"] == 70 and summ["batches"] == 2


def test_only_self_loops(gfa):
    v = np.array([3, 3, 0, 99, 64, 64, 64], np.int32)
    dist, summ = _check(gfa, 100, v, v, [3, 0, 64, 5])
    assert summ["arcs"] == 0 and summ["reached"] == 4 and summ["max_distance"] == 0
    assert (dist >= 0).sum() == 4


def test_one_edge_repeated(gfa):
    s, d = np.full(1000, 6, np.int32), np.full(1000, 2, np.int32)
    dist, summ = _check(gfa, 9, s, d, [2, 6])
    assert summ["arcs"] == 1 and summ["reached"] == 3 and summ["max_distance"] == 1
    assert dist[0, 6] == 1 and dist[1, 2] == -1   # 6 -> 2: 6 reaches 2, 2 does not reach 6


# ---- 2. batch edges ----
@pytest.fixture(scope="module")
def mix():
    V, s, d = degree_mix()
    lms = sp_ref.evenly_spaced(V, 130)
    ref = sp_ref.shortest_paths(V, s, d, lms)
    ref.setflags(write=False)
    return V, s, d, lms, ref


def test_batch_edges(gfa, mix):
    V, s, d, lms, ref = mix
    with gfa.Graph(s, d, V) as g:
        for n in (1, 63, 64, 65, 130):
            _, summ = _check(gfa, V, s, d, lms[:n], g=g, ref=ref[:n])
            assert summ["batches"] == (n + 63) // 64


def test_repeated_landmarks(gfa, mix):
    V, s, d, lms, ref = mix
    a, b = int(lms[3]), int(lms[40])
    rep = [a] * 40 + [b] + [a] * 30   # the repeats straddle the batch edge
    dist, _ = _check(gfa, V, s, d, rep)
    for i, l in enumerate(rep):
        assert np.array_equal(dist[i], ref[3 if l == a else 40])


# ---- 3. transpose tail ----
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000])
def test_transpose_tail(gfa, V):
    _, s, d = random_multigraph(V, 3 * V, 11 + V)
    lms = np.arange(V, dtype=np.int32) if V <= 65 else np.arange(0, V, 7, dtype=np.int32)
    _check(gfa, V, s, d, lms)
    _check(gfa, V, s, d, lms[::-1].copy())


# ---- 4. depth and direction ----
def test_directed_path(gfa):
    n = 2000
    V, s, d = sp_ref.path(n)
    dist, summ = _check(gfa, V, s, d, [n - 1, 0])
    assert np.array_equal(dist[0], n - 1 - np.arange(n))
    assert dist[1, 0] == 0 and (dist[1, 1:] == -1).all()
    assert summ["max_distance"] == n - 1 and summ["reached"] == n + 1


def test_directed_cycle(gfa):
    n = 1000
    V, s, d = sp_ref.cycle(n)
    lms = [0, 1, 499, 999]
    dist, summ = _check(gfa, V, s, d, lms)
    for row, l in zip(dist, lms):
        assert np.array_equal(row, (l - np.arange(n)) % n)
    assert summ["max_distance"] == n - 1 and summ["reached"] == 4 * n


def test_two_cliques_directed_bridge(gfa):
    """The bridge 0 -> n is directed: the first clique reaches the second, not the reverse."""
    V, s, d = two_cliques(5)
    dist, _ = _check(gfa, V, s, d, [0, 5, 10])
    assert (dist[0, 5:] == -1).all() and (dist[0, :5] >= 0).all()
    assert dist[1, 0] == 1 and dist[1, 1] == 2 and dist[2, 0] == 2 and dist[2, 3] == 3


# ---- 5. long lists ----
@pytest.mark.parametrize("env", SP_OVERRIDES, ids=SP_IDS)
def test_star_into_hub(gfa, monkeypatch, env):
    """leaves -> hub: the hub's in-list of 100 000 in the push (its block form)."""
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    V, d, s = star(100_000)
    dist, summ = _check(gfa, V, s, d, [0, 1, 77_777, 100_000])
    assert dist[0, 0] == 0 and (dist[0, 1:] == 1).all()
    assert (dist[1:] >= 0).sum() == 3 and summ["arcs"] == 100_000 and summ["max_distance"] == 1


@pytest.mark.parametrize("env", SP_OVERRIDES, ids=SP_IDS)
def test_star_out_of_hub(gfa, monkeypatch, env):
    """hub -> leaves: the hub's out-list of 100 000 in the pull (its block form, early exit)."""
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    V, s, d = star(100_000)
    dist, summ = _check(gfa, V, s, d, [0, 1, 77_777, 100_000])
    assert (dist[0] >= 0).sum() == 1
    for row, l in zip(dist[1:], (1, 77_777, 100_000)):
        assert row[0] == 1 and row[l] == 0 and (row >= 0).sum() == 2
    assert summ["max_distance"] == 1


# ---- 6. schedule independence ----
def _under_overrides(gfa, monkeypatch, V, s, d, lms, ref):
    got = []
    for env in SP_OVERRIDES:
        with monkeypatch.context() as mp:
            for key, val in env.items():
                mp.setenv(key, val)
            g = gfa.Graph(s, d, V)   # the overrides are read when the handle is created
        try:
            got.append(g.shortest_paths(lms, stats=True))
        finally:
            g.close()
    for res in got:
        _compare(res, V, s, d, lms, ref)
        assert np.array_equal(res[0], got[0][0])
    (_, dflt), (_, push), (_, pull) = got
    assert push["pull_levels"] == 0 and pull["push_levels"] == 0
    assert (dflt["push_levels"] + dflt["pull_levels"] == push["push_levels"] + push["pull_levels"]
            == pull["push_levels"] + pull["pull_levels"])


def test_schedules_agree_on_degree_mix(gfa, monkeypatch, mix):
    V, s, d, lms, ref = mix
    _under_overrides(gfa, monkeypatch, V, s, d, lms, ref)


def test_schedules_agree_on_r9(gfa, monkeypatch, golden):
    V = int(golden["ids"].size)
    s, d = golden["src"], golden["dst"]
    lms = sp_ref.top_in_degree(V, s, d, 70)
    ref = sp_ref.shortest_paths(V, s, d, lms)
    assert int(ref.max()) == 6
    _under_overrides(gfa, monkeypatch, V, s, d, lms, ref)


# ---- 7. invariance ----
def test_edge_order_duplicates_and_loops(gfa, mix):
    V, s, d, lms, ref = mix
    rng = np.random.default_rng(9)
    perm = rng.permutation(s.size)
    dup = rng.integers(0, s.size, size=5000)
    loops = rng.integers(0, V, size=500).astype(np.int32)
    variants = [(s[::-1].copy(), d[::-1].copy()), (s[perm], d[perm]),
                (np.concatenate([s, s[dup]]), np.concatenate([d, d[dup]])),
                (np.concatenate([loops, s]), np.concatenate([loops, d]))]
    for vs, vd in variants:
        with gfa.Graph(vs, vd, V) as g:
            got = g.shortest_paths(lms, stats=True)
        _compare(got, V, s, d, lms, ref)


def test_calls_and_handles(gfa, mix):
    V, s, d, lms, ref = mix
    with gfa.Graph(s, d, V) as g:
        a = g.shortest_paths(lms, stats=True)
        b = g.shortest_paths(lms, stats=True)
    with gfa.Graph(s, d, V) as g:
        c = g.shortest_paths(lms, stats=True)
    assert np.array_equal(a[0], ref) and np.array_equal(b[0], ref) and np.array_equal(c[0], ref)
    assert a[1] == b[1] == c[1]


# ---- 8. isolation ----
def test_does_not_disturb_lpa(gfa, mix):
    V, s, d, lms, ref = mix
    with gfa.Graph(s, d, V) as g:
        want = g.run(5)
        before = g.info()["device_bytes"]
        dist = g.shortest_paths(lms[:65])
        assert g.info()["device_bytes"] == before
        assert np.array_equal(g.labels(), want)
        assert np.array_equal(g.run(5), want)
        assert g.info()["device_bytes"] == before
    assert np.array_equal(dist, ref[:65])
    with gfa.Graph(s, d, V) as g:   # between supersteps
        g.reset()
        g.step(2)
        g.shortest_paths(lms[:3])
        g.step(3)
        assert np.array_equal(g.labels(), want)


def test_device_tensor(gfa, mix):
    import torch

    V, s, d, lms, ref = mix
    n = 65
    with gfa.Graph(s, d, V) as g:
        out = torch.full((n, V), 7, dtype=torch.int32, device="cuda:0")
        assert g.shortest_paths(lms[:n], out=out) is out
        assert np.array_equal(out.cpu().numpy(), ref[:n])
        out.fill_(7)
        dist, summ = g.shortest_paths(lms[:n], out=out, stats=True)
        assert dist is out
        _compare((out.cpu().numpy(), summ), V, s, d, lms[:n], ref[:n])
        assert np.array_equal(g.shortest_paths(lms[:n]), ref[:n])   # host output of the same handle
        with pytest.raises(ValueError, match="int32"):
            g.shortest_paths(lms[:n], out=torch.empty((n, V), dtype=torch.int64, device="cuda:0"))
        with pytest.raises(ValueError, match=f"{V}"):
            g.shortest_paths(lms[:n], out=torch.empty((n, V - 1), dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError, match=f"{n}"):
            g.shortest_paths(lms[:n], out=torch.empty((n + 1, V), dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError, match="contiguous"):
            g.shortest_paths(lms[:n], out=torch.empty((n, 2 * V), dtype=torch.int32, device="cuda:0")[:, ::2])
        with pytest.raises(ValueError, match="device tensor"):
            g.shortest_paths(lms[:n], out=np.empty((n, V), np.int32))
        with pytest.raises(ValueError, match=f"landmark {V}"):
            g.shortest_paths([0, V])
        with pytest.raises(TypeError, match="landmark"):
            g.shortest_paths([0.5])
        # the C ABI's own argument checks
        lm = np.array([0, V], np.int32)
        buf = np.empty((2, V), np.int32)
        lib = g._lib
        i32p = gfa._lib._i32p
        assert lib.lpa_shortest_paths(g._handle(), lm.ctypes.data_as(i32p), 2, buf.ctypes.data, 0, None) == gfa._lib.LPA_EINVAL
        assert "landmark" in gfa._lib.last_error()
        assert lib.lpa_shortest_paths(g._handle(), lm.ctypes.data_as(i32p), -1, buf.ctypes.data, 0, None) == gfa._lib.LPA_EINVAL
        assert lib.lpa_shortest_paths(g._handle(), None, 1, buf.ctypes.data, 0, None) == gfa._lib.LPA_EINVAL
        assert lib.lpa_shortest_paths(g._handle(), lm.ctypes.data_as(i32p), 1, None, 0, None) == gfa._lib.LPA_EINVAL


def test_two_loopback_ranks(gfa, mix):
    V, s, d, lms, ref = mix
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        _compare(ranks[0].shortest_paths(lms[:65], stats=True), V, s, d, lms[:65], ref[:65])
        # LPA_EINVAL, which the binding raises as ValueError (as for the other edge-list calls)
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].shortest_paths(lms[:65])
    finally:
        for g in ranks:
            g.close()
        lb.close()


# ---- 9. drop-in ----
def test_graphframe_integral_ids(gfa):
    """10 -> 20 -> 30 -> 10, 40 -> 10, 50 alone, and a dangling 40 -> 99."""
    v = pd.DataFrame({"id": np.array([30, 10, 50, 20, 40], np.int64), "name": ["c", "a", "e", "b", "d"]})
    e = pd.DataFrame({"src": np.array([10, 20, 40, 30, 40], np.int64), "dst": np.array([20, 30, 99, 10, 10], np.int64)})
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.shortestPaths([30, 50, 30, 40, 10])
        with pytest.raises(ValueError, match="landmark 99 is not a vertex id"):
            gf.shortestPaths([10, 99])
        again = gf.shortestPaths((40,))
    finally:
        gf.close()
    assert list(out.columns) == ["id", "name", "distances"] and out["distances"].dtype == object
    assert out["id"].tolist() == [10, 20, 30, 40, 50] and out["name"].tolist() == ["a", "b", "c", "d", "e"]
    want = [{30: 2, 10: 0}, {30: 1, 10: 2}, {30: 0, 10: 1}, {30: 3, 40: 0, 10: 1}, {50: 0}]
    got = out["distances"].tolist()
    assert got == want
    assert [list(m) for m in got] == [list(m) for m in want]   # the landmarks' order, repeats collapsed
    assert all(type(x) is int for m in got for x in m.values())
    assert again["distances"].tolist() == [{}, {}, {}, {40: 0}, {}]
    assert out.equals(gfa.shortest_paths(v, e, [30, 50, 30, 40, 10]))


def test_graphframe_string_ids(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    V = ig.num_vertices
    dense = sp_ref.top_in_degree(V, ig.src, ig.dst, 5)[::-1].copy()
    lms = [str(ig.ids[i]) for i in dense]
    ref = sp_ref.shortest_paths(V, ig.src, ig.dst, dense)
    out = gfa.shortest_paths(v, e, lms)
    assert list(out.columns) == ["id", "name", "distances"]
    assert np.array_equal(out["id"].to_numpy(), ig.ids)
    for vtx, m in enumerate(out["distances"].tolist()):
        hit = np.flatnonzero(ref[:, vtx] >= 0)
        assert list(m) == [lms[l] for l in hit] and list(m.values()) == [int(ref[l, vtx]) for l in hit]
    assert 0 < sum(len(m) for m in out["distances"]) < 5 * V   # some landmark is out of some vertex's reach
