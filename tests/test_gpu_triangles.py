"""Triangle counting on the GPU (lpa_triangle_count, csrc/lpa_tc.hip): every result
bit-exact against the scipy reference tests/tc_ref.py (count[v] = triangles of the
canonical simple undirected graph that contain v), simple degrees and the summary against
numpy over the reference.  Drop-in call: GraphFrame.triangleCount; the package's own
GraphFrame.clusteringCoefficient on top of it."""
from math import comb

import numpy as np
import pandas as pd
import pytest

import tc_ref
from graphs import degree_mix, random_multigraph, star, two_cliques

pytestmark = pytest.mark.gpu

# the create-time overrides of the kernel-form boundaries (DESIGN.md "Triangle counting"),
# each at its smallest legal value
TC_ENV = ("LPA_TC_SHORT", "LPA_TC_WAVE", "LPA_TC_LDS")


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _check(gfa, V, s, d, ref=None):
    """triangle_count() of a fresh handle, plain and with stats, against the reference."""
    s = np.asarray(s, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    if ref is None:
        ref = tc_ref.triangles(V, s, d)
    rcount, rdeg = ref
    rsumm = tc_ref.summary(rcount, rdeg)
    with gfa.Graph(s, d, V) as g:
        count = g.triangle_count()
        count2, deg, summ = g.triangle_count(stats=True)
    assert count.dtype == np.int64 and count.shape == (V,)
    bad = int((count != rcount).sum())
    assert bad == 0, f"{bad} of {V} triangle counts differ from the reference"
    assert np.array_equal(count2, count)
    assert deg.dtype == np.int64 and deg.shape == (V,) and np.array_equal(deg, rdeg)
    assert summ == rsumm
    return count, summ


def _clique(n, first=0):
    iu, ju = np.triu_indices(n, 1)
    return (iu + first).astype(np.int32), (ju + first).astype(np.int32)


# ---- 1. degenerate ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        assert g.triangle_count().size == 0
        count, deg, summ = g.triangle_count(stats=True)
    assert count.size == 0 and deg.size == 0
    assert summ == dict(n_triangles=0, simple_edges=0, wedges=0, n_in_triangle=0, max_count=0, max_count_id=-1)


def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    count, summ = _check(gfa, 1, e, e)
    assert count.tolist() == [0]
    assert summ == dict(n_triangles=0, simple_edges=0, wedges=0, n_in_triangle=0, max_count=0, max_count_id=0)


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    count, summ = _check(gfa, 70, e, e)
    assert not count.any() and summ["simple_edges"] == 0 and summ["max_count_id"] == 0


def test_only_self_loops(gfa):
    v = np.array([3, 3, 0, 99, 64, 64, 64], np.int32)
    count, summ = _check(gfa, 100, v, v)
    assert not count.any() and summ["simple_edges"] == 0 and summ["wedges"] == 0


def test_one_edge_repeated(gfa):
    count, summ = _check(gfa, 9, np.full(1000, 6, np.int32), np.full(1000, 2, np.int32))
    assert not count.any() and summ["simple_edges"] == 1 and summ["wedges"] == 0


def test_both_directions_only(gfa):
    count, summ = _check(gfa, 4, np.array([1, 3], np.int32), np.array([3, 1], np.int32))
    assert not count.any() and summ["simple_edges"] == 1


def test_triangle_as_heavy_multigraph(gfa):
    """1000 copies of each edge in both directions, plus self-loops at the corners."""
    a = np.array([0, 1, 2, 1, 2, 0], np.int32)
    b = np.array([1, 2, 0, 0, 1, 2], np.int32)
    s = np.concatenate([np.tile(a, 1000), [0, 1, 2, 2]]).astype(np.int32)
    d = np.concatenate([np.tile(b, 1000), [0, 1, 2, 2]]).astype(np.int32)
    count, summ = _check(gfa, 3, s, d)
    assert count.tolist() == [1, 1, 1]
    assert summ == dict(n_triangles=1, simple_edges=3, wedges=3, n_in_triangle=3, max_count=1, max_count_id=0)


# ---- 2. closed forms ----
@pytest.mark.parametrize("n", [3, 5, 70])
def test_complete_graph(gfa, n):
    """All degrees equal: the id tie-break orients every edge; K70's rows cross 64 lanes."""
    count, summ = _check(gfa, n, *_clique(n))
    assert (count == comb(n - 1, 2)).all() and summ["n_triangles"] == comb(n, 3)
    assert comb(69, 2) == 2346


def test_circulant(gfa):
    n = 1000
    i = np.arange(n)
    s = np.concatenate([i, i])
    d = np.concatenate([(i + 1) % n, (i + 2) % n])
    count, summ = _check(gfa, n, s, d)
    assert (count == 3).all() and summ["n_triangles"] == n


def test_wheel(gfa):
    n = 5000
    rim = np.arange(1, n + 1)
    s = np.concatenate([np.zeros(n, np.int64), rim])
    d = np.concatenate([rim, rim % n + 1])
    count, summ = _check(gfa, n + 1, s, d)
    assert count[0] == n and (count[1:] == 2).all()
    assert summ["n_triangles"] == n and summ["max_count_id"] == 0


def test_book(gfa):
    """Two adjacent hubs sharing 5000 leaves: every match adds to the same two counters."""
    n = 5000
    leaves = np.arange(2, n + 2)
    s = np.concatenate([[0], np.zeros(n, np.int64), np.ones(n, np.int64)])
    d = np.concatenate([[1], leaves, leaves])
    count, summ = _check(gfa, n + 2, s, d)
    assert count[0] == n and count[1] == n and (count[2:] == 1).all()
    assert summ["n_triangles"] == n and summ["max_count"] == n and summ["max_count_id"] == 0


# ---- 3. work without matches ----
def test_star(gfa):
    V, s, d = star(5000)
    count, summ = _check(gfa, V, s, d)
    assert not count.any() and summ["wedges"] == 12_497_500 and summ["n_triangles"] == 0


def test_complete_bipartite(gfa):
    a, b = np.meshgrid(np.arange(64), np.arange(64, 128))
    count, summ = _check(gfa, 128, a.ravel(), b.ravel())
    assert not count.any() and summ["simple_edges"] == 4096


# ---- 4. every boundary of the kernel forms ----
# K_{B+2} has out-lists of every length 0 .. B + 1.  Defaults: group <= 8 < wave <= 1024 <
# block with the list in LDS <= 15360 < block with the list in global memory.
@pytest.mark.parametrize("n, env", [
    (10, {}),                                             # B = 8, the group form's end
    (1026, {}),                                           # B = 1024, the wave form's end; one LDS-block row
    (66, {"LPA_TC_WAVE": "16", "LPA_TC_LDS": "64"}),      # B = 64, the LDS boundary lowered: all four forms
    (1026, {"LPA_TC_WAVE": "0"}),                         # LDS-block rows of up to five 256-neighbour chunks
    (1026, {"LPA_TC_WAVE": "0", "LPA_TC_LDS": "0"}),      # the same rows with the list in global memory
    (300, {"LPA_TC_SHORT": "0"}),                         # no group form: wave rows from length 2
    (300, {"LPA_TC_SHORT": "299"}),                       # the group form on lists far beyond its 8 lanes
], ids=["K10", "K1026", "K66-lds64", "K1026-block", "K1026-global", "K300-nogroup", "K300-group"])
def test_form_boundaries(gfa, monkeypatch, n, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, d = _clique(n)
    want = np.full(n, comb(n - 1, 2), np.int64)
    count, summ = _check(gfa, n, s, d, ref=(want, np.full(n, n - 1, np.int64)))
    assert summ["n_triangles"] == comb(n, 3)


@pytest.fixture(scope="module")
def mix():
    V, s, d = degree_mix()
    ref = tc_ref.triangles(V, s, d)
    for a in ref:
        a.setflags(write=False)
    return V, s, d, ref


@pytest.mark.parametrize("env", [{}, {"LPA_TC_SHORT": "0"}, {"LPA_TC_WAVE": "0"}, {"LPA_TC_LDS": "0"},
                                 {k: "0" for k in TC_ENV}],
                         ids=["defaults", "short0", "wave0", "lds0", "all0"])
def test_degree_mix_under_overrides(gfa, monkeypatch, mix, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    V, s, d, ref = mix
    _check(gfa, V, s, d, ref=ref)


# ---- 5. mixed graphs ----
def test_two_cliques(gfa):
    V, s, d = two_cliques()
    count, summ = _check(gfa, V, s, d)
    # K5 on 0..4, K6 on 5..10, the bridge 0-5 closes nothing
    assert count.tolist() == [6] * 5 + [10] * 6 and summ["n_triangles"] == 10 + 20


def test_degree_mix(gfa, mix):
    V, s, d, ref = mix
    _, summ = _check(gfa, V, s, d, ref=ref)
    assert summ == dict(n_triangles=13736, simple_edges=23002, wedges=3368604, n_in_triangle=2673,
                        max_count=11868, max_count_id=616)


def test_sparse_random(gfa):
    V, s, d = random_multigraph(20000, 200000, 3)
    _, summ = _check(gfa, V, s, d)
    assert summ["n_triangles"] == 1310


@pytest.fixture(scope="module")
def dense_random():
    V, s, d = random_multigraph(2000, 60000, 7)
    ref = tc_ref.triangles(V, s, d)
    for a in ref:
        a.setflags(write=False)
    return V, s, d, ref


def test_dense_random(gfa, dense_random):
    V, s, d, ref = dense_random
    _, summ = _check(gfa, V, s, d, ref=ref)
    assert summ["n_triangles"] == 34233 and summ["n_in_triangle"] == V


# ---- 6. determinism ----
def test_deterministic_across_edge_orders(gfa, dense_random):
    V, s, d, ref = dense_random
    order = np.random.default_rng(9).permutation(s.size)
    got = []
    for ss, dd in ((s, d), (s[::-1].copy(), d[::-1].copy()), (s[order], d[order]), (d, s)):
        with gfa.Graph(ss, dd, V) as g:
            got.append(g.triangle_count(stats=True))
    for count, deg, summ in got:
        assert np.array_equal(count, got[0][0]) and np.array_equal(deg, got[0][1]) and summ == got[0][2]
    assert np.array_equal(got[0][0], ref[0]) and np.array_equal(got[0][1], ref[1])
    assert got[0][2] == tc_ref.summary(*ref)


# ---- 7. device path ----
def test_device_tensors(gfa):
    import torch

    scale = 14
    V = 1 << scale
    s, d = gfa.gen_rmat(scale, 16, seed=1)
    rcount, rdeg = tc_ref.triangles(V, s.cpu().numpy(), d.cpu().numpy())
    rsumm = tc_ref.summary(rcount, rdeg)
    assert rsumm["n_triangles"] > 0
    with gfa.Graph(s, d, V) as g:
        out = torch.full((V,), -1, dtype=torch.int64, device=s.device)
        assert g.triangle_count(out=out) is out
        assert np.array_equal(out.cpu().numpy(), rcount)
        out.fill_(-1)
        count, deg, summ = g.triangle_count(out=out, stats=True)
        assert count is out and deg.is_cuda and deg.dtype == torch.int64
        assert np.array_equal(out.cpu().numpy(), rcount) and np.array_equal(deg.cpu().numpy(), rdeg)
        assert summ == rsumm
        assert np.array_equal(g.triangle_count(), rcount)   # host output of the same handle
        with pytest.raises(ValueError, match="int64"):
            g.triangle_count(out=torch.empty(V, dtype=torch.int32, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.triangle_count(out=torch.empty(V - 1, dtype=torch.int64, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.triangle_count(out=torch.empty(V + 1, dtype=torch.int64, device=s.device))
        with pytest.raises(ValueError, match="contiguous"):
            g.triangle_count(out=torch.empty(2 * V, dtype=torch.int64, device=s.device)[::2])
        with pytest.raises(ValueError, match="device tensor"):
            g.triangle_count(out=np.empty(V, np.int64))


# ---- 8. the LPA state is untouched ----
def test_does_not_disturb_lpa(gfa, mix):
    V, s, d, ref = mix
    with gfa.Graph(s, d, V) as g:
        want = g.run(3)
    with gfa.Graph(s, d, V) as g:
        g.reset()
        g.step(1)
        before = g.info()["device_bytes"]
        c1 = g.triangle_count()
        assert g.info()["device_bytes"] == before
        g.step(1)
        c2, _, _ = g.triangle_count(stats=True)
        assert g.info()["device_bytes"] == before
        g.step(1)
        got = g.labels()
    assert np.array_equal(got, want)
    assert np.array_equal(c1, ref[0]) and np.array_equal(c2, ref[0])


# ---- 9. drop-in ----
def test_graphframe_string_ids(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    rcount, _ = tc_ref.triangles(ig.num_vertices, ig.src, ig.dst)
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.triangleCount()
    finally:
        gf.close()
    assert list(out.columns) == ["id", "name", "count"] and out["count"].dtype == np.int64
    assert np.array_equal(out["id"].to_numpy(), ig.ids)
    assert np.array_equal(out["count"].to_numpy(), rcount)
    assert int(out["count"].sum()) == 3 * 2834
    assert out.equals(gfa.triangle_count(v, e))


def test_graphframe_integral_ids(gfa):
    v = pd.DataFrame({"id": np.array([30, 10, 20, 40], np.int64), "name": ["c", "a", "b", "d"]})
    e = pd.DataFrame({"src": np.array([10, 20, 30, 40], np.int64), "dst": np.array([20, 30, 10, 99], np.int64)})
    out = gfa.triangle_count(v, e)
    assert dict(zip(out["id"].tolist(), out["count"].tolist())) == {10: 1, 20: 1, 30: 1, 40: 0}
    assert dict(zip(out["id"].tolist(), out["name"].tolist())) == {10: "a", 20: "b", 30: "c", 40: "d"}
    assert out["count"].dtype == np.int64


def test_clustering_coefficient(gfa):
    """Two triangles sharing vertex 0, and a pendant vertex 5 on 1."""
    v = pd.DataFrame({"id": np.arange(6, dtype=np.int64)})
    e = pd.DataFrame({"src": np.array([0, 1, 2, 0, 3, 4, 5], np.int64),
                      "dst": np.array([1, 2, 0, 3, 4, 0, 5], np.int64)})
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.clusteringCoefficient()
    finally:
        gf.close()
    assert list(out.columns) == ["id", "count", "degree", "lcc"]
    assert out["count"].dtype == np.int64 and out["degree"].dtype == np.int64 and out["lcc"].dtype == np.float64
    assert out["count"].tolist() == [2, 1, 1, 1, 1, 0] and out["degree"].tolist() == [4, 2, 2, 2, 2, 0]
    assert out["lcc"].tolist() == [1 / 3, 1.0, 1.0, 1.0, 1.0, 0.0]
    assert out.attrs["transitivity"] == 0.6   # 3 * 2 triangles / 10 wedges
    # a pendant vertex (one neighbour) has lcc 0.0 and moves the transitivity only
    e2 = pd.concat([e, pd.DataFrame({"src": [5], "dst": [1]})], ignore_index=True)
    gf = gfa.GraphFrame(v, e2)
    try:
        out = gf.clusteringCoefficient()
    finally:
        gf.close()
    assert out["degree"].tolist() == [4, 3, 2, 2, 2, 1] and out["lcc"].tolist() == [1 / 3, 1 / 3, 1.0, 1.0, 1.0, 0.0]
    assert out.attrs["transitivity"] == 3 * 2 / 12


# ---- 10. partitioned job: rank 0 keeps the edge list ----
def test_two_loopback_ranks(gfa, mix):
    V, s, d, ref = mix
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        count, deg, summ = ranks[0].triangle_count(stats=True)
        assert np.array_equal(count, ref[0]) and np.array_equal(deg, ref[1])
        assert summ == tc_ref.summary(*ref)
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].triangle_count()
    finally:
        for g in ranks:
            g.close()
        lb.close()
