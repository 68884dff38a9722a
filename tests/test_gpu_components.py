"""Connected components on the GPU (lpa_components, csrc/lpa_cc.hip): every result
bit-exact against the numpy reference tests/cc_ref.py (comp[v] = the smallest dense id of
v's component), sizes and summary against np.bincount of the reference.  Drop-in call:
GraphFrame.connectedComponents."""
import numpy as np
import pandas as pd
import pytest

import cc_ref
from graphs import degree_mix, random_multigraph, star, two_cliques

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _check(gfa, V, s, d, ref=None):
    """components() of a fresh handle, plain and with sizes, against the reference."""
    s = np.asarray(s, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    if ref is None:
        ref = cc_ref.components(V, s, d)
    rsizes, rsumm = cc_ref.summary(ref)
    with gfa.Graph(s, d, V) as g:
        comp = g.components()
        comp2, sizes, summ = g.components(sizes=True)
    assert comp.dtype == np.int32 and comp.shape == (V,)
    bad = int((comp != ref).sum())
    assert bad == 0, f"{bad} of {V} component ids differ from the reference"
    assert np.array_equal(comp2, comp)
    assert sizes.dtype == np.int64 and np.array_equal(sizes, rsizes)
    assert summ == rsumm
    return comp, summ


# ---- 1. degenerate ----
def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    comp, summ = _check(gfa, 1, e, e)
    assert comp.tolist() == [0]
    assert summ == dict(n_components=1, n_singletons=1, largest_size=1, largest_id=0)


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    comp, summ = _check(gfa, 70, e, e)
    assert np.array_equal(comp, np.arange(70))
    assert summ == dict(n_components=70, n_singletons=70, largest_size=1, largest_id=0)


def test_only_self_loops(gfa):
    v = np.array([3, 3, 0, 99, 64, 64, 64], np.int32)
    comp, summ = _check(gfa, 100, v, v)
    assert np.array_equal(comp, np.arange(100)) and summ["n_singletons"] == 100


def test_one_edge_repeated(gfa):
    s = np.full(1000, 6, np.int32)
    d = np.full(1000, 2, np.int32)
    comp, summ = _check(gfa, 9, s, d)
    assert comp.tolist() == [0, 1, 2, 3, 4, 5, 2, 7, 8]
    assert summ == dict(n_components=8, n_singletons=7, largest_size=2, largest_id=2)


def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        assert g.components().size == 0
        comp, sizes, summ = g.components(sizes=True)
    assert comp.size == 0 and sizes.size == 0
    assert summ == dict(n_components=0, n_singletons=0, largest_size=0, largest_id=-1)


# ---- 2. two cliques and their bridge ----
def test_two_cliques(gfa):
    V, s, d = two_cliques()
    comp, summ = _check(gfa, V, s, d)
    assert not comp.any()
    assert summ == dict(n_components=1, n_singletons=0, largest_size=V, largest_id=0)


# ---- 3. contention on one root ----
def test_star(gfa):
    V, s, d = star(5000)
    comp, _ = _check(gfa, V, s, d)
    assert not comp.any()


def test_star_hub_is_largest_id(gfa):
    """Every edge first sees the hub V - 1; the root must still end at 0."""
    V = 5001
    leaves = np.arange(V - 1, dtype=np.int32)
    comp, summ = _check(gfa, V, np.full(V - 1, V - 1, np.int32), leaves)
    assert not comp.any() and summ["largest_size"] == V


# ---- 4. depth: one path of 65,536 vertices in three listings ----
@pytest.mark.parametrize("listing", ["ascending", "descending", "scrambled"])
def test_path(gfa, listing):
    V = 65536
    i = np.arange(V - 1, dtype=np.int32)
    if listing == "ascending":
        s, d = i, i + 1
    elif listing == "descending":
        s, d = (i + 1)[::-1].copy(), i[::-1].copy()
    else:
        rng = np.random.default_rng(4)
        p = rng.permutation(V).astype(np.int32)
        order = rng.permutation(V - 1)
        s, d = p[i][order], p[i + 1][order]
    comp, summ = _check(gfa, V, s, d, ref=np.zeros(V, np.int64))
    assert summ == dict(n_components=1, n_singletons=0, largest_size=V, largest_id=0)


# ---- 5. late merge ----
def test_late_merge(gfa):
    """Two scrambled 20,000-vertex paths; the last edge of the list joins their largest ids."""
    n = 20000
    rng = np.random.default_rng(5)
    p = rng.permutation(2 * n).astype(np.int32)
    a, b = p[:n], p[n:]
    s = np.concatenate([a[:-1], b[:-1]])
    d = np.concatenate([a[1:], b[1:]])
    order = rng.permutation(s.size)
    s = np.concatenate([s[order], [a.max()]]).astype(np.int32)
    d = np.concatenate([d[order], [b.max()]]).astype(np.int32)
    comp, _ = _check(gfa, 2 * n, s, d)
    assert not comp.any()
    # without the last edge: two components
    comp, summ = _check(gfa, 2 * n, s[:-1], d[:-1])
    assert summ["n_components"] == 2 and summ["largest_size"] == n
    assert set(np.unique(comp).tolist()) == {int(a.min()), int(b.min())}


# ---- 6. many small components / 9. determinism ----
@pytest.fixture(scope="module")
def many_small():
    V, s, d = random_multigraph(200000, 150000, 3)
    ref = cc_ref.components(V, s, d)
    ref.setflags(write=False)
    return V, s, d, ref


def test_many_small_components(gfa, many_small):
    V, s, d, ref = many_small
    _, summ = _check(gfa, V, s, d, ref=ref)
    assert summ["n_components"] == 57312 and summ["largest_size"] == 116251
    assert summ["n_singletons"] == int((np.bincount(ref, minlength=V) == 1).sum())


def test_deterministic_across_edge_orders(gfa, many_small):
    V, s, d, ref = many_small
    order = np.random.default_rng(9).permutation(s.size)
    got = []
    for ss, dd in ((s, d), (s[::-1].copy(), d[::-1].copy()), (s[order], d[order]), (d, s)):
        with gfa.Graph(ss, dd, V) as g:
            got.append(g.components(sizes=True))
    for comp, sizes, summ in got:
        assert np.array_equal(comp, got[0][0]) and np.array_equal(sizes, got[0][1]) and summ == got[0][2]
    assert np.array_equal(got[0][0], ref)


# ---- 7. hubs, duplicates, self-loops, isolated ids ----
def test_degree_mix(gfa):
    V, s, d = degree_mix()
    _, summ = _check(gfa, V, s, d)
    assert summ["n_components"] == 8 and summ["largest_size"] == 3047


# ---- 8. device path ----
def test_device_tensors(gfa):
    import torch

    scale = 16
    V = 1 << scale
    s, d = gfa.gen_rmat(scale, 16, seed=1)
    ref = cc_ref.components(V, s.cpu().numpy(), d.cpu().numpy())
    rsizes, rsumm = cc_ref.summary(ref)
    with gfa.Graph(s, d, V) as g:
        out = torch.full((V,), -1, dtype=torch.int32, device=s.device)
        assert g.components(out=out) is out
        assert np.array_equal(out.cpu().numpy(), ref)
        out.fill_(-1)
        comp, sizes, summ = g.components(out=out, sizes=True)
        assert comp is out and sizes.is_cuda and sizes.dtype == torch.int64
        assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(sizes.cpu().numpy(), rsizes)
        assert summ == rsumm
        assert np.array_equal(g.components(), ref)   # host output of the same handle
        with pytest.raises(ValueError, match="int32"):
            g.components(out=torch.empty(V, dtype=torch.int64, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.components(out=torch.empty(V - 1, dtype=torch.int32, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.components(out=torch.empty(V + 1, dtype=torch.int32, device=s.device))
        with pytest.raises(ValueError, match="contiguous"):
            g.components(out=torch.empty(2 * V, dtype=torch.int32, device=s.device)[::2])
        with pytest.raises(ValueError, match="device tensor"):
            g.components(out=np.empty(V, np.int32))


# ---- 10. the LPA state is untouched ----
def test_does_not_disturb_lpa(gfa):
    V, s, d = degree_mix()
    ref = cc_ref.components(V, s, d)
    with gfa.Graph(s, d, V) as g:
        want = g.run(3)
    with gfa.Graph(s, d, V) as g:
        g.reset()
        g.step(1)
        before = g.info()["device_bytes"]
        c1 = g.components()
        assert g.info()["device_bytes"] == before
        g.step(1)
        c2, _, _ = g.components(sizes=True)
        assert g.info()["device_bytes"] == before
        g.step(1)
        got = g.labels()
    assert np.array_equal(got, want)
    assert np.array_equal(c1, ref) and np.array_equal(c2, ref)


# ---- 11. drop-in ----
def test_graphframe_string_ids(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    ref = cc_ref.components(ig.num_vertices, ig.src, ig.dst)
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.connectedComponents()
        again = gf.connectedComponents(algorithm="graphx", checkpointInterval=5, broadcastThreshold=10)
    finally:
        gf.close()
    assert out["component"].dtype == np.int64 and list(out.columns) == ["id", "name", "component"]
    assert np.array_equal(out["id"].to_numpy(), ig.ids)
    assert np.array_equal(out["component"].to_numpy(), ref)
    counts = out["component"].value_counts()
    assert counts.size == 34 and int(counts.max()) == 4440
    assert out.equals(again)
    assert out.equals(gfa.connected_components(v, e))


def test_graphframe_integral_ids(gfa):
    v = pd.DataFrame({"id": np.array([30, 10, 20, 40], np.int64), "name": ["c", "a", "b", "d"]})
    e = pd.DataFrame({"src": np.array([10, 40], np.int64), "dst": np.array([30, 99], np.int64)})
    out = gfa.connected_components(v, e)
    assert dict(zip(out["id"].tolist(), out["component"].tolist())) == {10: 10, 30: 10, 20: 20, 40: 40}
    assert dict(zip(out["id"].tolist(), out["name"].tolist())) == {10: "a", 20: "b", 30: "c", 40: "d"}
    assert out["component"].dtype == np.int64


# ---- 12. partitioned job: rank 0 keeps the edge list ----
def test_two_loopback_ranks(gfa):
    V, s, d = degree_mix()
    ref = cc_ref.components(V, s, d)
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        comp, sizes, summ = ranks[0].components(sizes=True)
        assert np.array_equal(comp, ref)
        rsizes, rsumm = cc_ref.summary(ref)
        assert np.array_equal(sizes, rsizes) and summ == rsumm
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].components()
    finally:
        for g in ranks:
            g.close()
        lb.close()
