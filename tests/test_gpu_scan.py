"""SCAN structural clustering on the GPU (lpa_scan, csrc/lpa_scan.hip): label, role, nsim, common
and every summary field bit-exact against the set-based reference tests/scan_ref.py, or against
the closed form where the reference would be slow (complete graphs).  The package's own calls:
Graph.scan, GraphFrame.scan, GraphFrame.structuralSimilarity."""
from math import comb

import numpy as np
import pandas as pd
import pytest

import scan_cases
import scan_ref

pytestmark = pytest.mark.gpu

EPS = (0.3, 0.5, 0.7)
MU = (2, 3, 5)


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _same(got, want, what):
    label, role, nsim, summ, common = got
    rlabel, rrole, rnsim, rsumm, rcommon = want
    for name, a, b, dt in (("label", label, rlabel, np.int32), ("role", role, rrole, np.uint8),
                           ("nsim", nsim, rnsim, np.int32), ("common", common, rcommon, np.int32)):
        assert a.dtype == dt and a.shape == b.shape, f"{what}: {name} is {a.dtype}{a.shape}"
        bad = int((a != b).sum())
        assert bad == 0, f"{what}: {bad} of {a.size} entries of {name} differ from the reference"
    assert summ == rsumm, what


def _check(g, prep, eps, mu, what=""):
    """One scan of the handle with every output, against the reference; the plain call agrees."""
    want = scan_ref.scan(prep, eps, mu) + (prep.common_rows,)
    got = g.scan(eps, mu, stats=True, common=True)
    _same(got, want, f"{what} eps={eps} mu={mu}")
    label, role = g.scan(eps, mu)
    assert np.array_equal(label, got[0]) and np.array_equal(role, got[1])
    return got


# ---- 1. closed forms ----
@pytest.mark.parametrize("name", list(scan_cases.CLOSED))
def test_closed_forms(gfa, name):
    V, edges, eps, mu, labels, letters = scan_cases.CLOSED[name]
    s, d = scan_cases.arrays(edges)
    with gfa.Graph(s, d, V) as g:
        label, role, nsim, summ, common = _check(g, scan_ref.prepare(V, s, d), eps, mu, name)
    assert label.tolist() == labels
    assert role.tolist() == scan_cases.roles(letters).tolist()
    assert [gfa.graph.SCAN_ROLES[r][0] for r in role] == list(letters)


# ---- 2. every row form at its boundaries ----
def _clique(n, first=0):
    iu, ju = np.triu_indices(n, 1)
    return (iu + first).astype(np.int32), (ju + first).astype(np.int32)


def _clique_want(n, mu):
    """K_n: every edge has n - 2 common neighbours and sigma = 1; one cluster of cores when mu <= n."""
    e = comb(n, 2)
    core = mu <= n
    return (np.zeros(n, np.int32) if core else np.arange(n, dtype=np.int32), np.full(n, 3 if core else 0, np.uint8),
            np.full(n, n - 1, np.int32),
            dict(simple_edges=e, triangles=comb(n, 3), similar_edges=e, n_clusters=int(core), n_cores=n if core else 0,
                 n_borders=0, n_hubs=0, n_outliers=0 if core else n, largest_cluster=n if core else 0,
                 largest_cluster_label=0 if core else -1),
            np.full(e, n - 2, np.int32))


def test_small_cliques_agree_with_the_reference(gfa):
    """The closed form the large cliques are held to, against the reference."""
    for n in (1, 2, 3, 7):
        s, d = _clique(n)
        want = _clique_want(n, 2)
        ref = scan_ref.scan(scan_ref.prepare(n, s, d), 0.9, 2)
        assert all(np.array_equal(a, b) for a, b in zip(ref[:3], want[:3])) and ref[3] == want[3]


# K_n orients every edge by id: the out-lists take every length 0 .. n - 1.  Defaults: group <= 8 <
# wave <= 1024 < block with the list in LDS.  Lowered: rows at L = boundary and boundary + 1 of
# every form, and lists that cross a team's chunk (64 lanes, 256 lanes).
@pytest.mark.parametrize("n, env", [
    (1030, {}),
    (300, {"LPA_TC_SHORT": "4", "LPA_TC_WAVE": "100", "LPA_TC_LDS": "200"}),
    (300, {"LPA_TC_SHORT": "0", "LPA_TC_WAVE": "299"}),
    (300, {"LPA_TC_SHORT": "0", "LPA_TC_WAVE": "0", "LPA_TC_LDS": "299"}),
    (300, {"LPA_TC_SHORT": "0", "LPA_TC_WAVE": "0", "LPA_TC_LDS": "0"}),
    (300, {"LPA_TC_SHORT": "299"}),
], ids=["K1030", "K300-four-forms", "K300-wave", "K300-block", "K300-global", "K300-group"])
def test_row_forms(gfa, monkeypatch, n, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, d = _clique(n)
    with gfa.Graph(s, d, n) as g:
        _same(g.scan(0.8, 3, stats=True, common=True), _clique_want(n, 3), f"K{n} {env}")
        if n == 300:
            _same(g.scan(1.0, n + 1, stats=True, common=True), _clique_want(n, n + 1), f"K{n} mu above n")


def _hub_edge():
    """A star plus a clique, with a second centre: 0 and 1 are adjacent to each other and to all
    of 2 .. N + 1, and 2 .. 41 form a clique.  Every leaf's triangle adds to the slot of 0 - 1."""
    N = 3000
    leaves = np.arange(2, N + 2)
    cs, cd = _clique(40, first=2)
    s = np.concatenate([[0], np.zeros(N, np.int64), np.ones(N, np.int64), cs]).astype(np.int32)
    d = np.concatenate([[1], leaves, leaves, cd]).astype(np.int32)
    return N + 2, s, d


@pytest.fixture(scope="module")
def hub_edge():
    V, s, d = _hub_edge()
    return V, s, d, scan_ref.prepare(V, s, d)


@pytest.mark.parametrize("env", [{}, {"LPA_TC_SHORT": "0"}, {"LPA_TC_SHORT": "0", "LPA_TC_WAVE": "0"},
                                 {"LPA_TC_SHORT": "0", "LPA_TC_WAVE": "0", "LPA_TC_LDS": "0"}],
                         ids=["defaults", "wave", "block", "global"])
def test_hub_edge(gfa, monkeypatch, hub_edge, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    V, s, d, prep = hub_edge
    assert prep.common_rows[0] == 3000
    with gfa.Graph(s, d, V) as g:
        for eps, mu in ((0.5, 2), (0.9, 3)):
            _check(g, prep, eps, mu, f"hub edge {env}")


# ---- 3. random graphs under relabelings ----
def _gnp(n, p, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    return n, iu[keep].astype(np.int32), ju[keep].astype(np.int32)


def _relabel(V, s, d, seed):
    perm = np.random.default_rng(seed).permutation(V).astype(np.int32)
    return V, perm[s], perm[d]


@pytest.fixture(scope="module")
def random_graphs(gfa):
    """G(300, p) below and above the density where eps = 0.5 still finds similar edges, R-MAT
    scale 11, and each under a random relabeling of the ids."""
    sparse, dense = _gnp(300, 0.012, 11), _gnp(300, 0.15, 12)
    rs, rd = gfa.gen_rmat(11, 16, seed=5)
    rmat = (1 << 11, rs.cpu().numpy(), rd.cpu().numpy())
    out = {"gnp-sparse": sparse, "gnp-sparse-relabelled": _relabel(*sparse, 1), "gnp-dense": dense,
           "gnp-dense-relabelled": _relabel(*dense, 2), "rmat11": rmat, "rmat11-relabelled": _relabel(*rmat, 3)}
    return {k: (V, s, d, scan_ref.prepare(V, s, d)) for k, (V, s, d) in out.items()}


@pytest.mark.parametrize("name", ["gnp-sparse", "gnp-sparse-relabelled", "gnp-dense", "gnp-dense-relabelled", "rmat11",
                                  "rmat11-relabelled"])
def test_random_graphs(gfa, random_graphs, name):
    V, s, d, prep = random_graphs[name]
    with gfa.Graph(s, d, V) as g:
        for eps in EPS:
            for mu in MU:
                _check(g, prep, eps, mu, name)


# ---- 4. invariance ----
def test_invariant_under_edge_order_direction_duplicates_and_loops(gfa, random_graphs):
    V, s, d, prep = random_graphs["rmat11"]
    eps, mu = 0.5, 3
    with gfa.Graph(s, d, V) as g:
        base = _check(g, prep, eps, mu)
        again = g.scan(eps, mu, stats=True, common=True)   # two calls on one handle
    _same(again, base, "second call")
    order = np.random.default_rng(4).permutation(s.size)
    with gfa.Graph(s[order], d[order], V) as g:
        got = g.scan(eps, mu, stats=True, common=True)
    _same(got, base[:4] + (base[4][order],), "shuffled")
    loops = np.arange(0, V, 3, dtype=np.int32)
    s2, d2 = np.concatenate([s, d, s, loops]), np.concatenate([d, s, d, loops])
    with gfa.Graph(s2, d2, V) as g:
        got = g.scan(eps, mu, stats=True, common=True)
    _same(got, base[:4] + (np.concatenate([base[4]] * 3 + [np.full(loops.size, -1, np.int32)]),), "multigraph")


# ---- 5. the rest of the handle is untouched ----
def test_does_not_disturb_other_calls(gfa, random_graphs):
    V, s, d, prep = random_graphs["rmat11"]
    with gfa.Graph(s, d, V) as g:
        want = g.run(3)
    with gfa.Graph(s, d, V) as g:
        tc = g.triangle_count(stats=True)
        cc = g.components()
        g.reset()
        g.step(1)
        before = g.info()["device_bytes"]
        got = _check(g, prep, 0.5, 2)
        assert g.info()["device_bytes"] == before   # nothing is kept on the handle
        g.step(2)
        assert np.array_equal(g.labels(), want)
        tc2 = g.triangle_count(stats=True)
        assert np.array_equal(tc2[0], tc[0]) and np.array_equal(tc2[1], tc[1]) and tc2[2] == tc[2]
        assert np.array_equal(g.components(), cc)
    assert got[3]["triangles"] == tc[2]["n_triangles"] and got[3]["simple_edges"] == tc[2]["simple_edges"]


# ---- 6. empty inputs ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        label, role, nsim, summ, common = g.scan(0.7, 2, stats=True, common=True)
    assert label.size == 0 and role.size == 0 and nsim.size == 0 and common.size == 0
    assert summ == dict(zip(scan_ref.SUMMARY_KEYS, [0] * 9 + [-1]))


def test_no_edges(gfa):
    e = np.empty(0, np.int32)
    prep = scan_ref.prepare(5, e, e)
    with gfa.Graph(e, e, 5) as g:
        a = _check(g, prep, 0.7, 2)
        b = _check(g, prep, 0.7, 1)   # mu = 1: every vertex a core of its own cluster
    assert a[1].tolist() == [0] * 5 and a[3]["n_outliers"] == 5 and a[3]["largest_cluster_label"] == -1
    assert b[1].tolist() == [3] * 5 and b[0].tolist() == list(range(5)) and b[3]["n_clusters"] == 5
    assert b[3]["largest_cluster"] == 1 and b[3]["largest_cluster_label"] == 0


def test_only_self_loops(gfa):
    v = np.array([3, 3, 0], np.int32)
    with gfa.Graph(v, v, 4) as g:
        got = _check(g, scan_ref.prepare(4, v, v), 0.5, 2)
    assert got[4].tolist() == [-1, -1, -1] and got[3]["simple_edges"] == 0


# ---- 7. device path ----
def test_device_tensors(gfa, random_graphs):
    import torch

    V, s, d, prep = random_graphs["rmat11"]
    want = scan_ref.scan(prep, 0.5, 3) + (prep.common_rows,)
    ts, td = torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda()
    with gfa.Graph(ts, td, V) as g:
        out = torch.full((V,), -1, dtype=torch.int32, device="cuda:0")
        label, role, nsim, summ, common = g.scan(0.5, 3, out=out, stats=True, common=True)
        assert label is out and role.is_cuda and role.dtype == torch.uint8
        assert nsim.is_cuda and nsim.dtype == torch.int32 and common.is_cuda and common.dtype == torch.int32
        _same((label.cpu().numpy(), role.cpu().numpy(), nsim.cpu().numpy(), summ, common.cpu().numpy()), want, "device")
        label, role = g.scan(0.5, 3, out=out)
        assert label is out and np.array_equal(role.cpu().numpy(), want[1])
        with pytest.raises(ValueError, match="int32"):
            g.scan(0.5, 3, out=torch.empty(V, dtype=torch.int64, device="cuda:0"))
        with pytest.raises(ValueError, match=f"{V}"):
            g.scan(0.5, 3, out=torch.empty(V + 1, dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError, match="device tensor"):
            g.scan(0.5, 3, out=np.empty(V, np.int32))


# ---- 8. GraphFrame ----
def test_graphframe_string_ids(gfa, golden):
    """String ids: labels are dense indices in ascending id order, as labelPropagation's."""
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    prep = scan_ref.prepare(ig.num_vertices, ig.src, ig.dst)
    rlabel, rrole, _, rsumm = scan_ref.scan(prep, 0.5, 3)
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.scan(0.5, 3)
        sim = gf.structuralSimilarity()
        scores = gf.outlierScores(labels=out)
    finally:
        gf.close()
    assert list(out.columns) == ["id", "name", "label", "role"] and out["label"].dtype == np.int64
    assert np.array_equal(out["id"].to_numpy(), ig.ids)
    assert np.array_equal(out["label"].to_numpy(), rlabel)
    assert out["role"].tolist() == [scan_ref.ROLES[r] for r in rrole]
    assert {k: out.attrs[k] for k in scan_ref.SUMMARY_KEYS} == rsumm
    assert set(out["role"]) == {"core", "border", "hub", "outlier"}
    assert np.array_equal(scores.vertices["label"].to_numpy(), rlabel)   # outlierScores takes the labels
    assert list(sim.columns) == ["src", "dst", "common", "similarity"] and len(sim) == len(e)
    assert sim["common"].dtype == np.int64 and sim["similarity"].dtype == np.float64
    assert np.array_equal(sim["common"].to_numpy(), prep.common_rows)
    assert out.equals(gfa.scan(v, e, 0.5, 3))


def test_graphframe_integral_ids(gfa):
    """The bridged triangles with ids 10 x: labels are original ids; rows that are no edges."""
    V, edges, eps, mu, labels, letters = scan_cases.CLOSED["bridged-0.75"]
    s, d = scan_cases.arrays(edges)
    v = pd.DataFrame({"id": 10 * np.arange(V, dtype=np.int64)[::-1], "tag": list("hgfedcba")})
    e = pd.DataFrame({"src": np.concatenate([10 * s.astype(np.int64), [20, 30, 999]]),
                      "dst": np.concatenate([10 * d.astype(np.int64), [20, 5, 0]]), "w": np.arange(12.0)})
    out = gfa.scan(v, e, epsilon=eps, mu=mu)
    assert out["id"].tolist() == [10 * i for i in range(V)] and out["tag"].tolist() == list("abcdefgh")
    assert out["label"].tolist() == [10 * x for x in labels]
    assert out["role"].tolist() == ["core"] * 6 + ["hub", "outlier"]
    assert out.attrs["n_clusters"] == 2 and out.attrs["largest_cluster_label"] == 0 and out.attrs["n_hubs"] == 1
    sim = gfa.structural_similarity(v, e)
    # the two rows with an end that is no vertex id are dropped; the self-loop row stays, as no edge
    assert list(sim.columns) == ["src", "dst", "w", "common", "similarity"] and sim["w"].tolist() == list(np.arange(10.0))
    assert sim["common"].tolist() == [1] * 6 + [0, 0, 0, -1]
    assert np.isnan(sim["similarity"].iloc[-1])
    deg = np.array([3, 2, 2, 3, 2, 2, 3, 1], np.float64)
    want = (sim["common"].to_numpy()[:9] + 2.0) / np.sqrt((deg[s] + 1) * (deg[d] + 1))
    assert np.array_equal(sim["similarity"].to_numpy()[:9], want)
    none = gfa.scan(v, e, epsilon=1.0, mu=9)
    assert none.attrs["largest_cluster_label"] is None and set(none["role"]) == {"outlier"}


# ---- 9. partitioned job: rank 0 keeps the edge list ----
def test_two_loopback_ranks(gfa, hub_edge):
    V, s, d, prep = hub_edge
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        _check(ranks[0], prep, 0.5, 2)
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].scan(0.5, 2)
    finally:
        for g in ranks:
            g.close()
        lb.close()
