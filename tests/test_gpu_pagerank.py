"""Static PageRank on the GPU (lpa_pagerank, csrc/lpa_pr.hip) against the numpy reference
tests/pr_ref.py: |gpu - ref| <= bound * ref per vertex with bound = pr_ref.bound(k, D, V)
computed from the case (k supersteps, largest in-degree D, V vertices), the same zero
pattern, exact degrees and summary integers; bit-identical ranks across edge orders and
calls.  Drop-in calls: GraphFrame.pageRank / inDegrees / outDegrees, page_rank."""
import numpy as np
import pandas as pd
import pytest

import pr_ref
from graphs import degree_mix, random_multigraph, star

pytestmark = pytest.mark.gpu

KS = (1, 5, 20)
# the create-time overrides of the row-form boundaries (DESIGN.md "PageRank")
PR_OVERRIDES = [{}, {"LPA_PR_SHORT": "0"}, {"LPA_PR_WAVE": "0"}, {"LPA_PR_SHORT": "0", "LPA_PR_WAVE": "0"},
                {"LPA_PR_SHORT": "100000"}]
PR_IDS = ["defaults", "short0", "wave0", "both0", "all-short"]


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _compare(got, ref, k, unique_max=True):
    """One stats=True result against one reference result; returns the bound used."""
    rank, odeg, ideg, summ = got
    rrank, rodeg, rideg, rS = ref
    V = rrank.size
    assert rank.dtype == np.float64 and rank.shape == (V,)
    assert odeg.dtype == np.int64 and np.array_equal(odeg, rodeg)
    assert ideg.dtype == np.int64 and np.array_equal(ideg, rideg)
    b = pr_ref.bound(k, int(rideg.max()) if V else 0, V)
    err = np.abs(rank - rrank)
    worst = float(np.max(err / np.where(rrank > 0, rrank, 1.0))) if V else 0.0
    print(f"V={V} k={k} D={int(rideg.max()) if V else 0} bound={b:.3e} worst relative difference={worst:.3e}")
    assert (err <= b * rrank).all(), f"relative difference {worst:.3e} above the bound {b:.3e}"
    assert np.array_equal(rank == 0.0, rrank == 0.0)
    rsumm = pr_ref.summary(rrank, rodeg, rideg, rS)
    for key in ("edges", "sinks", "max_in_degree"):
        assert summ[key] == rsumm[key], key
    assert abs(summ["rank_sum"] - rS) <= b * rS
    assert abs(summ["max_rank"] - rsumm["max_rank"]) <= b * rsumm["max_rank"]
    # the library's own maximum, exactly; the reference's vertex where the maximum is one vertex's
    top = float(rank.max()) if V else 0.0
    assert summ["max_rank"] == top and summ["max_rank_id"] == (int(np.flatnonzero(rank == top)[0]) if V else -1)
    if unique_max:
        assert summ["max_rank_id"] == rsumm["max_rank_id"]
    return b


def _check(gfa, V, s, d, k, a=0.15, source=None, unique_max=True, g=None):
    """pagerank() plain and with stats (of a fresh handle unless g is given) against the reference."""
    s = np.asarray(s, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    ref = pr_ref.pagerank(V, s, d, k, a, source)
    own = g is None
    if own:
        g = gfa.Graph(s, d, V)
    try:
        rank = g.pagerank(k, a, source)
        got = g.pagerank(k, a, source, stats=True)
    finally:
        if own:
            g.close()
    assert np.array_equal(rank, got[0])
    _compare(got, ref, k, unique_max)
    return got


# ---- 1. degenerate ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        assert g.pagerank(3).size == 0
        rank, odeg, ideg, summ = g.pagerank(3, stats=True)
    assert rank.size == 0 and odeg.size == 0 and ideg.size == 0
    assert summ == dict(rank_sum=0.0, max_rank=0.0, max_rank_id=-1, edges=0, sinks=0, max_in_degree=0)


def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    for k in KS:
        rank, _, _, summ = _check(gfa, 1, e, e, k)
        assert rank.tolist() == [1.0]
        assert summ == dict(rank_sum=0.15, max_rank=1.0, max_rank_id=0, edges=0, sinks=1, max_in_degree=0)


def test_edgeless(gfa):
    """Every raw rank is a: the normalised ranks are a * (70 / S), 1.0 to within the sum's rounding."""
    e = np.empty(0, np.int32)
    rank, _, _, summ = _check(gfa, 70, e, e, 5, unique_max=False)
    assert (np.abs(rank - 1.0) <= pr_ref.bound(5, 0, 70)).all() and np.unique(rank).size == 1
    assert summ["sinks"] == 70 and summ["edges"] == 0 and summ["max_rank_id"] == 0


def test_only_self_loops(gfa):
    v = np.array([3, 3, 0, 99, 64, 64, 64], np.int32)
    for k in KS:
        _, odeg, ideg, summ = _check(gfa, 100, v, v, k, unique_max=False)
        assert summ["edges"] == 7 and summ["sinks"] == 96 and summ["max_in_degree"] == 3
        assert np.array_equal(odeg, ideg)


def test_one_edge_repeated(gfa):
    s, d = np.full(1000, 6, np.int32), np.full(1000, 2, np.int32)
    for k in KS:
        rank, odeg, ideg, summ = _check(gfa, 9, s, d, k)
        assert odeg[6] == 1000 and ideg[2] == 1000 and summ["edges"] == 1000 and summ["max_rank_id"] == 2
        once, _, _, _ = pr_ref.pagerank(9, [6], [2], k)
        assert (np.abs(rank - once) <= pr_ref.bound(k, 1000, 9) * once).all()


# ---- 2. closed forms ----
def test_directed_cycle(gfa):
    n = 1000
    i = np.arange(n)
    for k in KS:
        rank, _, _, summ = _check(gfa, n, i, (i + 1) % n, k, unique_max=False)
        assert (rank == 1.0).all() and summ["rank_sum"] == n and summ["max_rank_id"] == 0 and summ["sinks"] == 0


def test_cycle_without_reset(gfa):
    n = 1000
    i = np.arange(n)
    rank, _, _, summ = _check(gfa, n, i, (i + 1) % n, 5, a=0.0, unique_max=False)
    assert (rank == 1.0).all() and summ["rank_sum"] == n
    # from one vertex the whole mass walks five steps on
    rank, _, _, _ = _check(gfa, n, i, (i + 1) % n, 5, a=0.0, source=998)
    assert rank[3] == 1.0 and np.count_nonzero(rank) == 1


def test_complete_digraph(gfa):
    n = 70
    a, b = np.nonzero(~np.eye(n, dtype=bool))
    for k in KS:
        rank, _, ideg, _ = _check(gfa, n, a, b, k, unique_max=False)
        assert (ideg == n - 1).all() and (np.abs(rank - 1.0) <= pr_ref.bound(k, n - 1, n)).all()


def test_star_out(gfa):
    """star(5000) as given: the hub points at 5000 sinks, every in-degree is 1 or 0."""
    V, s, d = star(5000)
    for k in KS:
        rank, _, _, summ = _check(gfa, V, s, d, k)
        assert summ["sinks"] == 5000 and summ["max_in_degree"] == 1 and summ["max_rank_id"] == 1
        assert np.unique(rank[1:]).size == 1


def test_star_in(gfa):
    """The star reversed: one row of in-degree 5000, the block form; closed form
    raw r[0] = a + (1 - a) 5000 a from superstep 2 on (the leaves hold a)."""
    V, d, s = star(5000)
    for k in KS:
        rank, _, _, summ = _check(gfa, V, s, d, k)
        assert summ["sinks"] == 1 and summ["max_in_degree"] == 5000 and summ["max_rank_id"] == 0
    hub = 0.15 + 0.85 * (5000 * 0.15)
    S = hub + 5000 * 0.15
    assert abs(rank[0] - hub * V / S) <= pr_ref.bound(20, 5000, V) * rank[0]


def test_two_vertices_one_edge(gfa):
    """0 -> 1: raw (0.15, 1.0) after superstep 1, (0.15, 0.2775) after every later one."""
    rank, _, _, summ = _check(gfa, 2, [0], [1], 1)
    assert abs(summ["rank_sum"] - 1.15) <= pr_ref.bound(1, 1, 2) * 1.15
    for k in (2, 5, 20):
        rank, _, _, summ = _check(gfa, 2, [0], [1], k)
        b = pr_ref.bound(k, 1, 2)
        assert abs(summ["rank_sum"] - 0.4275) <= b * 0.4275
        for got, raw in zip(rank.tolist(), (0.15, 0.2775)):
            assert abs(got - raw * 2 / 0.4275) <= b * got


def test_reset_probability_one(gfa):
    V, s, d = random_multigraph(300, 2000, 1)
    for k in KS:
        rank, _, _, summ = _check(gfa, V, s, d, k, a=1.0, unique_max=False)
        assert (rank == 1.0).all() and summ["rank_sum"] == V and summ["max_rank_id"] == 0
        rank, _, _, summ = _check(gfa, V, s, d, k, a=1.0, source=4)
        assert rank[4] == 1.0 and np.count_nonzero(rank) == 1 and summ["max_rank_id"] == 4


# ---- 3. every boundary of the row forms ----
# The transitive tournament u -> v for u < v on B + 2 vertices has in-degree v at vertex v:
# every length 0 .. B + 1.  Defaults: short <= 32 < wave <= 1024 < block; B = 1024.
@pytest.fixture(scope="module")
def tournament():
    n = 1026
    s, d = np.triu_indices(n, 1)
    s, d = s.astype(np.int32), d.astype(np.int32)
    refs = {(k, src): pr_ref.pagerank(n, s, d, k, 0.15, src) for k in KS for src in (None, 0)}
    for ref in refs.values():
        for a in ref[:3]:
            a.setflags(write=False)
    return n, s, d, refs


@pytest.mark.parametrize("env", PR_OVERRIDES, ids=PR_IDS)
def test_form_boundaries(gfa, monkeypatch, tournament, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    n, s, d, refs = tournament
    with gfa.Graph(s, d, n) as g:
        for (k, src), ref in refs.items():
            got = g.pagerank(k, 0.15, src, stats=True)
            _compare(got, ref, k)
            assert np.array_equal(got[2], np.arange(n)) and got[3]["max_in_degree"] == n - 1


# ---- 4. mixed graphs ----
def _mixed(gfa, V, s, d, source):
    with gfa.Graph(s, d, V) as g:
        for k in KS:
            for src in (None, source):
                _check(gfa, V, s, d, k, source=src, g=g)


def test_r9_sample(gfa, golden):
    V = int(golden["ids"].size)
    s, d = golden["src"], golden["dst"]
    outdeg, indeg = pr_ref.degrees(V, s, d)
    assert int((outdeg == 0).sum()) == 3917 and int(indeg.max()) == 1223
    _mixed(gfa, V, s, d, int(np.argmax(outdeg)))


@pytest.mark.parametrize("env", PR_OVERRIDES, ids=PR_IDS)
def test_degree_mix_under_overrides(gfa, monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    V, s, d = degree_mix()
    _mixed(gfa, V, s, d, int(s[0]))


@pytest.fixture(scope="module")
def dense_random():
    return random_multigraph(2000, 60000, 7)


def test_dense_random(gfa, dense_random):
    V, s, d = dense_random
    _mixed(gfa, V, s, d, 17)


def test_sparse_random(gfa):
    V, s, d = random_multigraph(20000, 200000, 3)
    _mixed(gfa, V, s, d, int(s[5]))


# ---- 5. determinism ----
def test_bit_identical_across_edge_orders(gfa, dense_random):
    V, s, d = dense_random
    m = s.size
    perm = np.random.default_rng(9).permutation(m)
    # duplicates are neighbours after a sort by (src, dst); a stride coprime to m moves them apart
    by_key = np.lexsort((d, s))
    stride = 7919
    assert np.gcd(stride, m) == 1
    apart = by_key[(np.arange(m, dtype=np.int64) * stride) % m]
    assert np.array_equal(np.sort(apart), np.arange(m))
    got = []
    for order in (np.arange(m), np.arange(m)[::-1], perm, apart):
        with gfa.Graph(s[order].copy(), d[order].copy(), V) as g:
            got.append([g.pagerank(k, 0.15, src, stats=True) for k in (5, 20) for src in (None, 17)])
    for other in got[1:]:
        for (r0, o0, i0, s0), (r1, o1, i1, s1) in zip(got[0], other):
            assert np.array_equal(r0, r1) and np.array_equal(o0, o1) and np.array_equal(i0, i1) and s0 == s1


def test_bit_identical_across_calls_and_direction_matters(gfa, dense_random):
    V, s, d = dense_random
    with gfa.Graph(s, d, V) as g:
        r1 = g.pagerank(20)
        r2 = g.pagerank(20)
    assert np.array_equal(r1, r2)
    with gfa.Graph(d, s, V) as g:
        rev = g.pagerank(20)
    assert not np.array_equal(rev, r1)
    rrev, _, _, _ = pr_ref.pagerank(V, d, s, 20)
    assert (np.abs(rev - rrev) <= pr_ref.bound(20, int(np.bincount(s).max()), V) * rrev).all()


# ---- 6. device path ----
def test_device_tensors(gfa):
    import torch

    scale = 14
    V = 1 << scale
    s, d = gfa.gen_rmat(scale, 16, seed=1)
    k = 5
    ref = pr_ref.pagerank(V, s.cpu().numpy(), d.cpu().numpy(), k)
    with gfa.Graph(s, d, V) as g:
        out = torch.full((V,), -1.0, dtype=torch.float64, device=s.device)
        assert g.pagerank(k, out=out) is out
        first = out.cpu().numpy()
        out.fill_(-1.0)
        rank, odeg, ideg, summ = g.pagerank(k, out=out, stats=True)
        assert rank is out and odeg.is_cuda and ideg.is_cuda and odeg.dtype == torch.int64 and ideg.dtype == torch.int64
        assert np.array_equal(out.cpu().numpy(), first)
        _compare((out.cpu().numpy(), odeg.cpu().numpy(), ideg.cpu().numpy(), summ), ref, k)
        assert np.array_equal(g.pagerank(k), first)   # host output of the same handle
        with pytest.raises(ValueError, match="float64"):
            g.pagerank(k, out=torch.empty(V, dtype=torch.float32, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.pagerank(k, out=torch.empty(V - 1, dtype=torch.float64, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.pagerank(k, out=torch.empty(V + 1, dtype=torch.float64, device=s.device))
        with pytest.raises(ValueError, match="contiguous"):
            g.pagerank(k, out=torch.empty(2 * V, dtype=torch.float64, device=s.device)[::2])
        with pytest.raises(ValueError, match="device tensor"):
            g.pagerank(k, out=np.empty(V, np.float64))
        # the C ABI's own argument checks
        with pytest.raises(ValueError, match="max_iter"):
            g.pagerank(0)
        with pytest.raises(ValueError, match="reset_prob"):
            g.pagerank(3, 1.5)
        with pytest.raises(ValueError, match="reset_prob"):
            g.pagerank(3, float("nan"))
        with pytest.raises(ValueError, match="source"):
            g.pagerank(3, source=V)


# ---- 7. the LPA state is untouched ----
def test_does_not_disturb_lpa(gfa):
    V, s, d = degree_mix()
    ref = pr_ref.pagerank(V, s, d, 5)
    with gfa.Graph(s, d, V) as g:
        want = g.run(3)
    with gfa.Graph(s, d, V) as g:
        g.reset()
        g.step(1)
        before = g.info()["device_bytes"]
        r1 = g.pagerank(5)
        assert g.info()["device_bytes"] == before
        g.step(1)
        got2 = g.pagerank(5, stats=True)
        assert g.info()["device_bytes"] == before
        g.step(1)
        got = g.labels()
    assert np.array_equal(got, want)
    assert np.array_equal(r1, got2[0])
    _compare(got2, ref, 5)


# ---- 8. drop-in ----
def test_graphframe_string_ids(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    rrank, routdeg, rindeg, _ = pr_ref.pagerank(ig.num_vertices, ig.src, ig.dst, 5)
    gf = gfa.GraphFrame(v, e)
    try:
        res = gf.pageRank(maxIter=5)
        ind, outd = gf.inDegrees(), gf.outDegrees()
    finally:
        gf.close()
    assert isinstance(res, gfa.GraphFrame)
    out = res.vertices
    assert list(out.columns) == ["id", "name", "pagerank"] and out["pagerank"].dtype == np.float64
    assert np.array_equal(out["id"].to_numpy(), ig.ids)
    b = pr_ref.bound(5, int(rindeg.max()), ig.num_vertices)
    assert (np.abs(out["pagerank"].to_numpy() - rrank) <= b * rrank).all()
    ed = res.edges
    assert list(ed.columns) == ["src", "dst", "weight"] and ed["weight"].dtype == np.float64 and len(ed) == len(e)
    assert np.array_equal(ed["src"].to_numpy(), e["src"].to_numpy()) and np.array_equal(ed["dst"].to_numpy(), e["dst"].to_numpy())
    assert np.array_equal(ed["weight"].to_numpy(), 1.0 / routdeg[ig.src])
    assert list(ind.columns) == ["id", "name", "inDegree"] and ind["inDegree"].dtype == np.int64
    assert list(outd.columns) == ["id", "name", "outDegree"] and outd["outDegree"].dtype == np.int64
    assert np.array_equal(ind["inDegree"].to_numpy(), np.bincount(ig.dst, minlength=ig.num_vertices))
    assert np.array_equal(outd["outDegree"].to_numpy(), np.bincount(ig.src, minlength=ig.num_vertices))
    assert out.equals(gfa.page_rank(v, e, 5))


def test_graphframe_integral_ids(gfa):
    """10 -> 20 -> 30 -> 10, 40 -> 10, and a dangling 40 -> 99."""
    v = pd.DataFrame({"id": np.array([30, 10, 20, 40], np.int64), "name": ["c", "a", "b", "d"]})
    e = pd.DataFrame({"src": np.array([10, 20, 40, 30, 40], np.int64), "dst": np.array([20, 30, 99, 10, 10], np.int64)})
    gf = gfa.GraphFrame(v, e)
    try:
        res = gf.pageRank(maxIter=5)
        pers = gf.pageRank(maxIter=2, sourceId=10)
        outd = gf.outDegrees()
        with pytest.raises(ValueError, match="sourceId"):
            gf.pageRank(maxIter=5, sourceId=99)
    finally:
        gf.close()
    assert res.edges["src"].tolist() == [10, 20, 30, 40] and res.edges["dst"].tolist() == [20, 30, 10, 10]
    assert res.edges["weight"].tolist() == [1.0, 1.0, 1.0, 1.0]
    assert dict(zip(outd["id"].tolist(), outd["outDegree"].tolist())) == {10: 1, 20: 1, 30: 1, 40: 1}
    rrank, _, _, _ = pr_ref.pagerank(4, [0, 1, 2, 3], [1, 2, 0, 0], 5)
    got = res.vertices
    assert got["id"].tolist() == [10, 20, 30, 40] and got["name"].tolist() == ["a", "b", "c", "d"]
    assert (np.abs(got["pagerank"].to_numpy() - rrank) <= pr_ref.bound(5, 2, 4) * rrank).all()
    # two supersteps from 10 reach 20 and 30; 40 is never reached
    p = pers.vertices["pagerank"].to_numpy()
    prank, _, _, _ = pr_ref.pagerank(4, [0, 1, 2, 3], [1, 2, 0, 0], 2, source=0)
    assert (p == 0.0).tolist() == [False, False, False, True] and np.array_equal(p == 0.0, prank == 0.0)
    assert (np.abs(p - prank) <= pr_ref.bound(2, 2, 4) * prank).all() and abs(p.sum() - 1.0) <= 4 * 2.0 ** -52


# ---- 9. partitioned job: rank 0 keeps the edge list ----
def test_two_loopback_ranks(gfa):
    V, s, d = degree_mix()
    with gfa.Graph(s, d, V) as g:
        single = g.pagerank(5, stats=True)
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        rank, odeg, ideg, summ = ranks[0].pagerank(5, stats=True)
        assert np.array_equal(rank, single[0]) and np.array_equal(odeg, single[1]) and np.array_equal(ideg, single[2])
        assert summ == single[3]
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].pagerank(5)
    finally:
        for g in ranks:
            g.close()
        lb.close()
