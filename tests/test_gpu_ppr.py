"""Parallel personalized PageRank on the GPU (lpa_parallel_pagerank, csrc/lpa_ppr.hip): every
column against the per-source numpy reference pr_ref.pagerank(..., source=x) --
|gpu - ref| <= bound * ref per vertex with bound = pr_ref.bound(k, D, V) computed from the case,
the same zero pattern, the sums within the bound, exact summary integers; columns bit-identical
across edge orders, calls, positions in the source list and company.  No test knows the default
batch width: W is read from summary["batch_width"].  Drop-in calls:
GraphFrame.parallelPersonalizedPageRank, parallel_personalized_page_rank."""
import numpy as np
import pandas as pd
import pytest

import pr_ref
from graphs import degree_mix, random_multigraph
from ppr_ref import degree_mix_sources, tournament_sources

pytestmark = pytest.mark.gpu

KS = (1, 5, 20)
# the create-time overrides of the row-form boundaries (DESIGN.md "PageRank"), as test_gpu_pagerank.py's
PR_OVERRIDES = [{}, {"LPA_PR_SHORT": "0"}, {"LPA_PR_WAVE": "0"}, {"LPA_PR_SHORT": "0", "LPA_PR_WAVE": "0"},
                {"LPA_PR_SHORT": "100000"}]
PR_IDS = ["defaults", "short0", "wave0", "both0", "all-short"]


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


class Refs:
    """pr_ref.pagerank per (k, a, source) of one graph, each computed once and read-only."""

    def __init__(self, V, s, d):
        self.V, self.s, self.d = V, np.asarray(s, np.int32), np.asarray(d, np.int32)
        self.outdeg, self.indeg = pr_ref.degrees(V, s, d)
        self._got = {}

    def get(self, k, a, x):
        key = (k, a, int(x))
        if key not in self._got:
            rank, _, _, S = pr_ref.pagerank(self.V, self.s, self.d, k, a, int(x))
            rank.setflags(write=False)
            self._got[key] = (rank, S)
        return self._got[key]


def _compare(got, refs, sources, k, a=0.15):
    """One stats=True result against the per-source references; returns W."""
    ranks, sums, summ = got
    V, n = refs.V, len(sources)
    ranks = ranks.cpu().numpy() if hasattr(ranks, "cpu") else ranks
    assert ranks.dtype == np.float64 and ranks.shape == (n, V)
    assert sums.dtype == np.float64 and sums.shape == (n,)
    D = int(refs.indeg.max()) if V else 0
    b = pr_ref.bound(k, D, V)
    worst, nonzero = 0.0, 0
    for l, x in enumerate(sources):
        rrank, rS = refs.get(k, a, x)
        err = np.abs(ranks[l] - rrank)
        worst = max(worst, float(np.max(err / np.where(rrank > 0, rrank, 1.0))))
        assert (err <= b * rrank).all(), f"column {l} (source {x}): relative difference {worst:.3e} above {b:.3e}"
        assert np.array_equal(ranks[l] == 0.0, rrank == 0.0), f"column {l} (source {x}): zero pattern"
        assert abs(sums[l] - rS) <= b * rS, f"column {l} (source {x}): S"
        nonzero += int(np.count_nonzero(rrank))
    print(f"V={V} k={k} D={D} n={n} W={summ['batch_width']} bound={b:.3e} worst relative difference={worst:.3e}")
    W = summ["batch_width"]
    assert W in (4, 8, 16)
    assert summ["edges"] == int(refs.outdeg.sum()) and summ["sinks"] == int((refs.outdeg == 0).sum())
    assert summ["max_in_degree"] == D
    assert summ["nonzero"] == nonzero and summ["batches"] == -(-n // W)
    assert summ["rank_sum_min"] == float(sums.min()) and summ["rank_sum_max"] == float(sums.max())
    return W


def _check(gfa, refs, sources, k, a=0.15, g=None):
    """parallel_pagerank() plain and with stats (of a fresh handle unless g is given)."""
    own = g is None
    if own:
        g = gfa.Graph(refs.s, refs.d, refs.V)
    try:
        ranks = g.parallel_pagerank(sources, k, a)
        got = g.parallel_pagerank(sources, k, a, stats=True)
    finally:
        if own:
            g.close()
    assert np.array_equal(ranks, got[0])
    _compare(got, refs, sources, k, a)
    return got


ZEROS = dict(edges=0, sinks=0, max_in_degree=0, batches=0, batch_width=0, nonzero=0, rank_sum_min=0.0,
             rank_sum_max=0.0)


# ---- 1. degenerate ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        assert g.parallel_pagerank([], 3).shape == (0, 0)
        ranks, sums, summ = g.parallel_pagerank([], 3, stats=True)
        with pytest.raises(ValueError, match="source"):
            g.parallel_pagerank([0], 3)
    assert ranks.shape == (0, 0) and sums.shape == (0,) and summ == ZEROS


def test_no_sources(gfa):
    V, s, d = random_multigraph(300, 2000, 1)
    outdeg, indeg = pr_ref.degrees(V, s, d)
    with gfa.Graph(s, d, V) as g:
        assert g.parallel_pagerank([], 3).shape == (0, V)
        ranks, sums, summ = g.parallel_pagerank([], 3, stats=True)
    assert ranks.shape == (0, V) and ranks.dtype == np.float64 and sums.shape == (0,)
    assert summ == dict(ZEROS, edges=2000, sinks=int((outdeg == 0).sum()), max_in_degree=int(indeg.max()))


def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    refs = Refs(1, e, e)
    for k in KS:
        ranks, sums, summ = _check(gfa, refs, [0, 0, 0], k)
        assert ranks.tolist() == [[1.0]] * 3 and sums.tolist() == [0.15] * 3
        assert summ["sinks"] == 1 and summ["edges"] == 0 and summ["nonzero"] == 3


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    refs = Refs(70, e, e)
    ranks, sums, summ = _check(gfa, refs, [69, 0, 33], 5)
    assert np.array_equal(ranks, np.eye(70)[[69, 0, 33]]) and (sums == 0.15).all()
    assert summ["sinks"] == 70 and summ["nonzero"] == 3


def test_sink_source(gfa):
    V, s, d = random_multigraph(300, 600, 2)
    refs = Refs(V, s, d)
    sink = int(np.flatnonzero(refs.outdeg == 0)[0])
    for k in KS:
        ranks, sums, _ = _check(gfa, refs, [3, sink], k, 0.25)
        assert ranks[1, sink] == 1.0 and np.count_nonzero(ranks[1]) == 1 and sums[1] == 0.25


def test_reset_probability_one(gfa):
    V, s, d = random_multigraph(300, 2000, 1)
    refs = Refs(V, s, d)
    for k in KS:
        ranks, sums, summ = _check(gfa, refs, [4, 299, 0], k, 1.0)
        assert np.array_equal(ranks, np.eye(V)[[4, 299, 0]]) and (sums == 1.0).all() and summ["nonzero"] == 3


def test_cycle_without_reset(gfa):
    """From one vertex of a directed cycle the whole mass walks k steps on."""
    n = 1000
    i = np.arange(n)
    refs = Refs(n, i, (i + 1) % n)
    ranks, sums, summ = _check(gfa, refs, [998, 0], 5, 0.0)
    assert ranks[0, 3] == 1.0 and ranks[1, 5] == 1.0 and summ["nonzero"] == 2 and (sums == 1.0).all()


# ---- 2. batch edges ----
@pytest.fixture(scope="module")
def dense_random():
    V, s, d = random_multigraph(2000, 60000, 7)
    return Refs(V, s, d)


@pytest.fixture(scope="module")
def default_width(gfa):
    """The width of a handle created without LPA_PPR_BATCH."""
    import os

    saved = os.environ.pop("LPA_PPR_BATCH", None)
    try:
        e = np.zeros(1, np.int32)
        with gfa.Graph(e, e, 1) as g:
            return g.parallel_pagerank([0], 1, stats=True)[2]["batch_width"]
    finally:
        if saved is not None:
            os.environ["LPA_PPR_BATCH"] = saved


@pytest.mark.parametrize("batch", ["4", "8", "16", "5"])
def test_batch_edges(gfa, monkeypatch, dense_random, default_width, batch):
    monkeypatch.setenv("LPA_PPR_BATCH", batch)
    refs = dense_random
    W = default_width if batch == "5" else int(batch)   # an illegal value selects the default
    order = np.random.default_rng(4).permutation(refs.V)
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        for n in (1, W - 1, W, W + 1, 2 * W + 3):
            sources = [int(x) for x in order[:n]]
            got = g.parallel_pagerank(sources, 5, stats=True)
            assert _compare(got, refs, sources, 5) == W


# ---- 3. every row length across both form boundaries ----
# The transitive tournament u -> v for u < v on B + 2 vertices has in-degree v at vertex v:
# every length 0 .. B + 1.  Defaults: short <= 32 < wave <= 1024 < block; B = 1024.
@pytest.fixture(scope="module")
def tournament():
    n = 1026
    s, d = np.triu_indices(n, 1)
    return Refs(n, s, d)


@pytest.mark.parametrize("env", PR_OVERRIDES, ids=PR_IDS)
def test_form_boundaries(gfa, monkeypatch, tournament, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    refs, sources = tournament, tournament_sources()
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        for k in KS:
            got = g.parallel_pagerank(sources, k, stats=True)
            _compare(got, refs, sources, k)
            assert got[2]["max_in_degree"] == refs.V - 1
            assert sources[2] == sources[13] and np.array_equal(got[0][2], got[0][13])   # the repeat


@pytest.mark.parametrize("batch", ["4", "8", "16"])
def test_form_boundaries_at_every_width(gfa, monkeypatch, tournament, batch):
    """Every row length through the three forms of every instantiated width."""
    monkeypatch.setenv("LPA_PPR_BATCH", batch)
    refs, sources = tournament, tournament_sources()
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        assert _compare(g.parallel_pagerank(sources, 5, stats=True), refs, sources, 5) == int(batch)


# ---- 4. a block-form row whose terms all carry mass ----
def test_fan(gfa):
    """0 -> i for i in 1 .. 5000, i -> 5001, 5001 -> 0: from 0, row 5001 sums 5000 positive terms."""
    leaves = np.arange(1, 5001)
    s = np.concatenate([np.zeros(5000, np.int64), leaves, [5001]])
    d = np.concatenate([leaves, np.full(5000, 5001), [0]])
    refs = Refs(5002, s, d)
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        for k in KS:
            ranks, _, summ = _check(gfa, refs, [0, 5001, 17], k, g=g)
            assert summ["max_in_degree"] == 5000 and summ["sinks"] == 0
            if k >= 2:
                assert ranks[0, 5001] > 0.0 and np.unique(ranks[0, 1:5001]).size == 1


# ---- 5. mixed graphs ----
@pytest.fixture(scope="module")
def mix():
    V, s, d = degree_mix()
    return Refs(V, s, d), degree_mix_sources(V, s, d)


@pytest.mark.parametrize("env", PR_OVERRIDES, ids=PR_IDS)
def test_degree_mix_under_overrides(gfa, monkeypatch, mix, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    refs, sources = mix
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        for k in KS:
            _check(gfa, refs, sources, k, g=g)


def test_r9_sample(gfa, golden):
    V = int(golden["ids"].size)
    refs = Refs(V, golden["src"], golden["dst"])
    assert int((refs.outdeg == 0).sum()) == 3917 and int(refs.indeg.max()) == 1223
    rest = np.random.default_rng(5).choice(V, size=14, replace=False)
    sources = [int(np.argmax(refs.outdeg)), int(np.argmax(refs.indeg)), int(np.flatnonzero(refs.outdeg == 0)[0])]
    sources += [int(x) for x in rest]
    with gfa.Graph(refs.s, refs.d, V) as g:
        for k in KS:
            _check(gfa, refs, sources, k, g=g)


# ---- 6. determinism ----
def test_bit_identical_across_edge_orders(gfa, dense_random):
    refs = dense_random
    V, s, d = refs.V, refs.s, refs.d
    m = s.size
    perm = np.random.default_rng(9).permutation(m)
    # duplicates are neighbours after a sort by (src, dst); a stride coprime to m moves them apart
    by_key = np.lexsort((d, s))
    stride = 7919
    assert np.gcd(stride, m) == 1
    apart = by_key[(np.arange(m, dtype=np.int64) * stride) % m]
    assert np.array_equal(np.sort(apart), np.arange(m))
    sources = list(range(0, 2000, 59))
    got = []
    for order in (np.arange(m), np.arange(m)[::-1], perm, apart):
        with gfa.Graph(s[order].copy(), d[order].copy(), V) as g:
            got.append([g.parallel_pagerank(sources, k, stats=True) for k in (5, 20)])
    for other in got[1:]:
        for (r0, s0, m0), (r1, s1, m1) in zip(got[0], other):
            assert np.array_equal(r0, r1) and np.array_equal(s0, s1) and m0 == m1


def test_bit_identical_across_calls_positions_and_company(gfa, dense_random):
    refs = dense_random
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        base = list(range(0, 2000, 59))           # 34 sources: more than one pass at every width
        r1, s1, summ = g.parallel_pagerank(base, 20, stats=True)
        r2, s2, _ = g.parallel_pagerank(base, 20, stats=True)
        assert np.array_equal(r1, r2) and np.array_equal(s1, s2)
        W = summ["batch_width"]
        col = {x: (r1[l], s1[l]) for l, x in enumerate(base)}
        # permuted
        perm = [base[i] for i in np.random.default_rng(2).permutation(len(base))]
        rp, sp, _ = g.parallel_pagerank(perm, 20, stats=True)
        for l, x in enumerate(perm):
            assert np.array_equal(rp[l], col[x][0]) and sp[l] == col[x][1]
        # alone, with fewer, with more (others added in front and behind)
        x = base[0]
        for sources in ([x], base[:3], [1, 2, 3] + base + [1999]):
            r, s, _ = g.parallel_pagerank(sources, 20, stats=True)
            l = sources.index(x)
            assert np.array_equal(r[l], col[x][0]) and s[l] == col[x][1]
        # another pass: position 0 against position W + 1; and repeated within a call
        others = [v for v in range(1, 2 * W + 2) if v != x]
        sources = others[:W + 1] + [x] + others[W + 1:W + 3] + [x]
        assert sources.index(x) == W + 1
        r, s, _ = g.parallel_pagerank(sources, 20, stats=True)
        assert np.array_equal(r[W + 1], col[x][0]) and s[W + 1] == col[x][1]
        assert np.array_equal(r[-1], col[x][0]) and s[-1] == col[x][1]


# ---- 7. device path ----
def test_device_tensors(gfa):
    import torch

    scale = 12
    V = 1 << scale
    s, d = gfa.gen_rmat(scale, 16, seed=1)
    refs = Refs(V, s.cpu().numpy(), d.cpu().numpy())
    k, n = 5, 19
    sources = [int(x) for x in np.flatnonzero(refs.outdeg > 0)[:n]]
    with gfa.Graph(s, d, V) as g:
        out = torch.full((n, V), -1.0, dtype=torch.float64, device=s.device)
        assert g.parallel_pagerank(sources, k, out=out) is out
        first = out.cpu().numpy()
        out.fill_(-1.0)
        ranks, sums, summ = g.parallel_pagerank(sources, k, out=out, stats=True)
        assert ranks is out and isinstance(sums, np.ndarray)
        assert np.array_equal(out.cpu().numpy(), first)
        _compare((out, sums, summ), refs, sources, k)
        assert np.array_equal(g.parallel_pagerank(sources, k), first)   # host output of the same handle
        with pytest.raises(ValueError, match="float64"):
            g.parallel_pagerank(sources, k, out=torch.empty((n, V), dtype=torch.float32, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.parallel_pagerank(sources, k, out=torch.empty((n, V - 1), dtype=torch.float64, device=s.device))
        with pytest.raises(ValueError, match=f"{n}"):
            g.parallel_pagerank(sources, k, out=torch.empty((n + 1, V), dtype=torch.float64, device=s.device))
        with pytest.raises(ValueError, match=f"{V}"):
            g.parallel_pagerank(sources, k, out=torch.empty(n * V, dtype=torch.float64, device=s.device))
        with pytest.raises(ValueError, match="contiguous"):
            g.parallel_pagerank(sources, k, out=torch.empty((n, 2 * V), dtype=torch.float64, device=s.device)[:, ::2])
        with pytest.raises(ValueError, match="device tensor"):
            g.parallel_pagerank(sources, k, out=np.empty((n, V), np.float64))
        # the C ABI's own argument checks
        with pytest.raises(ValueError, match="max_iter"):
            g.parallel_pagerank(sources, 0)
        with pytest.raises(ValueError, match="reset_prob"):
            g.parallel_pagerank(sources, 3, 1.5)
        with pytest.raises(ValueError, match="reset_prob"):
            g.parallel_pagerank(sources, 3, float("nan"))
        with pytest.raises(ValueError, match="source"):
            g.parallel_pagerank([0, V], 3)
        with pytest.raises(ValueError, match="source"):
            g.parallel_pagerank([-1], 3)


def test_c_abi_einval(gfa):
    """The checks Graph.parallel_pagerank makes itself first, straight at the C ABI."""
    import ctypes

    from graphframes_amd import _lib

    V, s, d = random_multigraph(50, 200, 1)
    with gfa.Graph(s, d, V) as g:
        lib, h = g._lib, g._handle()
        out = np.empty((2, V), np.float64)
        good = np.array([1, 2], np.int32).ctypes.data_as(_lib._i32p)
        bad = np.array([1, V], np.int32).ctypes.data_as(_lib._i32p)
        neg = np.array([-1, 2], np.int32).ctypes.data_as(_lib._i32p)
        assert lib.lpa_parallel_pagerank(h, 3, 0.15, good, 2, out.ctypes.data, 0, None, None) == _lib.LPA_OK
        assert lib.lpa_parallel_pagerank(h, 3, 0.15, good, -1, out.ctypes.data, 0, None, None) == _lib.LPA_EINVAL
        assert "n_sources" in _lib.last_error()
        assert lib.lpa_parallel_pagerank(h, 3, 0.15, None, 2, out.ctypes.data, 0, None, None) == _lib.LPA_EINVAL
        assert "sources" in _lib.last_error()
        assert lib.lpa_parallel_pagerank(h, 3, 0.15, good, 2, None, 0, None, None) == _lib.LPA_EINVAL
        assert "rank output" in _lib.last_error()
        for ptr in (bad, neg):
            assert lib.lpa_parallel_pagerank(h, 3, 0.15, ptr, 2, out.ctypes.data, 0, None, None) == _lib.LPA_EINVAL
            assert "not a vertex" in _lib.last_error()
        # no sources: nothing is read or written, the summary carries the graph's integers
        summ = _lib.LpaPprSummary(9, 9, 9, 9, 9, 9, 9.0, 9.0)
        assert lib.lpa_parallel_pagerank(h, 3, 0.15, None, 0, None, 0, None, ctypes.byref(summ)) == _lib.LPA_OK
        assert summ.to_dict() == dict(ZEROS, edges=200, sinks=int((np.bincount(s, minlength=V) == 0).sum()),
                                      max_in_degree=int(np.bincount(d, minlength=V).max()))


# ---- 8. the LPA state is untouched ----
def test_does_not_disturb_lpa(gfa, mix):
    refs, sources = mix
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        want = g.run(3)
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        g.reset()
        g.step(1)
        before = g.info()["device_bytes"]
        r1 = g.parallel_pagerank(sources, 5)
        assert g.info()["device_bytes"] == before
        g.step(1)
        got2 = g.parallel_pagerank(sources, 5, stats=True)
        assert g.info()["device_bytes"] == before
        g.step(1)
        got = g.labels()
    assert np.array_equal(got, want)
    assert np.array_equal(r1, got2[0])
    _compare(got2, refs, sources, 5)


# ---- 9. drop-in ----
def test_graphframe_string_ids(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    V = ig.num_vertices
    refs = Refs(V, ig.src, ig.dst)
    dense = [int(np.argmax(refs.outdeg)), 5, int(np.argmax(refs.indeg)), 5]
    source_ids = [ids[x] for x in dense]
    gf = gfa.GraphFrame(v, e)
    try:
        res = gf.parallelPersonalizedPageRank(resetProbability=0.15, sourceIds=source_ids, maxIter=5)
        plain = gf.pageRank(maxIter=1)
    finally:
        gf.close()
    assert isinstance(res, gfa.GraphFrame)
    out = res.vertices
    assert list(out.columns) == ["id", "name", "pageranks"] and out["pageranks"].dtype == object
    assert np.array_equal(out["id"].to_numpy(), ig.ids)
    cells = out["pageranks"].to_numpy()
    assert all(isinstance(c, np.ndarray) and c.dtype == np.float64 and c.shape == (4,) for c in cells)
    got = np.stack(cells, axis=1)   # (4, V)
    b = pr_ref.bound(5, int(refs.indeg.max()), V)
    for l, x in enumerate(dense):
        rrank, _ = refs.get(5, 0.15, x)
        assert (np.abs(got[l] - rrank) <= b * rrank).all() and np.array_equal(got[l] == 0.0, rrank == 0.0)
    assert np.array_equal(got[1], got[3])
    ed = res.edges
    assert list(ed.columns) == ["src", "dst", "weight"] and ed["weight"].dtype == np.float64 and len(ed) == len(e)
    assert ed.equals(plain.edges)
    again = gfa.parallel_personalized_page_rank(v, e, np.array(source_ids), 5)
    assert list(again.columns) == list(out.columns) and again[["id", "name"]].equals(out[["id", "name"]])
    assert np.array_equal(np.stack(again["pageranks"].to_numpy(), axis=1), got)


def test_graphframe_integral_ids(gfa):
    """10 -> 20 -> 30 -> 10, 40 -> 10, and a dangling 40 -> 99."""
    v = pd.DataFrame({"id": np.array([30, 10, 20, 40], np.int64), "name": ["c", "a", "b", "d"]})
    e = pd.DataFrame({"src": np.array([10, 20, 40, 30, 40], np.int64), "dst": np.array([20, 30, 99, 10, 10], np.int64)})
    gf = gfa.GraphFrame(v, e)
    try:
        res = gf.parallelPersonalizedPageRank(sourceIds=(40, 10), maxIter=2)
        plain = gf.pageRank(maxIter=1)
        with pytest.raises(ValueError, match="99"):
            gf.parallelPersonalizedPageRank(sourceIds=[10, 99], maxIter=2)
    finally:
        gf.close()
    assert res.edges["src"].tolist() == [10, 20, 30, 40] and res.edges["dst"].tolist() == [20, 30, 10, 10]
    assert res.edges["weight"].tolist() == [1.0, 1.0, 1.0, 1.0] and res.edges.equals(plain.edges)
    got = res.vertices
    assert list(got.columns) == ["id", "name", "pageranks"]
    assert got["id"].tolist() == [10, 20, 30, 40] and got["name"].tolist() == ["a", "b", "c", "d"]
    p = np.stack(got["pageranks"].to_numpy(), axis=1)   # (2, 4): from 40, from 10
    b = pr_ref.bound(2, 2, 4)
    for l, x in enumerate((3, 0)):
        rrank, _, _, _ = pr_ref.pagerank(4, [0, 1, 2, 3], [1, 2, 0, 0], 2, source=x)
        assert (np.abs(p[l] - rrank) <= b * rrank).all() and np.array_equal(p[l] == 0.0, rrank == 0.0)
        assert abs(p[l].sum() - 1.0) <= 4 * 2.0 ** -52
    # two supersteps from 10 reach 20 and 30 but never 40; from 40 they reach 10 and 20, not 30
    assert (p[1] == 0.0).tolist() == [False, False, False, True]
    assert (p[0] == 0.0).tolist() == [False, False, True, False]


# ---- 10. partitioned job: rank 0 keeps the edge list ----
def test_two_loopback_ranks(gfa, mix):
    refs, sources = mix
    with gfa.Graph(refs.s, refs.d, refs.V) as g:
        single = g.parallel_pagerank(sources, 5, stats=True)
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(refs.s, refs.d, refs.V, rank=r, loopback=lb) for r in range(2)]
    try:
        rank, sums, summ = ranks[0].parallel_pagerank(sources, 5, stats=True)
        assert np.array_equal(rank, single[0]) and np.array_equal(sums, single[1]) and summ == single[2]
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].parallel_pagerank(sources, 5)
    finally:
        for g in ranks:
            g.close()
        lb.close()
