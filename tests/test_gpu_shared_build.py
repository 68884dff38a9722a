"""The shared edge-list builds (csrc/lpa_adj.hip) under every call that rests on them, at the
vertex counts where bits_for(V) and bits_for(V - 1) part ways (V = 2^8, 2^16 and 2^24 and their
neighbours: one radix pass a half more for the directed-arc keys, which hold values up to V,
than for the simple-edge keys, which hold ids).  One generated multigraph per case and one handle:
every call against the numpy reference its own test file uses, the edge counts of the summaries
against numpy counts of the same list, and a second call on the handle against the first.

The multigraph of SIZES has 4024 edges: less than one tile of the sort and the scans (4096
elements to a block, csrc/lpa_prims.hip), so one block, one scan level and one histogram column.
EDGE_CASES run the same calls with the edge list at a tile's edge (4096 and 4097 edges) and over
several tiles (12289 = 3 * 4096 + 1); tests/test_gpu_prims.py checks the primitives themselves
there."""
import numpy as np
import pytest

import cc_ref
import kcore_ref
import pr_ref
import scc_ref
import sp_ref
import tc_ref

pytestmark = pytest.mark.gpu

SIZES = [255, 256, 257, 65535, 65536, 65537, 2**24 - 1, 2**24, 2**24 + 1]
BASE_EDGES = 4024
EDGE_CASES = [(65536, 4096), (65536, 4097), (257, 12289)]   # (V, edges)
CASES = [(v, BASE_EDGES) for v in SIZES] + EDGE_CASES
PR_ITERS = 10


def generate(V, seed=9, m=BASE_EDGES):
    """(s, d, isolated): m edges, every appended extra counted (m >= 2024; 4024 is under one tile
    of the build's sort), among at most 300 vertices spread over [0, V), with edges at vertex 0
    and at V - 1, both directions of some pairs, duplicates, self-loops (one on V - 1) and a
    vertex without any edge."""
    rng = np.random.default_rng(seed + V)
    isolated = V // 2
    others = np.setdiff1d(np.arange(1, V - 1), [isolated])
    pool = np.concatenate([[0, V - 1], rng.choice(others, size=min(V // 2, 300) - 2, replace=False)])
    n = m - 1024   # the extras below: 500 reversed, 500 duplicates, 21 loops, 3 more
    assert n >= 1000
    a = rng.choice(pool, size=n)
    b = rng.choice(pool, size=n)
    loops = np.concatenate([[V - 1], rng.choice(pool, size=20)])
    s = np.concatenate([a, b[:500], a[500:1000], loops, [0, V - 1, 0]])
    d = np.concatenate([b, a[:500], b[500:1000], loops, [V - 1, 0, pool[5]]])
    assert s.size == m and d.size == m
    order = rng.permutation(s.size)
    return s[order].astype(np.int32), d[order].astype(np.int32), isolated


@pytest.fixture(scope="module", params=CASES,
                ids=[f"V{v}" if m == BASE_EDGES else f"V{v}-m{m}" for v, m in CASES])
def case(request):
    import graphframes_amd

    V, m = request.param
    s, d, isolated = generate(V, m=m)
    assert s.size == m
    touched = np.zeros(V, bool)
    touched[s] = True
    touched[d] = True
    assert touched[0] and touched[V - 1] and not touched[isolated]
    assert ((s == V - 1) & (d == V - 1)).any()
    with graphframes_amd.Graph(s, d, V) as g:
        yield V, s, d, g


def _same(a, b):
    """Two results of one call: the arrays are equal."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if not isinstance(x, dict):
            assert np.array_equal(x, y)


def test_shortest_paths(case):
    V, s, d, g = case
    lms = [V - 1]
    ref = sp_ref.shortest_paths(V, s, d, lms)
    dist, summ = g.shortest_paths(lms, stats=True)
    assert dist.dtype == np.int32 and np.array_equal(dist, ref)
    want = sp_ref.summary(V, s, d, ref)
    levels = want.pop("levels")
    assert {k: summ[k] for k in want} == want
    assert summ["push_levels"] + summ["pull_levels"] == levels
    assert summ["arcs"] == sp_ref.arcs(V, s, d)[0].size
    _, only = g.shortest_paths([], stats=True)   # the count-only path of the build
    assert only["arcs"] == summ["arcs"]
    _same(g.shortest_paths(lms, stats=True), (dist, summ))


def test_strongly_connected_components(case):
    V, s, d, g = case
    want, wsumm = scc_ref.scc_rounds(V, s, d)
    comp, size, summ = g.strongly_connected_components(sizes=True)
    assert comp.dtype == np.int32 and np.array_equal(comp, want)
    assert np.array_equal(size, np.bincount(want, minlength=V))
    assert summ == wsumm
    _same(g.strongly_connected_components(sizes=True), (comp, size, summ))


def test_triangle_count(case):
    V, s, d, g = case
    rcount, rdeg = tc_ref.triangles(V, s, d)
    count, deg, summ = g.triangle_count(stats=True)
    assert count.dtype == np.int64 and np.array_equal(count, rcount)
    assert np.array_equal(deg, rdeg)
    assert summ == tc_ref.summary(rcount, rdeg)
    assert summ["simple_edges"] == tc_ref.simple_edges(V, s, d)[0].size
    _same(g.triangle_count(stats=True), (count, deg, summ))


def test_core_numbers(case):
    V, s, d, g = case
    rcore, rdeg = kcore_ref.core_numbers(V, s, d)
    core, deg, summ = g.core_numbers(stats=True)
    assert core.dtype == np.int32 and np.array_equal(core, rcore)
    assert np.array_equal(deg, rdeg)
    assert {k: summ[k] for k in kcore_ref.PURE_KEYS} == kcore_ref.summary_of(rcore, rdeg)
    assert summ["simple_edges"] == tc_ref.simple_edges(V, s, d)[0].size
    _same(g.core_numbers(stats=True), (core, deg, summ))


def test_pagerank(case):
    V, s, d, g = case
    rrank, rodeg, rideg, rS = pr_ref.pagerank(V, s, d, PR_ITERS)
    rank, odeg, ideg, summ = g.pagerank(PR_ITERS, stats=True)
    assert np.array_equal(odeg, rodeg) and np.array_equal(ideg, rideg)
    b = pr_ref.bound(PR_ITERS, int(rideg.max()), V)
    assert (np.abs(rank - rrank) <= b * rrank).all()
    rsumm = pr_ref.summary(rrank, rodeg, rideg, rS)
    for key in ("edges", "sinks", "max_in_degree"):
        assert summ[key] == rsumm[key], key
    assert abs(summ["rank_sum"] - rS) <= b * rS
    _same(g.pagerank(PR_ITERS, stats=True), (rank, odeg, ideg, summ))   # bit-identical across calls


def test_components(case):
    V, s, d, g = case
    ref = cc_ref.components(V, s, d)
    rsizes, rsumm = cc_ref.summary(ref)
    comp, sizes, summ = g.components(sizes=True)
    assert comp.dtype == np.int32 and np.array_equal(comp, ref)
    assert np.array_equal(sizes, rsizes)
    assert summ == rsumm
    _same(g.components(sizes=True), (comp, sizes, summ))
