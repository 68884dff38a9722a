"""Betweenness centrality on the GPU (lpa_betweenness, csrc/lpa_bc.hip) against the two CPU
references of tests/bc_ref.py (plain-Python Brandes; networkx) and the fixtures' closed forms.

Tolerance, derived and not measured.  All terms are non-negative; a row of n terms summed in any
order, with a division and a product per term, is within about (n + 4) 2^-53 relative, and that
compounds over the D levels.  Every comparison first asserts from the reference's own numbers
that (max_depth + 1) (max_list + 4) 2^-53 < 1e-10, then compares with rtol = 1e-9, atol = 0 and
requires an exact 0 wherever the reference is 0.  The integers of the summary are compared
exactly.  Determinism is bit for bit: across calls, handles, input edge orders and batch widths.
Drop-in calls: GraphFrame.betweennessCentrality, betweenness_centrality."""
import math
import os

import numpy as np
import pandas as pd
import pytest

import bc_ref
from graphs import degree_mix, random_multigraph

pytestmark = pytest.mark.gpu

BATCHES = (0, 1, 16)   # the library's width and the two forced ends
WIDTHS = (1, 4, 8, 16)


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _i32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32))


def _bound_holds(ref):
    assert (ref["max_depth"] + 1) * (ref["max_list"] + 4) * 2.0 ** -53 < 1e-10, (ref["max_depth"], ref["max_list"])


def _compare(got, want, what=""):
    """rtol = 1e-9, atol = 0, and an exact 0 where the reference is 0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape
    nz = want != 0
    worst = float(np.max(np.abs(got[nz] - want[nz]) / want[nz])) if nz.any() else 0.0
    print(f"{what} worst relative difference {worst:.3g} over {int(nz.sum())} non-zero of {want.size}")
    assert np.array_equal(got == 0, want == 0), f"{what}: zeros differ at {np.flatnonzero((got == 0) != (want == 0))[:8]}"
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)


def _check(gfa, V, s, d, sources, directed, ref=None, batches=BATCHES, g=None):
    """betweenness(stats=True) at every width of `batches` (of a fresh handle unless g is given)
    against the reference dict: the values within the bound, the summary's integers exactly.
    Returns the raw array of the first width."""
    s, d = _i32(s), _i32(d)
    if ref is None:
        ref = bc_ref.brandes(V, s, d, sources, directed)
    _bound_holds(ref)
    n = V if sources is None else len(sources)
    own = g is None
    if own:
        g = gfa.Graph(s, d, V)
    first = None
    try:
        for batch in batches:
            raw, summ = g.betweenness(sources, directed=directed, batch=batch, stats=True)
            print(f"V={V} sources={n} directed={directed} batch={batch} summary={summ}")
            _compare(raw, ref["raw"], f"batch {batch}")
            width = batch or summ["batch_width"]   # batch 0: the library's default, whichever it is
            assert summ["batch_width"] == width and width in WIDTHS
            assert summ["batches"] == math.ceil(n / width)
            assert summ["sources"] == n
            for key in ("arcs", "reached", "max_depth"):
                assert summ[key] == ref[key], key
            assert summ["levels"] >= summ["batches"] and summ["levels"] <= summ["batches"] * (ref["max_depth"] + 1)
            if first is None:
                first = raw
            else:
                assert np.array_equal(raw, first), f"batch {batch} changes bits"
    finally:
        if own:
            g.close()
    return first


# ---- 1. base cases ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        for batch in BATCHES:
            raw, summ = g.betweenness(batch=batch, stats=True)
            assert raw.shape == (0,) and raw.dtype == np.float64
            assert summ == dict(arcs=0, sources=0, batches=0, batch_width=0, reached=0, max_depth=-1, levels=0)
        assert g.betweenness([]).shape == (0,)
        with pytest.raises(ValueError, match="source 0"):
            g.betweenness([0])


@pytest.mark.parametrize("V", [1, 2, 3])
def test_edgeless(gfa, V):
    e = np.empty(0, np.int32)
    for directed in (True, False):
        raw = _check(gfa, V, e, e, None, directed)
        assert np.array_equal(raw, np.zeros(V))


def test_single_arc(gfa):
    for directed in (True, False):
        raw = _check(gfa, 2, [0], [1], None, directed)
        assert np.array_equal(raw, np.zeros(2))
    raw = _check(gfa, 3, [0], [1], None, True)
    assert np.array_equal(raw, np.zeros(3))


def test_two_cycle_with_loops_and_duplicates(gfa):
    """0 <-> 1 -> 2: self-loops and duplicate rows change nothing."""
    s, d = [0, 1, 1], [1, 0, 2]
    plain = _check(gfa, 3, s, d, None, True)
    assert plain.tolist() == [0.0, 1.0, 0.0]
    noisy = _check(gfa, 3, s + [0, 1, 2, 2, 0, 1, 1], d + [0, 1, 2, 2, 1, 0, 2], None, True)
    assert np.array_equal(noisy, plain)
    und = _check(gfa, 3, s + [2, 2], d + [2, 1], None, False)
    assert und.tolist() == [0.0, 2.0, 0.0]   # both orientations of the pair (0, 2) pass through 1


def test_no_sources_writes_zeros(gfa):
    V, s, d = random_multigraph(50, 200, 3)
    with gfa.Graph(s, d, V) as g:
        raw, summ = g.betweenness([], stats=True)
        assert np.array_equal(raw, np.zeros(V))
        arcs = bc_ref.brandes(V, s, d, [])["arcs"]
        assert summ.pop("batch_width") in WIDTHS
        assert summ == dict(arcs=arcs, sources=0, batches=0, reached=0, max_depth=-1, levels=0)


def test_library_argument_errors(gfa):
    """The C call's own checks (Graph.betweenness checks first; this goes below it)."""
    import ctypes

    from graphframes_amd import _lib

    V, s, d = random_multigraph(20, 60, 1)
    out = np.zeros(V)
    with gfa.Graph(s, d, V) as g:
        def call(sources, n, batch=0, ptr=out.ctypes.data):
            sv = None if sources is None else _i32(sources).ctypes.data_as(_lib._i32p)
            return g._lib.lpa_betweenness(g._handle(), sv, n, 1, batch, ptr, 0, None)

        assert call([0, 1], -1) == _lib.LPA_EINVAL
        assert call([0, 20], 2) == _lib.LPA_EINVAL
        assert call([0, -1], 2) == _lib.LPA_EINVAL
        assert call([3, 4, 3], 3) == _lib.LPA_EINVAL
        for batch in (2, 3, 5, 32, -1):
            assert call([0], 1, batch) == _lib.LPA_EINVAL
        assert call([0], 1, 0, None) == _lib.LPA_EINVAL
        assert call(None, -7) == _lib.LPA_OK        # null sources: every vertex, n_sources ignored
        assert np.array_equal(out, g.betweenness())
        assert call([0, 1], 0) == _lib.LPA_OK and np.array_equal(out, np.zeros(V))


def test_device_output(gfa):
    import torch

    V, s, d = random_multigraph(300, 1500, 4)
    with gfa.Graph(s, d, V) as g:
        host = g.betweenness()
        out = torch.full((V,), -1.0, dtype=torch.float64, device="cuda:0")
        got, summ = g.betweenness(out=out, stats=True)
        assert got is out and np.array_equal(out.cpu().numpy(), host) and summ["sources"] == V
        with pytest.raises(ValueError, match="float64"):
            g.betweenness(out=torch.zeros(V, device="cuda:0"))
        with pytest.raises(ValueError, match="contiguous entries"):
            g.betweenness(out=torch.zeros(V + 1, dtype=torch.float64, device="cuda:0"))


# ---- 2. depth, width, path counts ----
def test_path_of_300_is_deeper_than_255(gfa):
    V, s, d = bc_ref.path(300)
    i = np.arange(300.0)
    ref = dict(raw=i * (299 - i), max_depth=299, reached=300 * 301 // 2, arcs=299, max_list=1)
    raw = _check(gfa, V, s, d, None, True, ref)
    assert np.array_equal(raw, ref["raw"])   # small integers: every sum is exact


def test_star_of_5000_leaves(gfa):
    """The centre is a block-form row; undirected, unnormalised: (n - 1)(n - 2) / 2 at the centre."""
    n = 5001
    s, d = np.zeros(n - 1, np.int32), np.arange(1, n, dtype=np.int32)
    want = np.zeros(n)
    want[0] = (n - 1) * (n - 2)          # raw: both orientations of every pair of leaves
    ref = dict(raw=want, max_depth=2, reached=n * n, arcs=2 * (n - 1), max_list=n - 1)
    raw = _check(gfa, n, s, d, None, False, ref, batches=(0,))
    assert raw[0] / 2 == (n - 1) * (n - 2) / 2
    # a subset (the centre and 40 leaves) at every width: a leaf sees the n - 2 others through the centre
    S = [0] + list(range(7, 5000, 128))
    want = np.zeros(n)
    want[0] = (len(S) - 1) * (n - 2)
    ref = dict(raw=want, max_depth=2, reached=len(S) * n, arcs=2 * (n - 1), max_list=n - 1)
    _check(gfa, n, s, d, S, False, ref)
    # directed: nothing passes through the centre, a leaf reaches nothing
    ref = dict(raw=np.zeros(n), max_depth=1, reached=n + len(S) - 1, arcs=n - 1, max_list=n - 1)
    _check(gfa, n, s, d, S, True, ref)


@pytest.fixture(scope="module")
def stars():
    V, s, d, centres = bc_ref.form_stars()
    refs = {directed: bc_ref.brandes(V, s, d, None, directed) for directed in (True, False)}
    for r in refs.values():
        r["raw"].setflags(write=False)
    return V, s, d, centres, refs


@pytest.mark.parametrize("directed", [True, False], ids=["directed", "undirected"])
def test_lists_at_the_form_thresholds(gfa, stars, directed):
    """Out-lists and in-lists of 0, 1, 8, 9, 32, 33 (kBcShort +- ...), 1024 and 1025 (kBcWave) entries."""
    V, s, d, centres, refs = stars
    assert refs[directed]["raw"].max() > 0
    _check(gfa, V, s, d, None, directed, refs[directed])


def test_degree_mix_hubs(gfa):
    """degree_mix: hub rows of hundreds to thousands of distinct arcs beside the short bands; the
    four hubs, the first low vertices and a spread of the rest as sources."""
    V, s, d = degree_mix()
    S = list(range(12)) + list(range(100, V, 251))
    with gfa.Graph(_i32(s), _i32(d), V) as g:
        for directed in (True, False):
            ref = bc_ref.brandes(V, s, d, S, directed)
            assert ref["max_list"] > 1024
            _check(gfa, V, s, d, S, directed, ref, g=g)


def test_diamond_chain_sigma_above_2_53(gfa):
    V, s, d = bc_ref.diamond_chain(40)
    assert V == 161 and 3 ** 40 > 2 ** 53
    ref = bc_ref.brandes(V, s, d)
    assert ref["max_depth"] == 80
    _check(gfa, V, s, d, None, True, ref)
    _compare(ref["raw"], bc_ref.networkx_bc(V, s, d, True, False), "brandes against networkx")


def test_components_and_isolated(gfa):
    """A 3-path, a 4-cycle with a tail and isolated vertices; sources that reach nothing give zeros."""
    s = [0, 1, 10, 11, 12, 13, 13]
    d = [1, 2, 11, 12, 13, 10, 14]
    V = 20
    _check(gfa, V, s, d, None, True)
    _check(gfa, V, s, d, None, False)
    raw = _check(gfa, V, s, d, [2, 5, 14, 19], True)
    assert np.array_equal(raw, np.zeros(V))
    raw = _check(gfa, V, s, d, [5, 6, 19], False)
    assert np.array_equal(raw, np.zeros(V))


@pytest.fixture(scope="module")
def small():
    V, s, d = random_multigraph(200, 900, 11)
    return V, s, d


@pytest.mark.parametrize("n", [15, 16, 17])
def test_pass_edges(gfa, small, n):
    V, s, d = small
    S = bc_ref.pivots(V, n, 5)[::-1].tolist()   # descending: the order of the sources is the caller's
    with gfa.Graph(s, d, V) as g:
        for directed in (True, False):
            _check(gfa, V, s, d, S, directed, g=g, batches=(0, 1, 4, 8, 16))


def test_unequal_depths_in_one_pass(gfa):
    """One pass holds the end of a 300-path (depth 299) and the centre of a star (depth 1)."""
    V, s, d = bc_ref.path(300)
    leaves = np.arange(301, 331, dtype=np.int32)
    s = np.concatenate([s, np.full(leaves.size, 300, np.int32)])
    d = np.concatenate([d, leaves])
    S = [0, 300, 150, 305, 299]
    raw = _check(gfa, 331, s, d, S, True)
    i = np.arange(300.0)
    want = np.zeros(331)
    want[1:299] = 298 - i[:298]           # source 0: vertex v lies before 299 - v others
    want[151:299] += 298 - i[150:298]     # source 150
    assert np.array_equal(raw, want)
    _check(gfa, 331, s, d, S, False)


# ---- 3. the random multigraph: both references, determinism ----
@pytest.fixture(scope="module")
def big():
    V, s, d = random_multigraph(2000, 12000, 7)
    S = bc_ref.pivots(V, 64, 2).tolist()
    refs = {}
    for directed in (True, False):
        full = bc_ref.brandes(V, s, d, None, directed)
        sub = bc_ref.brandes(V, s, d, S, directed)
        nxv = bc_ref.networkx_bc(V, s, d, directed, normalized=False)
        for a in (full["raw"], sub["raw"], nxv):
            a.setflags(write=False)
        refs[directed] = (full, sub, nxv)
    return V, s, d, S, refs


@pytest.mark.parametrize("directed", [True, False], ids=["directed", "undirected"])
def test_random_multigraph_all_sources(gfa, big, directed):
    V, s, d, S, refs = big
    full, sub, nxv = refs[directed]
    raw = _check(gfa, V, s, d, None, directed, full)
    _compare(bc_ref.scale(raw, V, V, directed, normalized=False), nxv, "against networkx")


@pytest.mark.parametrize("directed", [True, False], ids=["directed", "undirected"])
def test_random_multigraph_subset(gfa, big, directed):
    V, s, d, S, refs = big
    _check(gfa, V, s, d, S, directed, refs[directed][1])


@pytest.mark.parametrize("directed", [True, False], ids=["directed", "undirected"])
def test_bit_identical(gfa, big, directed):
    V, s, d, S, refs = big
    S3 = S[:37]
    with gfa.Graph(s, d, V) as g:
        a = g.betweenness(directed=directed)
        assert np.array_equal(g.betweenness(directed=directed), a)                       # two calls
        by_width = [g.betweenness(S3, directed=directed, batch=b) for b in WIDTHS]
        sub = g.betweenness(S, directed=directed)
    for x in by_width[1:]:
        assert np.array_equal(x, by_width[0])                                             # batch widths
    perm = np.random.default_rng(8).permutation(s.size)
    with gfa.Graph(s[perm], d[perm], V) as g2:                                            # another handle,
        assert np.array_equal(g2.betweenness(directed=directed), a)                       # another edge order
        assert np.array_equal(g2.betweenness(S, directed=directed), sub)
    assert not np.array_equal(sub, a)


def test_create_time_batch_override(gfa, big):
    V, s, d, S, refs = big
    with gfa.Graph(s, d, V) as g:
        want, summ = g.betweenness(S, stats=True)
        default = summ["batch_width"]
        assert default in WIDTHS
    old = os.environ.get("LPA_BC_BATCH")
    try:
        for value, width in (("4", 4), ("1", 1), ("8", 8), ("5", default)):
            os.environ["LPA_BC_BATCH"] = value
            with gfa.Graph(s, d, V) as g:
                raw, summ = g.betweenness(S, stats=True)
                assert summ["batch_width"] == width and summ["batches"] == math.ceil(len(S) / width)
                assert np.array_equal(raw, want)
                assert g.betweenness(S, batch=8, stats=True)[1]["batch_width"] == 8     # the argument wins
    finally:
        if old is None:
            os.environ.pop("LPA_BC_BATCH", None)
        else:
            os.environ["LPA_BC_BATCH"] = old


# ---- 4. the drop-in calls ----
@pytest.fixture(scope="module")
def frame():
    """String ids in an order that is not the sorted one, an extra vertex column, an edge whose
    end is no vertex, duplicates and self-loops."""
    V, s, d = random_multigraph(60, 170, 21)
    names = np.array([f"n{(7 * i) % 60:02d}" for i in range(60)])     # a permutation of n00 .. n59
    v = pd.DataFrame({"id": names, "weight": np.arange(60) * 1.5})
    e = pd.DataFrame({"src": np.concatenate([names[s], ["n03", "ghost"]]),
                      "dst": np.concatenate([names[d], ["n03", "n01"]])})
    return v, e


def _networkx_of_frame(v, e, directed, normalized):
    import networkx as nx

    G = nx.DiGraph() if directed else nx.Graph()
    G.add_nodes_from(v["id"])
    ids = set(v["id"])
    G.add_edges_from((a, b) for a, b in zip(e["src"], e["dst"]) if a != b and a in ids and b in ids)
    bc = nx.betweenness_centrality(G, normalized=normalized)
    return np.asarray([bc[x] for x in sorted(ids)])


@pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "unnormalized"])
@pytest.mark.parametrize("directed", [True, False], ids=["directed", "undirected"])
def test_graphframe_against_networkx(gfa, frame, directed, normalized):
    v, e = frame
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.betweennessCentrality(normalized=normalized, directed=directed)
    finally:
        gf.close()
    assert list(out.columns) == ["id", "weight", "betweenness"]
    assert out["id"].tolist() == sorted(v["id"]) and out["betweenness"].dtype == np.float64
    assert np.array_equal(out["weight"].to_numpy(), v.set_index("id").loc[out["id"], "weight"].to_numpy())
    want = _networkx_of_frame(v, e, directed, normalized)
    assert want.max() > 0
    _bound_holds(bc_ref.brandes(60, *_dense(v, e), None, directed))
    _compare(out["betweenness"].to_numpy(), want, "GraphFrame against networkx")
    assert out.attrs["sources"] == 60 and out.attrs["exact"] is True
    assert 1 <= out.attrs["max_depth"] < 60


def test_graphframe_pivots_and_function_form(gfa, frame):
    v, e = frame
    ids = np.sort(v["id"].to_numpy())
    draw = np.sort(np.random.default_rng(3).choice(60, size=10, replace=False))
    gf = gfa.GraphFrame(v, e)
    try:
        by_k = gf.betweennessCentrality(k=10, seed=3)
        by_sources = gf.betweennessCentrality(sources=list(ids[draw]))
        raw, summ = gf._gpu_graph().betweenness(draw.astype(np.int32), stats=True)
        exact = gf.betweennessCentrality()
    finally:
        gf.close()
    assert np.array_equal(by_k["betweenness"].to_numpy(), by_sources["betweenness"].to_numpy())
    assert np.array_equal(by_k["betweenness"].to_numpy(), raw * (60 / 10) / (59 * 58))
    assert by_k.attrs == dict(sources=10, max_depth=summ["max_depth"], exact=False)
    assert by_sources.attrs == by_k.attrs
    fn = gfa.betweenness_centrality(v, e)
    assert fn.equals(exact) and fn.attrs == exact.attrs
    fn = gfa.betweenness_centrality(v, e, k=10, seed=3, normalized=False, directed=False)
    ref = bc_ref.scale(bc_ref.brandes(60, *_dense(v, e), draw, False)["raw"], 60, 10, False, False)
    _compare(fn["betweenness"].to_numpy(), ref, "function form, undirected pivots")


def _dense(v, e):
    ids = np.sort(v["id"].to_numpy())
    ok = e["src"].isin(ids) & e["dst"].isin(ids)
    return np.searchsorted(ids, e["src"][ok].to_numpy()), np.searchsorted(ids, e["dst"][ok].to_numpy())


def test_graphframe_small_frames(gfa):
    v = pd.DataFrame({"id": [5, 9]})
    e = pd.DataFrame({"src": [5], "dst": [9]})
    for normalized in (True, False):
        out = gfa.betweenness_centrality(v, e, normalized=normalized)
        assert out["betweenness"].tolist() == [0.0, 0.0]          # V <= 2
    v = pd.DataFrame({"id": [1, 2, 3]})
    e = pd.DataFrame({"src": [1, 2], "dst": [2, 3]})
    assert gfa.betweenness_centrality(v, e)["betweenness"].tolist() == [0.0, 0.5, 0.0]
    assert gfa.betweenness_centrality(v, e, normalized=False, directed=False)["betweenness"].tolist() == [0.0, 1.0, 0.0]
