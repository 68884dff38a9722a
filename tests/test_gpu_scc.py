"""Strongly connected components on the GPU (lpa_strongly_connected_components,
csrc/lpa_scc.hip) against the numpy restatement of GraphX's rounds, tests/scc_ref.py: exact
equality of comp, of the sizes and of every summary field at the same max_iter, converged or
stopped early; identical results across edge orders, calls, handles and in-block trim sizes.
Drop-in calls: GraphFrame.stronglyConnectedComponents, strongly_connected_components.

One figure of the issue is not asserted as written: it expects rounds == 3 for a graph of
self-loops only.  By the contract's own rounds (and GraphX's loop) such vertices are coloured
and marked in round 1 and written in round 2, after which nothing is alive: rounds == 2, the
count the issue's own chain cases imply (twenty SCCs one after another: 21; all at once: 2).
The reference and the library both give 2, and test_only_self_loops asserts 2."""
import numpy as np
import pandas as pd
import pytest

import scc_ref
from graphs import degree_mix, random_multigraph, star, two_cliques

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _compare(got, V, s, d, max_iter=None, ref=None):
    """One sizes=True result against the reference at the same max_iter; returns the reference."""
    comp, size, summ = got
    if ref is None:
        ref = scc_ref.scc_rounds(V, s, d, scc_ref.CONVERGE if max_iter is None else max_iter)
    want, wsumm = ref
    print(f"V={V} max_iter={max_iter} summary={summ}")
    assert comp.dtype == np.int32 and comp.shape == (V,)
    assert np.array_equal(comp, want), f"{int((comp != want).sum())} of {V} components differ"
    assert size.dtype == np.int64 and np.array_equal(size, np.bincount(want, minlength=V))
    assert summ == wsumm
    return ref


def _check(gfa, V, s, d, max_iter=None, g=None, ref=None):
    """strongly_connected_components() plain and with sizes (of a fresh handle unless g is given)."""
    s = np.asarray(s, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    own = g is None
    if own:
        g = gfa.Graph(s, d, V)
    try:
        comp = g.strongly_connected_components(max_iter)
        got = g.strongly_connected_components(max_iter, sizes=True)
    finally:
        if own:
            g.close()
    assert np.array_equal(comp, got[0])
    _compare(got, V, s, d, max_iter, ref)
    return got


# ---- 1. degenerate ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        assert g.strongly_connected_components().shape == (0,)
        comp, size, summ = g.strongly_connected_components(3, sizes=True)
    assert comp.shape == (0,) and size.shape == (0,)
    assert summ == dict(n_components=0, n_singletons=0, largest_size=0, largest_id=-1, rounds=0, trimmed=0,
                        unresolved=0)


def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    comp, _, summ = _check(gfa, 1, e, e)
    assert comp.tolist() == [0] and summ["rounds"] == 1 and summ["trimmed"] == 1


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    comp, _, summ = _check(gfa, 70, e, e)
    assert np.array_equal(comp, np.arange(70)) and summ["n_singletons"] == 70 and summ["trimmed"] == 70


def test_only_self_loops(gfa):
    """Coloured and marked in round 1, written in round 2 (see the module's docstring)."""
    v = np.arange(70, dtype=np.int32)
    comp, _, summ = _check(gfa, 70, v, v)
    assert np.array_equal(comp, v) and summ["rounds"] == 2 and summ["trimmed"] == 0
    few = np.array([3, 3, 0, 99, 64, 64, 64], np.int32)
    _, _, summ = _check(gfa, 100, few, few)
    assert summ["rounds"] == 2 and summ["trimmed"] == 96
    _, _, one = _check(gfa, 100, few, few, max_iter=1)
    assert one["rounds"] == 1 and one["unresolved"] == 4


def test_one_edge_repeated(gfa):
    s, d = np.full(1000, 6, np.int32), np.full(1000, 2, np.int32)
    comp, _, summ = _check(gfa, 9, s, d)
    assert np.array_equal(comp, np.arange(9)) and summ["rounds"] == 1 and summ["trimmed"] == 9


def test_two_cycle(gfa):
    comp, _, summ = _check(gfa, 5, [3, 1], [1, 3])
    assert comp.tolist() == [0, 1, 2, 1, 4] and summ["rounds"] == 2 and summ["largest_id"] == 1
    assert _check(gfa, 5, [3, 1], [1, 3], max_iter=1)[0].tolist() == [0, 1, 2, 3, 4]


# ---- 2. depth ----
@pytest.mark.parametrize("block", [None, "0", "64"], ids=["default", "launch-per-level", "block-64"])
def test_directed_path(gfa, monkeypatch, block):
    """1000 trim levels of two vertices each: the in-block trim; the same by a launch per level."""
    if block is not None:
        monkeypatch.setenv("LPA_SCC_BLOCK", block)
    V, s, d = scc_ref.path(2000)
    comp, _, summ = _check(gfa, V, s, d)
    assert np.array_equal(comp, np.arange(V)) and summ["rounds"] == 1 and summ["trimmed"] == V


def test_trim_levels_grow_and_shrink(gfa, monkeypatch):
    """A path into the centre of a star of 100 000.  Leaves without a way out: the first level
    holds them all (a launch per form), the centre's out-count takes 10^5 decrements, the path's
    levels of one or two vertices run in the block.  Leaves that all feed one sink: the in-block
    trim starts on two vertices (the path's head, the sink) and its first level removes 100 001,
    more than its LDS queue holds, so it hands back to the launches."""
    monkeypatch.setenv("LPA_SCC_BLOCK", "4096")
    n, k = 200, 100_000
    i = np.arange(n - 1)
    leaves = n + np.arange(k)
    s = np.concatenate([i, np.full(k, n - 1)])
    d = np.concatenate([i + 1, leaves])
    _, _, summ = _check(gfa, n + k, s, d)
    assert summ["trimmed"] == n + k and summ["rounds"] == 1
    sink = n + k
    _, _, summ = _check(gfa, sink + 1, np.concatenate([s[::-1], leaves]), np.concatenate([d[::-1], np.full(k, sink)]))
    assert summ["trimmed"] == sink + 1 and summ["rounds"] == 1


def test_directed_cycle_rotated(gfa):
    V, s, d = scc_ref.cycle(1000, rotate=333)
    comp, _, summ = _check(gfa, V, s, d)
    assert (comp == 0).all() and summ["n_components"] == 1 and summ["largest_id"] == 0 and summ["rounds"] == 2


@pytest.mark.parametrize("ascending", [True, False], ids=["ascending", "descending"])
def test_max_iter_sweep_on_chains(gfa, ascending):
    V, s, d = scc_ref.chain_of_2cycles(20, ascending)
    with gfa.Graph(s, d, V) as g:
        for r in range(1, 23):
            _, _, summ = _check(gfa, V, s, d, max_iter=r, g=g)
            assert summ["rounds"] == min(r, 21 if ascending else 2)
        _, _, summ = _check(gfa, V, s, d, g=g)
    assert summ["unresolved"] == 0 and summ["n_components"] == 20


# ---- 3. tails ----
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000])
def test_tails(gfa, V):
    _, s, d = random_multigraph(V, 3 * V, 11 + V)
    _check(gfa, V, s, d)
    _check(gfa, V, s, d, max_iter=2)


# ---- 4. long lists ----
def test_star_out_of_hub(gfa):
    """hub -> 100 000 leaves: all of them the trim's first level, the hub's out-list a block row."""
    V, s, d = star(100_000)
    _, _, summ = _check(gfa, V, s, d)
    assert summ["trimmed"] == V and summ["rounds"] == 1


def test_star_into_hub(gfa):
    V, d, s = star(100_000)
    _, _, summ = _check(gfa, V, s, d)
    assert summ["trimmed"] == V and summ["rounds"] == 1


def test_wheel(gfa):
    """hub <-> 100 000 leaves: one SCC; the hub's lists take the block row in colour and in mark."""
    V, s, d = scc_ref.wheel(100_000)
    comp, _, summ = _check(gfa, V, s, d)
    assert (comp == 0).all() and summ["largest_size"] == V and summ["rounds"] == 2 and summ["trimmed"] == 0
    # the hub's id the largest: the leaves colour the hub, the hub colours the leaves
    _check(gfa, V, (V - 1 - s).astype(np.int32), (V - 1 - d).astype(np.int32))


# ---- 5. mixed ----
@pytest.fixture(scope="module")
def mix():
    V, s, d = degree_mix()
    # degree_mix's hubs only point outwards: 3000 edges also run the other way
    back = np.random.default_rng(4).integers(0, s.size, size=3000)
    s, d = np.concatenate([s, d[back]]), np.concatenate([d, s[back]])
    ref = scc_ref.scc_rounds(V, s, d)
    ref[0].setflags(write=False)
    return V, s, d, ref


def test_degree_mix(gfa, mix):
    V, s, d, ref = mix
    assert ref[1]["largest_size"] > 100 and ref[1]["trimmed"] > 0
    _check(gfa, V, s, d, ref=ref)
    _check(gfa, *degree_mix())
    for r in (1, 2, 3):
        _check(gfa, V, s, d, max_iter=r)


def test_two_cliques_directed_bridge(gfa):
    V, s, d = two_cliques(5)
    comp, _, summ = _check(gfa, V, s, d)
    assert comp.tolist() == [0] * 5 + [5] * 6 and summ["n_components"] == 2


def test_r9(gfa, golden):
    V = int(golden["ids"].size)
    s, d = golden["src"], golden["dst"]
    with gfa.Graph(s, d, V) as g:
        for r in (1, 2, 3, None):
            _check(gfa, V, s, d, max_iter=r, g=g)
    assert np.array_equal(scc_ref.scc_rounds(V, s, d)[0], scc_ref.scc_tarjan(V, s, d))


# ---- 6. invariance ----
def test_edge_order_and_duplicates(gfa, mix):
    V, s, d, ref = mix
    rng = np.random.default_rng(9)
    perm = rng.permutation(s.size)
    dup = rng.integers(0, s.size, size=5000)
    variants = [(s[::-1].copy(), d[::-1].copy()), (s[perm], d[perm]),
                (np.concatenate([s, s[dup]]), np.concatenate([d, d[dup]]))]
    for vs, vd in variants:
        with gfa.Graph(vs, vd, V) as g:
            _compare(g.strongly_connected_components(sizes=True), V, s, d, ref=ref)


def test_added_self_loops(gfa, mix):
    """Loops keep their vertices from the trim: compared with the reference OF THAT INPUT."""
    V, s, d, ref = mix
    loops = np.random.default_rng(5).integers(0, V, size=500).astype(np.int32)
    s2, d2 = np.concatenate([loops, s]), np.concatenate([loops, d])
    comp, _, summ = _check(gfa, V, s2, d2)
    assert np.array_equal(comp, ref[0])             # the converged result is the same ...
    assert summ["trimmed"] < ref[1]["trimmed"]      # ... the way there is not
    _check(gfa, V, s2, d2, max_iter=2)


def test_calls_handles_and_trim_sizes(gfa, monkeypatch, mix):
    V, s, d, ref = mix
    with gfa.Graph(s, d, V) as g:
        a = g.strongly_connected_components(sizes=True)
        b = g.strongly_connected_components(sizes=True)
    got = [a, b]
    for block in ("0", "8", "4096"):
        monkeypatch.setenv("LPA_SCC_BLOCK", block)   # read when the handle is created
        with gfa.Graph(s, d, V) as g:
            got.append(g.strongly_connected_components(sizes=True))
    for res in got:
        _compare(res, V, s, d, ref=ref)
        assert res[2] == a[2]


# ---- 7. isolation ----
def test_does_not_disturb_lpa(gfa, mix):
    V, s, d, ref = mix
    with gfa.Graph(s, d, V) as g:
        want = g.run(5)
        before = g.info()["device_bytes"]
        comp = g.strongly_connected_components()
        assert g.info()["device_bytes"] == before
        assert np.array_equal(g.labels(), want)
        assert np.array_equal(g.run(5), want)
        assert g.info()["device_bytes"] == before
    assert np.array_equal(comp, ref[0])
    with gfa.Graph(s, d, V) as g:   # between supersteps
        g.reset()
        g.step(2)
        g.strongly_connected_components(3)
        g.step(3)
        assert np.array_equal(g.labels(), want)


def test_device_tensor(gfa, mix):
    import torch

    V, s, d, ref = mix
    with gfa.Graph(s, d, V) as g:
        out = torch.full((V,), 7, dtype=torch.int32, device="cuda:0")
        assert g.strongly_connected_components(out=out) is out
        assert np.array_equal(out.cpu().numpy(), ref[0])
        out.fill_(7)
        comp, size, summ = g.strongly_connected_components(out=out, sizes=True)
        assert comp is out and size.is_cuda and size.dtype == torch.int64
        _compare((out.cpu().numpy(), size.cpu().numpy(), summ), V, s, d, ref=ref)
        assert np.array_equal(g.strongly_connected_components(), ref[0])   # host output of the same handle
        with pytest.raises(ValueError, match="int32"):
            g.strongly_connected_components(out=torch.empty(V, dtype=torch.int64, device="cuda:0"))
        with pytest.raises(ValueError, match=f"{V}"):
            g.strongly_connected_components(out=torch.empty(V - 1, dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError, match="contiguous"):
            g.strongly_connected_components(out=torch.empty(2 * V, dtype=torch.int32, device="cuda:0")[::2])
        with pytest.raises(ValueError, match="device tensor"):
            g.strongly_connected_components(out=np.empty(V, np.int32))
        with pytest.raises(ValueError, match="greater than 0"):
            g.strongly_connected_components(0)
        with pytest.raises(TypeError, match="max_iter"):
            g.strongly_connected_components(2.5)
        # the C ABI's own argument checks
        buf = np.empty(V, np.int32)
        lib, einval = g._lib, gfa._lib.LPA_EINVAL
        assert lib.lpa_strongly_connected_components(g._handle(), 0, buf.ctypes.data, 0, None, None) == einval
        assert "max_iter" in gfa._lib.last_error()
        assert lib.lpa_strongly_connected_components(g._handle(), -3, buf.ctypes.data, 0, None, None) == einval
        assert lib.lpa_strongly_connected_components(g._handle(), 5, None, 0, None, None) == einval
        assert lib.lpa_strongly_connected_components(g._handle(), 5, buf.ctypes.data, 0, None, None) == 0
        assert np.array_equal(buf, ref[0])


def test_two_loopback_ranks(gfa, mix):
    V, s, d, ref = mix
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        _compare(ranks[0].strongly_connected_components(sizes=True), V, s, d, ref=ref)
        # LPA_EINVAL, which the binding raises as ValueError (as for the other edge-list calls)
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].strongly_connected_components()
    finally:
        for g in ranks:
            g.close()
        lb.close()


# ---- 8. drop-in ----
def test_graphframe_integral_ids(gfa):
    """10 -> 20 -> 30 -> 10, 40 -> 10, 50 alone, 60 <-> 70 behind 30, and a dangling 40 -> 99."""
    v = pd.DataFrame({"id": np.array([30, 10, 50, 20, 40, 70, 60], np.int64),
                      "name": ["c", "a", "e", "b", "d", "g", "f"]})
    e = pd.DataFrame({"src": np.array([10, 20, 40, 30, 40, 30, 70, 60], np.int64),
                      "dst": np.array([20, 30, 99, 10, 10, 70, 60, 70], np.int64)})
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.stronglyConnectedComponents(maxIter=10)
        first = gf.stronglyConnectedComponents(1)
        second = gf.stronglyConnectedComponents(2)
        with pytest.raises(ValueError, match="Number of iterations must be greater than 0, but got 0"):
            gf.stronglyConnectedComponents(0)
    finally:
        gf.close()
    assert list(out.columns) == ["id", "name", "component"] and out["component"].dtype == np.int64
    assert out["id"].tolist() == [10, 20, 30, 40, 50, 60, 70] and out["name"].tolist() == list("abcdefg")
    assert out["component"].tolist() == [10, 10, 10, 40, 50, 60, 60]
    assert first["component"].tolist() == [10, 20, 30, 40, 50, 60, 70]      # GraphX: numIter = 1 writes nothing
    # round 1 trims 40 and 50 and colours all the rest by 10; only {10, 20, 30} is written in round 2
    assert second["component"].tolist() == [10, 10, 10, 40, 50, 60, 70]
    assert out.equals(gfa.strongly_connected_components(v, e, 10))
    assert out.equals(gfa.strongly_connected_components(v, e, maxIter=3))


def test_graphframe_string_ids(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    V = ig.num_vertices
    for r in (2, 50):
        want, _ = scc_ref.scc_rounds(V, ig.src, ig.dst, r)
        out = gfa.strongly_connected_components(v, e, r)
        assert list(out.columns) == ["id", "name", "component"] and out["component"].dtype == np.int64
        assert np.array_equal(out["id"].to_numpy(), ig.ids)
        assert np.array_equal(out["component"].to_numpy(), want)   # the dense index, as for `label`
