"""lpa_louvain on the GPU (csrc/lpa_louvain.hip) against the CPU restatement tests/louvain_ref.py:
exact equality of comm, sizes, every level row and every integer of the summary; modularity to
1e-12 absolute."""
import functools
import os

import numpy as np
import pandas as pd
import pytest

import louvain_ref as lv
from graphs import degree_mix, outlier_l1_np, random_multigraph, star, two_cliques

pytestmark = pytest.mark.gpu

LV_OVERRIDES = [{}, {"LPA_LV_SHORT": "0"}, {"LPA_LV_WAVE": "0"}, {"LPA_LV_SHORT": "0", "LPA_LV_WAVE": "0"},
                {"LPA_LV_SHORT": "100000"}]
LV_IDS = ["defaults", "short0", "wave0", "both0", "all-short"]
# the LDS tables cut down: a wave or block row of more than half the slots takes the spill table
SPILL_OVERRIDES = [{"LPA_LV_TABLE": "16"}, {"LPA_LV_TABLE": "0"},
                   {"LPA_LV_TABLE": "64", "LPA_LV_SHORT": "4", "LPA_LV_WAVE": "40"}]
SPILL_IDS = ["table16", "table0", "table64-short4-wave40"]


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def ladder(n=300):
    """The threshold graph i ~ j iff i + j >= n: list lengths 0, 1, ..., n - 2, every one of them."""
    i, j = np.triu_indices(n, 1)
    keep = i + j >= n
    return n, i[keep].astype(np.int32), j[keep].astype(np.int32)


def block_edge_hubs(cap=4096):
    """Two joined hubs of cap / 2 and cap / 2 + 1 distinct neighbours (the last list length the
    block form's LDS table takes, and the first it spills), their leaves tied in pairs."""
    h = cap // 2
    leaves0 = 2 + np.arange(h - 1)
    leaves1 = 2 + (h - 1) + np.arange(h)
    s = np.concatenate([np.zeros(h - 1, np.int64), np.ones(h, np.int64), leaves0[:-1:2], leaves1[:-1:2], [0]])
    d = np.concatenate([leaves0, leaves1, leaves0[1::2], leaves1[1::2], [1]])
    return 2 + 2 * h - 1, s.astype(np.int32), d.astype(np.int32)


def heavy_two_cliques(times=3000):
    """two_cliques(5) with every edge repeated: a few neighbour communities, large weights."""
    V, s, d = two_cliques(5)
    return V, np.tile(s, times), np.tile(d, times)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r9_golden.npz")


def _r9():
    z = np.load(GOLDEN, allow_pickle=False)
    return int(z["ids"].size), z["src"], z["dst"]


GRAPHS = {
    "empty": lambda: (0, np.empty(0, np.int32), np.empty(0, np.int32)),
    "one_vertex": lambda: (1, np.empty(0, np.int32), np.empty(0, np.int32)),
    "edgeless70": lambda: (70, np.empty(0, np.int32), np.empty(0, np.int32)),
    "loops_only": lambda: (5, np.array([0, 1, 1, 3], np.int32), np.array([0, 1, 1, 3], np.int32)),
    "edge_x1000": lambda: (3, np.full(1000, 2, np.int32), np.full(1000, 1, np.int32)),
    "edge": lambda: (2, np.array([0], np.int32), np.array([1], np.int32)),
    "path4": lambda: lv.path(4),
    "two_cliques": lambda: two_cliques(5),
    "star5000": lambda: star(5000),
    "ring": lambda: lv.ring_of_cliques(30, 5),
    "path200": lambda: lv.path(200),
    "cycle1000": lambda: lv.cycle(1000),
    "ladder": ladder,
    "block_edge_hubs": block_edge_hubs,
    "star70000": lambda: star(70000),
    "degree_mix": degree_mix,
    "heavy_two_cliques": heavy_two_cliques,
    "r9": _r9,
    "rm2000": lambda: random_multigraph(2000, 60000, 7),
    "rm20000": lambda: random_multigraph(20000, 200000, 3),
}


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def ref(name, max_levels=64, max_rounds=1000):
    """The reference of a case, computed once and shared: a max_levels prefix is read from the
    trace of the full run."""
    if max_levels < 64 and max_rounds == 1000:
        full = ref(name)
        return _trace[name][max_levels - 1] if max_levels < len(_trace[name]) else full
    trace = []
    out = lv.louvain(*graph(name), max_levels=max_levels, max_rounds=max_rounds, trace=trace)
    if max_levels == 64 and max_rounds == 1000:
        _trace[name] = trace
    return out


_trace = {}


def _compare(got, want, V):
    comm, sizes, levels, summ = got
    rcomm, rlevels, rsumm = want
    assert comm.dtype == np.int32 and np.array_equal(comm, rcomm)
    assert sizes.dtype == np.int64 and np.array_equal(sizes, np.bincount(rcomm, minlength=V))
    assert levels == rlevels
    for key in lv.SUMMARY_KEYS[:-1]:
        assert summ[key] == rsumm[key], key
    assert abs(summ["modularity"] - rsumm["modularity"]) <= 1e-12


def _run(gfa, name, **kw):
    V, s, d = graph(name)
    with gfa.Graph(s, d, V) as g:
        got = g.louvain(stats=True, **kw)
        assert np.array_equal(g.louvain(**kw), got[0])
    _compare(got, ref(name, **kw), V)
    return got


# ---- 1. degenerate ----
@pytest.mark.parametrize("name", ["empty", "one_vertex", "edgeless70", "loops_only", "edge_x1000"])
def test_degenerate(gfa, name):
    V = graph(name)[0]
    comm, sizes, levels, summ = _run(gfa, name)
    if name == "edge_x1000":
        assert comm.tolist() == [0, 1, 1] and summ["arcs"] == 2000 and summ["levels"] == 1
    else:
        assert np.array_equal(comm, np.arange(V)) and levels == [] and summ["rounds"] == 0
        assert summ["largest_id"] == (0 if V else -1)


# ---- 2. closed forms (path200 and cycle1000: the many-rounds cases) ----
@pytest.mark.parametrize("name", ["edge", "path4", "two_cliques", "star5000", "ring", "path200", "cycle1000"])
def test_closed_forms(gfa, name):
    comm, sizes, levels, summ = _run(gfa, name)
    rows = [(r["rounds"], r["moves"], r["communities"]) for r in levels]
    want = {"edge": [(1, 1, 1)], "path4": [(1, 2, 2)], "two_cliques": [(2, 9, 2)], "star5000": [(1, 5000, 1)],
            "ring": [(2, 120, 30)], "path200": [(99, 9802, 100), (49, 2402, 50), (24, 577, 25), (11, 133, 13)],
            "cycle1000": [(500, 249999, 500)]}[name]
    assert rows[:len(want)] == want
    if name == "ring":
        assert np.array_equal(comm, 5 * (np.arange(150) // 5)) and round(summ["modularity"], 6) == 0.875758
    if name == "cycle1000":
        assert summ["n_communities"] == 31


def test_max_rounds_bounds_a_level(gfa):
    _run(gfa, "path200", max_levels=1, max_rounds=1)
    got = _run(gfa, "path200", max_levels=5, max_rounds=1)
    assert [r["rounds"] for r in got[2]] == [1] * 5


# ---- 3. row forms: every list length across the boundaries, every form forced ----
@pytest.mark.parametrize("env", LV_OVERRIDES, ids=LV_IDS)
def test_form_boundaries(gfa, monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    V, s, d = graph("ladder")
    lens = np.bincount(np.concatenate([s, d]), minlength=V)
    assert set(range(0, 258)) <= set(lens.tolist())   # 0 .. 32, 33 .. 256, 257 and on
    _run(gfa, "ladder")
    _run(gfa, "two_cliques")


def test_block_table_edge(gfa):
    V, s, d = graph("block_edge_hubs")
    lens = np.bincount(np.concatenate([s, d]), minlength=V)
    assert lens[0] == 2048 and lens[1] == 2049   # kLvBlockSlots / 2 and one more
    _run(gfa, "block_edge_hubs")


# ---- 4. spill ----
def test_spill_star(gfa):
    """One row of 70 000 distinct communities at level 0: no LDS table holds it."""
    comm, sizes, levels, summ = _run(gfa, "star70000")
    assert (comm == 0).all() and [(r["rounds"], r["moves"], r["communities"]) for r in levels] == [(1, 70000, 1)]


@pytest.mark.parametrize("env", SPILL_OVERRIDES, ids=SPILL_IDS)
def test_spill_small_tables(gfa, monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    _run(gfa, "degree_mix")
    _run(gfa, "ladder")


def test_heavy_weights_few_communities(gfa):
    comm, sizes, levels, summ = _run(gfa, "heavy_two_cliques")
    assert comm.tolist() == [0] * 5 + [5] * 6 and summ["arcs"] == 2 * graph("heavy_two_cliques")[1].size


# ---- 5. weighted levels ----
@pytest.mark.parametrize("max_levels", [1, 2, 64])
@pytest.mark.parametrize("name", ["r9", "rm2000", "rm20000", "degree_mix"])
def test_weighted_levels(gfa, name, max_levels):
    got = _run(gfa, name, max_levels=max_levels)
    if max_levels == 64 and name == "r9":
        assert got[3]["n_communities"] == 123 and [r["rounds"] for r in got[2]] == [12, 9, 2]


# ---- 6. determinism ----
def test_bit_identical_across_edge_orders_directions_and_calls(gfa):
    V, s, d = graph("rm2000")
    m = s.size
    perm = np.random.default_rng(9).permutation(m)
    # duplicates are neighbours after a sort by (src, dst); a stride coprime to m moves them apart
    by_key = np.lexsort((d, s))
    stride = 7919
    assert np.gcd(stride, m) == 1
    apart = by_key[(np.arange(m, dtype=np.int64) * stride) % m]
    assert np.array_equal(np.sort(apart), np.arange(m))
    want = ref("rm2000")
    for order in (np.arange(m), np.arange(m)[::-1], perm, apart):
        with gfa.Graph(s[order].copy(), d[order].copy(), V) as g:
            _compare(g.louvain(stats=True), want, V)
    with gfa.Graph(d, s, V) as g:
        _compare(g.louvain(stats=True), want, V)
        _compare(g.louvain(stats=True), want, V)
    flip = np.random.default_rng(4).random(m) < 0.5
    with gfa.Graph(np.where(flip, d, s), np.where(flip, s, d), V) as g:
        _compare(g.louvain(stats=True), want, V)


# ---- 7. ties with the rest of the library ----
def test_quality_agrees(gfa):
    for name in ("r9", "degree_mix"):
        V, s, d = graph(name)
        with gfa.Graph(s, d, V) as g:
            comm, sizes, levels, summ = g.louvain(stats=True)
            q = g.quality(comm)
        assert (q["n_communities"], q["intra_arcs"], q["arcs"]) == (summ["n_communities"], summ["intra_arcs"],
                                                                  summ["arcs"])
        assert abs(q["modularity"] - summ["modularity"]) <= 1e-12


def test_does_not_disturb_lpa(gfa):
    V, s, d = graph("degree_mix")
    with gfa.Graph(s, d, V) as g:
        want = g.run(3)
    with gfa.Graph(s, d, V) as g:
        g.reset()
        g.step(1)
        before = g.info()["device_bytes"]
        c1 = g.louvain()
        assert g.info()["device_bytes"] == before
        g.step(1)
        got2 = g.louvain(stats=True)
        assert g.info()["device_bytes"] == before
        g.step(1)
        got = g.labels()
    assert np.array_equal(got, want)
    assert np.array_equal(c1, got2[0])
    _compare(got2, ref("degree_mix"), V)


def test_device_tensors(gfa):
    import torch

    V, s, d = graph("r9")
    want = ref("r9")
    with gfa.Graph(s, d, V) as g:
        dev = torch.device("cuda", g.device)
        out = torch.full((V,), -1, dtype=torch.int32, device=dev)
        assert g.louvain(out=out) is out
        assert np.array_equal(out.cpu().numpy(), want[0])
        out.fill_(-1)
        comm, sizes, levels, summ = g.louvain(out=out, stats=True)
        assert comm is out and sizes.is_cuda and sizes.dtype == torch.int64
        _compare((out.cpu().numpy(), sizes.cpu().numpy(), levels, summ), want, V)
        with pytest.raises(ValueError, match="int32"):
            g.louvain(out=torch.empty(V, dtype=torch.int64, device=dev))
        with pytest.raises(ValueError, match=f"{V}"):
            g.louvain(out=torch.empty(V - 1, dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match=f"{V}"):
            g.louvain(out=torch.empty(V + 1, dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match="contiguous"):
            g.louvain(out=torch.empty(2 * V, dtype=torch.int32, device=dev)[::2])
        with pytest.raises(ValueError, match="device tensor"):
            g.louvain(out=np.empty(V, np.int32))
        # the C ABI's own argument checks
        lib, h = g._lib, g._handle()
        buf = np.empty(V, np.int32)
        assert lib.lpa_louvain(h, 0, 5, buf.ctypes.data, 0, None, None, 0, None) == -22
        assert lib.lpa_louvain(h, 5, 0, buf.ctypes.data, 0, None, None, 0, None) == -22
        assert lib.lpa_louvain(h, 5, 5, None, 0, None, None, 0, None) == -22
        assert lib.lpa_louvain(h, 5, 5, buf.ctypes.data, 0, None, None, 3, None) == -22


def test_two_loopback_ranks(gfa):
    V, s, d = graph("degree_mix")
    want = ref("degree_mix")
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        _compare(ranks[0].louvain(stats=True), want, V)
        with pytest.raises(ValueError, match="rank 0"):
            ranks[1].louvain()
    finally:
        for g in ranks:
            g.close()
        lb.close()


# ---- 8. drop-in ----
def test_graphframe_string_ids(gfa, golden):
    ids = golden["ids"]
    v = pd.DataFrame({"id": ids, "name": golden["names"]})
    e = pd.DataFrame({"src": ids[golden["src"]], "dst": ids[golden["dst"]]})
    ig = gfa.index_graph(v, e)
    rcomm, rlevels, rsumm = lv.louvain(ig.num_vertices, ig.src, ig.dst)
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.louvain()
        res = gf.outlierScores(labels=out, mode="L1")
    finally:
        gf.close()
    assert list(out.columns) == ["id", "name", "label"] and out["label"].dtype == np.int64
    assert np.array_equal(out["id"].to_numpy(), ig.ids)
    assert np.array_equal(out["label"].to_numpy(), rcomm)        # dense indices for string ids
    assert out.attrs["levels"] == rlevels and abs(out.attrs["modularity"] - rsumm["modularity"]) <= 1e-12
    assert out.equals(gfa.louvain(v, e))
    size, inc, flags, summ = outlier_l1_np(ig.num_vertices, ig.src, ig.dst, rcomm)
    assert list(res.vertices.columns) == ["id", "name", "label", "outlier"]
    assert np.array_equal(res.vertices["label"].to_numpy(), rcomm)
    assert np.array_equal(res.vertices["outlier"].to_numpy().astype(bool), flags)
    assert np.array_equal(res.flagged_ids, ig.ids[np.flatnonzero(flags)])
    present = np.flatnonzero(size > 0)
    assert np.array_equal(res.communities["label"].to_numpy(), present)
    assert np.array_equal(res.communities["size"].to_numpy(), size[present])
    assert np.array_equal(res.communities["incident_edges"].to_numpy(), inc[present])
    assert res.summary["n_flagged"] == summ["n_flagged"] and res.summary["n_groups"] == summ["n_groups"] == 123


def test_graphframe_integral_ids(gfa):
    """Two triangles 10-20-30 and 40-50-60 joined by 30-40, and a dangling 60 -> 99."""
    v = pd.DataFrame({"id": np.array([60, 10, 20, 30, 40, 50], np.int64), "name": list("fabcde")})
    e = pd.DataFrame({"src": np.array([10, 20, 30, 40, 50, 60, 30, 60], np.int64),
                      "dst": np.array([20, 30, 10, 50, 60, 40, 40, 99], np.int64)})
    gf = gfa.GraphFrame(v, e)
    try:
        out = gf.louvain()
        out2 = gf.louvain(maxLevels=1, maxRounds=1)
    finally:
        gf.close()
    assert list(out.columns) == ["id", "name", "label"]
    assert out["id"].tolist() == [10, 20, 30, 40, 50, 60] and out["name"].tolist() == list("abcdef")
    rcomm, rlevels, rsumm = lv.louvain(6, [0, 1, 2, 3, 4, 5, 2], [1, 2, 0, 4, 5, 3, 3])
    assert out["label"].tolist() == (10 * (rcomm + 1)).tolist() == [10, 10, 10, 40, 40, 40]
    assert out.attrs["levels"] == rlevels
    r1 = lv.louvain(6, [0, 1, 2, 3, 4, 5, 2], [1, 2, 0, 4, 5, 3, 3], max_levels=1, max_rounds=1)
    assert out2["label"].tolist() == (10 * (r1[0] + 1)).tolist() and out2.attrs["levels"] == r1[1]
