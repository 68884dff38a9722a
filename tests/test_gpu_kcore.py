"""k-core decomposition on the GPU (lpa_core_numbers, csrc/lpa_kcore.hip): every result bit-exact
against the numpy peel of tests/kcore_ref.py (core[v] = the largest k such that v lies in a
subgraph of the canonical simple undirected graph of minimum degree >= k), the simple degrees and
every summary field but `passes` (the schedule) with it.  The package's own calls on top:
GraphFrame.coreNumber and GraphFrame.kCore."""
import functools
import os

import numpy as np
import pandas as pd
import pytest

import kcore_ref as kc
from graphs import degree_mix, random_multigraph, star, two_cliques

pytestmark = pytest.mark.gpu

# the create-time overrides of the row forms and the in-block peel (DESIGN.md "k-core
# decomposition"), each at its smallest legal value
KC_ENV = ("LPA_KC_SHORT", "LPA_KC_WAVE", "LPA_KC_BLOCK")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r9_golden.npz")


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _r9():
    z = np.load(GOLDEN, allow_pickle=False)
    return int(z["ids"].size), z["src"], z["dst"]


GRAPHS = {
    "degree_mix": degree_mix,
    "rm2000": lambda: random_multigraph(2000, 30000, 1),
    "r9": _r9,
    "two_cliques": lambda: two_cliques(5),
}


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def ref(name):
    """The uncapped reference of a named graph, computed once, shared and read-only."""
    core, deg = kc.core_numbers(*graph(name))
    core.setflags(write=False)
    deg.setflags(write=False)
    return core, deg


def _check(gfa, V, s, d, ref=None, max_k=None):
    """core_numbers() of a fresh handle, plain and with stats, against the reference (ref: the
    UNCAPPED reference pair)."""
    s = np.asarray(s, dtype=np.int32)
    d = np.asarray(d, dtype=np.int32)
    if ref is None:
        ref = kc.core_numbers(V, s, d)
    rcore, rdeg = ref
    rsumm = kc.summary_of(rcore, rdeg, max_k)
    want = rcore if max_k is None else np.minimum(rcore, max_k)
    with gfa.Graph(s, d, V) as g:
        core = g.core_numbers(max_k=max_k)
        core2, deg, summ = g.core_numbers(max_k=max_k, stats=True)
    assert core.dtype == np.int32 and core.shape == (V,)
    bad = int((core != want).sum())
    assert bad == 0, f"{bad} of {V} core numbers differ from the reference"
    assert np.array_equal(core2, core)
    assert deg.dtype == np.int32 and deg.shape == (V,) and np.array_equal(deg, rdeg)
    assert tuple(summ) == kc.SUMMARY_KEYS
    assert {k: summ[k] for k in kc.PURE_KEYS} == rsumm
    assert summ["passes"] >= 0
    return core, summ


# ---- 1. degenerate ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        assert g.core_numbers().size == 0
        core, deg, summ = g.core_numbers(stats=True)
    assert core.size == 0 and deg.size == 0
    assert summ == dict.fromkeys(kc.SUMMARY_KEYS, 0)


def test_single_vertex(gfa):
    e = np.empty(0, np.int32)
    core, summ = _check(gfa, 1, e, e)
    assert core.tolist() == [0]
    assert (summ["degeneracy"], summ["main_core_size"], summ["levels"], summ["n_core0"]) == (0, 1, 1, 1)


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    core, summ = _check(gfa, 70, e, e)
    assert not core.any() and summ["simple_edges"] == 0 and summ["n_core0"] == 70 and summ["levels"] == 1


def test_only_self_loops(gfa):
    v = np.array([3, 3, 0, 99, 64, 64, 64], np.int32)
    core, summ = _check(gfa, 100, v, v)
    assert not core.any() and summ["simple_edges"] == 0 and summ["max_degree"] == 0


def test_one_edge_repeated(gfa):
    core, summ = _check(gfa, 9, np.full(1000, 6, np.int32), np.full(1000, 2, np.int32))
    assert core[6] == 1 and core[2] == 1 and core.sum() == 2
    assert summ["simple_edges"] == 1 and summ["n_core0"] == 7 and summ["levels"] == 2


def test_triangle_as_heavy_multigraph(gfa):
    """1000 copies of each edge in both directions, plus self-loops at the corners."""
    a = np.array([0, 1, 2, 1, 2, 0], np.int32)
    b = np.array([1, 2, 0, 0, 1, 2], np.int32)
    s = np.concatenate([np.tile(a, 1000), [0, 1, 2, 2]]).astype(np.int32)
    d = np.concatenate([np.tile(b, 1000), [0, 1, 2, 2]]).astype(np.int32)
    core, summ = _check(gfa, 3, s, d)
    assert core.tolist() == [2, 2, 2]
    assert (summ["degeneracy"], summ["main_core_size"], summ["simple_edges"], summ["max_degree"]) == (2, 3, 3, 2)


# ---- 2. closed forms with concurrency: where the claim rule can go wrong ----
def test_star(gfa):
    """The hub takes 5000 concurrent decrements from the seeds of level 1 and must be claimed exactly
    once, at level 1: its core is neither its final count nor anything lower.  A block-form row."""
    core, summ = _check(gfa, *star(5000))
    assert (core == 1).all()
    assert (summ["degeneracy"], summ["main_core_size"], summ["levels"], summ["max_degree"]) == (1, 5001, 1, 5000)


def test_k3_500(gfa):
    """Three hubs each take 500 decrements from the seeds of one level."""
    core, summ = _check(gfa, *kc.complete_bipartite(3, 500))
    assert (core == 3).all() and summ["levels"] == 1 and summ["main_core_size"] == 503


def test_clique_with_leaves(gfa):
    """K40, 100 pendant leaves on every member: the members' counts fall from 139 to 39 without a false
    claim, and the peel jumps over 37 empty levels."""
    core, summ = _check(gfa, *kc.clique_with_leaves(40, 100))
    assert (core[:40] == 39).all() and (core[40:] == 1).all()
    assert summ["levels"] == 2 and summ["degeneracy"] == 39 and summ["main_core_size"] == 40


def test_overshoot(gfa):
    """A vertex with 50 leaves and one edge into a triangle: its count falls from 51 to 1 at level 1."""
    core, summ = _check(gfa, *kc.overshoot(50))
    assert core.tolist() == [1, 2, 2, 2] + [1] * 50
    assert summ["levels"] == 2 and summ["main_core_size"] == 3


@pytest.mark.parametrize("n", [3, 5, 70])
def test_complete_graph(gfa, n):
    """K70's rows cross 64 lanes."""
    core, summ = _check(gfa, n, *kc.clique(n))
    assert (core == n - 1).all() and summ["levels"] == 1 and summ["main_core_size"] == n


def test_clique_chain(gfa):
    core, summ = _check(gfa, *kc.clique_chain(3, 12))
    assert np.bincount(core).tolist() == [0, 0] + list(range(3, 13))
    assert summ["levels"] == 10 and summ["degeneracy"] == 11 and summ["main_core_size"] == 12


def test_grid(gfa):
    """All cores 2, in 39 cascading sub-levels from the four corners."""
    core, summ = _check(gfa, *kc.grid(40, 40))
    assert (core == 2).all() and summ["levels"] == 1


def test_circulant(gfa):
    """C1000(1, 2): one level, every vertex a seed, nothing cascades."""
    core, summ = _check(gfa, *kc.circulant(1000, (1, 2)))
    assert (core == 4).all() and summ["levels"] == 1


def test_binary_tree(gfa):
    core, summ = _check(gfa, *kc.binary_tree(4095))
    assert (core == 1).all() and summ["levels"] == 1


# ---- 3. cascade ----
def test_path_cascades_inside_a_block(gfa):
    """A path of 5000 is 2500 sub-levels of two vertices.  Launched one by one they are 2500 host round
    trips; the in-block loop needs a handful.  A condition on the schedule, not a measurement."""
    core, summ = _check(gfa, *kc.path(5000))
    assert (core == 1).all() and summ["levels"] == 1
    assert summ["passes"] < 50, f"{summ['passes']} host round trips for a path of 5000"


def test_path_without_the_in_block_peel(gfa, monkeypatch):
    monkeypatch.setenv("LPA_KC_BLOCK", "0")
    core, summ = _check(gfa, *kc.path(300))
    assert (core == 1).all()
    assert summ["passes"] >= 150   # every sub-level was a launch: the knob was read


# ---- 4. kernel forms ----
@pytest.mark.parametrize("name", ["degree_mix", "rm2000", "r9"])
def test_forms_default(gfa, name):
    _check(gfa, *graph(name), ref=ref(name))


@pytest.mark.parametrize("env", KC_ENV + ("all",))
@pytest.mark.parametrize("name", ["degree_mix", "rm2000"])
def test_forms_forced(gfa, monkeypatch, name, env):
    """Each boundary at its smallest legal value (and all three at once: every row a block-form row,
    every sub-level a launch), so that small graphs reach every row form."""
    for e in KC_ENV if env == "all" else (env,):
        monkeypatch.setenv(e, "0")
    _check(gfa, *graph(name), ref=ref(name))


def test_sample_graph_histogram(gfa):
    V, s, d = graph("r9")
    with gfa.Graph(s, d, V) as g:
        core = g.core_numbers()
    assert np.bincount(core).tolist() == [0, 3430, 450, 202, 148, 164, 92, 73, 12, 42]


# ---- 5. API ----
@pytest.mark.parametrize("name", ["degree_mix", "r9", "two_cliques"])
def test_max_k(gfa, name):
    top = int(ref(name)[0].max())
    for max_k in (0, 1, 3, top, top + 5):
        _check(gfa, *graph(name), ref=ref(name), max_k=max_k)


def test_device_out(gfa):
    import torch

    V, s, d = graph("degree_mix")
    with gfa.Graph(s, d, V) as g:
        host = g.core_numbers()
        out = torch.full((V,), -1, dtype=torch.int32, device="cuda:0")
        assert g.core_numbers(out=out) is out
        assert np.array_equal(out.cpu().numpy(), host)
        out2 = torch.full((V,), -1, dtype=torch.int32, device="cuda:0")
        core, deg, summ = g.core_numbers(max_k=3, out=out2, stats=True)
        assert core is out2 and deg.dtype == torch.int32 and deg.is_cuda
        assert np.array_equal(out2.cpu().numpy(), np.minimum(host, 3))
        assert np.array_equal(deg.cpu().numpy(), ref("degree_mix")[1])
        assert summ["degeneracy"] == 3
        with pytest.raises(ValueError, match="int32"):
            g.core_numbers(out=torch.empty(V, dtype=torch.int64, device="cuda:0"))
        with pytest.raises(ValueError, match=f"{V} contiguous"):
            g.core_numbers(out=torch.empty(V + 1, dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError, match="device tensor"):
            g.core_numbers(out=np.empty(V, np.int32))


def test_two_calls_one_handle(gfa):
    V, s, d = graph("degree_mix")
    with gfa.Graph(s, d, V) as g:
        a, da, sa = g.core_numbers(stats=True)
        b, db, sb = g.core_numbers(stats=True)
    assert np.array_equal(a, b) and np.array_equal(da, db) and sa == sb


def test_lpa_state_untouched(gfa):
    V, s, d = graph("degree_mix")
    with gfa.Graph(s, d, V) as g:
        before = g.run(5)
        g.core_numbers()
        g.core_numbers(max_k=2)
        after = g.run(5)
        g.reset()
        g.step(2)
        g.core_numbers()
        g.step(3)
        stepped = g.labels()
    assert np.array_equal(before, after) and np.array_equal(before, stepped)


def _frames(ids, s, d, rng=None):
    """Vertex and edge tables over the id values ids[dense]; rows scrambled when rng is given."""
    v = pd.DataFrame({"id": ids, "name": [f"n{i}" for i in range(len(ids))]})
    e = pd.DataFrame({"src": ids[s], "dst": ids[d], "w": np.arange(len(s), dtype=np.float64)})
    if rng is not None:
        v = v.iloc[rng.permutation(len(v))].reset_index(drop=True)
    return v, e


def test_core_number_integral_ids(gfa):
    V, s, d = graph("two_cliques")
    ids = np.arange(V, dtype=np.int64) * 7 + 100
    v, e = _frames(ids, s, d, np.random.default_rng(1))
    out = gfa.GraphFrame(v, e).coreNumber()
    assert list(out.columns) == ["id", "name", "core"] and out["core"].dtype == np.int64
    assert out["id"].tolist() == ids.tolist()
    assert out["name"].tolist() == [f"n{i}" for i in range(V)]
    assert out["core"].tolist() == ref("two_cliques")[0].tolist()
    assert out.attrs["degeneracy"] == 5 and out.attrs["core_sizes"] == np.bincount(ref("two_cliques")[0]).tolist()
    fn = gfa.core_number(v, e)
    assert fn.equals(out) and fn.attrs == out.attrs


def test_core_number_string_ids(gfa):
    V, s, d = graph("two_cliques")
    ids = np.array([f"v{i:03d}" for i in range(V)], dtype=object)
    v, e = _frames(ids, s, d, np.random.default_rng(2))
    out = gfa.GraphFrame(v, e).coreNumber()
    assert out["id"].tolist() == ids.tolist() and out["core"].tolist() == ref("two_cliques")[0].tolist()


def test_k_core_of_the_sample(gfa):
    V, s, d = graph("r9")
    core = ref("r9")[0]
    ids = np.arange(V, dtype=np.int64) * 3 + 5
    v, e = _frames(ids, s, d, np.random.default_rng(3))
    gf = gfa.GraphFrame(v, e)
    sub = gf.kCore(3)
    assert isinstance(sub, gfa.GraphFrame)
    inside = core >= 3
    assert sub.vertices["id"].tolist() == ids[inside].tolist()
    assert list(sub.vertices.columns) == ["id", "name", "core"] and (sub.vertices["core"] == 3).all()
    assert sub.vertices["name"].tolist() == [f"n{i}" for i in np.flatnonzero(inside)]
    keep = inside[s] & inside[d]
    assert list(sub.edges.columns) == ["src", "dst", "w"]
    assert sub.edges["w"].tolist() == np.flatnonzero(keep).astype(np.float64).tolist()
    assert sub.edges["src"].tolist() == ids[s[keep]].tolist() and sub.edges["dst"].tolist() == ids[d[keep]].tolist()
    # the 3-core of the 3-core is itself, and it feeds the detectors unchanged
    again = sub.kCore(3)
    assert again.vertices["id"].tolist() == sub.vertices["id"].tolist() and len(again.edges) == len(sub.edges)
    lab = sub.labelPropagation(2)
    assert len(lab) == int(inside.sum()) and "label" in lab.columns
    fn = gfa.k_core(v, e, 3)
    assert fn.vertices.equals(sub.vertices) and fn.edges.equals(sub.edges)
    sub.close()
    again.close()
    gf.close()


def test_k_core_keeps_duplicates_and_loops(gfa):
    """The induced sub-MULTIgraph: repeats and self-loops among the survivors stay."""
    V, s, d = 6, np.array([0, 1, 2, 0, 0, 1, 1, 3, 4, 4, 5], np.int32), np.array([1, 2, 0, 1, 0, 1, 3, 4, 4, 5, 5], np.int32)
    v, e = _frames(np.arange(V, dtype=np.int64), s, d)
    sub = gfa.GraphFrame(v, e).kCore(2)
    assert sub.vertices["id"].tolist() == [0, 1, 2]
    assert sub.edges["w"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]


def test_k_core_bounds(gfa):
    V, s, d = graph("two_cliques")
    v, e = _frames(np.arange(V, dtype=np.int64), s, d)
    gf = gfa.GraphFrame(v, e)
    everything = gf.kCore(0)
    assert len(everything.vertices) == V and len(everything.edges) == len(e) and not everything.vertices["core"].any()
    nothing = gf.kCore(6)   # the degeneracy is 5
    assert len(nothing.vertices) == 0 and len(nothing.edges) == 0
    assert list(nothing.vertices.columns) == ["id", "name", "core"] and list(nothing.edges.columns) == ["src", "dst", "w"]
    top = gf.kCore(5)
    assert top.vertices["id"].tolist() == [5, 6, 7, 8, 9, 10]
    gf.close()
