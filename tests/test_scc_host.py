"""Strongly connected components, the part that needs no GPU: the C-ABI boundary of
lpa_strongly_connected_components, the exported names, the argument checks of
GraphFrame.stronglyConnectedComponents and Graph.strongly_connected_components (they run
before any device work), and the two CPU references of tests/scc_ref.py (GraphX's rounds in
numpy; an iterative Tarjan) checked against each other and against closed forms."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import scc_ref
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph, two_cliques


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_strongly_connected_components(None, 5, None, 0, None, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_scc():
    assert _lib.load().lpa_abi_version() >= 12


def test_summary_struct_layout():
    s = _lib.LpaSccSummary(1, 2, 3, 4, 5, 6, 7)
    assert s.to_dict() == dict(n_components=1, n_singletons=2, largest_size=3, largest_id=4, rounds=5, trimmed=6,
                               unresolved=7)
    assert ctypes.sizeof(_lib.LpaSccSummary) == 56


def test_function_form_exported():
    assert "strongly_connected_components" in gfa.__all__
    assert callable(gfa.strongly_connected_components)
    assert callable(gfa.GraphFrame.stronglyConnectedComponents)
    assert callable(gfa.Graph.strongly_connected_components)


# ---- argument checks: none of them reaches the device ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": np.array([30, 10, 20], np.int64), "name": ["c", "a", "b"]})
    e = pd.DataFrame({"src": np.array([10, 20], np.int64), "dst": np.array([20, 30], np.int64)})
    f = gfa.GraphFrame(v, e)
    yield f
    assert f._graph is None   # no handle was ever built


@pytest.mark.parametrize("bad", [0, -3])
def test_max_iter_must_be_positive(gf, bad):
    msg = f"requirement failed: Number of iterations must be greater than 0, but got {bad}"
    with pytest.raises(ValueError, match=msg):
        gf.stronglyConnectedComponents(bad)
    with pytest.raises(ValueError, match=msg):
        gfa.strongly_connected_components(gf.vertices, gf.edges, bad)
    with pytest.raises(ValueError, match="greater than 0"):
        gfa.Graph.strongly_connected_components(None, bad)


@pytest.mark.parametrize("bad", [2.5, True, "3", None, np.float64(4), np.bool_(True)])
def test_max_iter_must_be_an_int(gf, bad):
    with pytest.raises(TypeError, match="maxIter"):
        gf.stronglyConnectedComponents(bad)
    with pytest.raises(TypeError, match="maxIter"):
        gfa.strongly_connected_components(gf.vertices, gf.edges, bad)
    if bad is not None:   # None: run to convergence
        with pytest.raises(TypeError, match="max_iter"):
            gfa.Graph.strongly_connected_components(None, bad)


def test_max_iter_is_required(gf):
    with pytest.raises(TypeError):
        gf.stronglyConnectedComponents()


# ---- the two reference forms ----
def _both(V, s, d):
    comp, summ = scc_ref.scc_rounds(V, s, d, max_iter=V + 1)
    assert comp.dtype == np.int32 and comp.shape == (V,)
    assert np.array_equal(comp, scc_ref.scc_tarjan(V, s, d))
    assert summ["unresolved"] == 0 and 1 <= summ["rounds"] <= V + 1
    assert np.array_equal(comp[comp], comp) and (comp <= np.arange(V)).all()
    return comp, summ


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_references_agree_on_random_multigraph(seed):
    V, s, d = random_multigraph(400, 500 + 150 * seed, seed)
    comp, summ = _both(V, s, d)
    assert 1 < summ["n_components"] < V


def test_references_agree_on_degree_mix():
    comp, summ = _both(*degree_mix())
    assert summ["largest_size"] > 1 and summ["trimmed"] > 0


def test_references_agree_on_two_cliques():
    V, s, d = two_cliques(5)
    comp, summ = _both(V, s, d)
    assert comp.tolist() == [0] * 5 + [5] * 6   # the bridge 0 -> 5 is directed: two SCCs
    assert summ["n_components"] == 2 and summ["trimmed"] == 0


def test_references_agree_on_r9(golden):
    V = int(golden["ids"].size)
    comp, summ = _both(V, golden["src"], golden["dst"])
    assert summ["n_components"] == np.unique(comp).size


# ---- the rounds: what max_iter cuts off ----
def test_chain_ascending_resolves_one_scc_a_round():
    """S_0 holds the smallest ids and reaches every other SCC: every round colours the whole
    alive chain by its head and peels that one SCC."""
    k = 20
    V, s, d = scc_ref.chain_of_2cycles(k, ascending=True)
    odd = 2 * np.arange(k) + 1
    for r in range(1, k + 3):
        comp, summ = scc_ref.scc_rounds(V, s, d, max_iter=r)
        done = comp[odd] == odd - 1            # SCC i is resolved: 2i + 1 holds 2i
        assert (comp[odd][~done] == odd[~done]).all() and (comp[odd - 1] == odd - 1).all()
        assert done.tolist() == [i < r - 1 for i in range(k)]
        assert summ["rounds"] == min(r, k + 1) and summ["unresolved"] == 2 * (k - int(done.sum()))
        assert summ["trimmed"] == 0
    comp, summ = scc_ref.scc_rounds(V, s, d, max_iter=k + 1)
    assert summ["rounds"] == k + 1 and summ["unresolved"] == 0
    assert np.array_equal(comp, scc_ref.scc_tarjan(V, s, d))
    assert scc_ref.scc_rounds(V, s, d)[1] == summ


def test_chain_descending_converges_in_two_rounds():
    """Every SCC's smallest member is smaller than anything upstream: all are roots at once."""
    V, s, d = scc_ref.chain_of_2cycles(20, ascending=False)
    comp, summ = scc_ref.scc_rounds(V, s, d)
    assert summ["rounds"] == 2 and summ["unresolved"] == 0 and summ["n_components"] == 20
    assert np.array_equal(comp, scc_ref.scc_tarjan(V, s, d))
    ident, one = scc_ref.scc_rounds(V, s, d, max_iter=1)
    assert np.array_equal(ident, np.arange(V)) and one["rounds"] == 1 and one["unresolved"] == V


def test_self_loop_changes_the_round_not_the_result():
    """0 -> 1 <-> 2.  Without a loop 0 is trimmed in round 1 and {1, 2} is written in round 2;
    with 0 -> 0 it stays, colours {1, 2} with 0, is written alone in round 2, {1, 2} in round 3."""
    s, d = [0, 1, 2], [1, 2, 1]
    plain, ps = scc_ref.scc_rounds(3, s, d)
    looped, ls = scc_ref.scc_rounds(3, s + [0], d + [0])
    assert plain.tolist() == looped.tolist() == [0, 1, 1]
    assert ps["rounds"] == 2 and ps["trimmed"] == 1
    assert ls["rounds"] == 3 and ls["trimmed"] == 0


def test_closed_forms():
    V, s, d = scc_ref.path(2000)
    comp, summ = scc_ref.scc_rounds(V, s, d)
    assert np.array_equal(comp, np.arange(V)) and summ["rounds"] == 1 and summ["trimmed"] == V
    V, s, d = scc_ref.cycle(1000, rotate=333)
    comp, summ = scc_ref.scc_rounds(V, s, d)
    assert (comp == 0).all() and summ["rounds"] == 2 and summ["largest_size"] == V and summ["largest_id"] == 0
    V, s, d = scc_ref.wheel(50)
    assert (scc_ref.scc_rounds(V, s, d)[0] == 0).all()
    e = np.empty(0, np.int32)
    assert scc_ref.scc_rounds(0, e, e)[1] == dict(n_components=0, n_singletons=0, largest_size=0, largest_id=-1,
                                                  rounds=0, trimmed=0, unresolved=0)
    # only self-loops: nothing to trim, all roots in round 1, written in round 2
    comp, summ = scc_ref.scc_rounds(4, [0, 1, 2, 3], [0, 1, 2, 3])
    assert comp.tolist() == [0, 1, 2, 3] and summ["rounds"] == 2 and summ["trimmed"] == 0
