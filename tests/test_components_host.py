"""Connected components, the part that needs no GPU: the C-ABI boundary of
lpa_components, the GraphFrames-compatible argument check of connectedComponents, and the
numpy reference (tests/cc_ref.py) the GPU tests compare with, checked here against scipy
and against the recorded LPA labels (a label never leaves its component)."""
import numpy as np
import pandas as pd
import pytest

import cc_ref
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_components(None, None, 0, None, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_components():
    assert _lib.load().lpa_abi_version() >= 8


def test_summary_struct_layout():
    s = _lib.LpaComponentsSummary(1, 2, 3, 4)
    assert s.to_dict() == dict(n_components=1, n_singletons=2, largest_size=3, largest_id=4)
    import ctypes

    assert ctypes.sizeof(s) == 32


def _tiny_frame():
    return gfa.GraphFrame(pd.DataFrame({"id": [1, 2]}), pd.DataFrame({"src": [1], "dst": [2]}))


def test_algorithm_checked_before_device():
    with pytest.raises(ValueError, match=r"Supported algorithms are \{graphx, graphframes\}: bogus"):
        _tiny_frame().connectedComponents(algorithm="bogus")


def test_no_device_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.LpaError, match="device"):
        _tiny_frame().connectedComponents()
    with pytest.raises(_lib.LpaError, match="device"):
        gfa.connected_components(pd.DataFrame({"id": [1, 2]}), pd.DataFrame({"src": [1], "dst": [2]}))


def test_function_form_exported():
    assert "connected_components" in gfa.__all__
    assert callable(gfa.connected_components)


def _scipy_min_labels(V, s, d):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components

    a = sp.coo_matrix((np.ones(s.size, np.int8), (s, d)), shape=(V, V)).tocsr()
    n, lab = connected_components(a, directed=False)
    lo = np.full(n, V, np.int64)
    np.minimum.at(lo, lab, np.arange(V))
    return lo[lab]


@pytest.mark.parametrize("name, n_comp, largest, n_single", [
    ("r9", 34, 4440, 0),
    ("random", 57312, 116251, None),
    ("degree_mix", 8, 3047, None),
])
def test_reference_equals_scipy(golden, name, n_comp, largest, n_single):
    if name == "r9":
        V, s, d = int(golden["ids"].size), golden["src"], golden["dst"]
    elif name == "random":
        V, s, d = random_multigraph(200000, 150000, 3)
    else:
        V, s, d = degree_mix()
    comp = cc_ref.components(V, s, d)
    assert comp.dtype == np.int64 and comp.shape == (V,)
    sizes, summ = cc_ref.summary(comp)
    assert summ["n_components"] == n_comp and summ["largest_size"] == largest
    if n_single is not None:
        assert summ["n_singletons"] == n_single
    assert sizes.sum() == V and comp[summ["largest_id"]] == summ["largest_id"]
    assert np.array_equal(comp, _scipy_min_labels(V, s, d))


def test_reference_small_cases():
    # direction, duplicates, self-loops make no difference; an edgeless vertex is alone
    s = np.array([4, 4, 2, 3, 3, 5], np.int32)
    d = np.array([1, 1, 2, 6, 6, 3], np.int32)
    assert cc_ref.components(8, s, d).tolist() == [0, 1, 2, 3, 1, 3, 3, 7]
    assert cc_ref.components(3, s[:0], d[:0]).tolist() == [0, 1, 2]
    assert cc_ref.components(0, s[:0], d[:0]).size == 0
    sizes, summ = cc_ref.summary(cc_ref.components(8, s, d))
    assert sizes.tolist() == [1, 2, 1, 3, 0, 0, 0, 1]
    assert summ == dict(n_components=5, n_singletons=3, largest_size=3, largest_id=3)
    # a scrambled path: many hooking rounds
    rng = np.random.default_rng(0)
    p = rng.permutation(4096)
    assert not cc_ref.components(4096, p[:-1], p[1:]).any()


def test_lpa_labels_stay_inside_components(golden):
    V = int(golden["ids"].size)
    comp = cc_ref.components(V, golden["src"], golden["dst"])
    for k, lab in enumerate(golden["labels_iter"]):
        assert np.array_equal(comp[lab], comp), f"superstep {k + 1}: a label left its component"
