"""Triangle counting, the part that needs no GPU: the C-ABI boundary of
lpa_triangle_count, the exported names, and the two CPU references of tests/tc_ref.py
(scipy sparse products; oriented lists with np.intersect1d) checked against each other and
against the recorded values of the R9 sample."""
import ctypes

import numpy as np

import tc_ref
import graphframes_amd as gfa
from graphframes_amd import _lib
from graphs import degree_mix, random_multigraph


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_triangle_count(None, None, None, 0, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_triangle_count():
    assert _lib.load().lpa_abi_version() >= 9


def test_summary_struct_layout():
    s = _lib.LpaTriangleSummary(1, 2, 3, 4, 5, 6)
    assert s.to_dict() == dict(n_triangles=1, simple_edges=2, wedges=3, n_in_triangle=4, max_count=5,
                               max_count_id=6)
    assert ctypes.sizeof(_lib.LpaTriangleSummary) == 48


def test_function_form_exported():
    assert "triangle_count" in gfa.__all__
    assert callable(gfa.triangle_count)
    assert callable(gfa.GraphFrame.triangleCount) and callable(gfa.GraphFrame.clusteringCoefficient)
    assert callable(gfa.Graph.triangle_count)


def _both(V, s, d):
    c1, d1 = tc_ref.triangles(V, s, d)
    c2, d2 = tc_ref.triangles_oriented(V, s, d)
    assert c1.dtype == np.int64 and c1.shape == (V,) and d1.dtype == np.int64 and d1.shape == (V,)
    assert np.array_equal(c1, c2) and np.array_equal(d1, d2)
    assert int(c1.sum()) % 3 == 0
    return c1, d1


def test_references_agree_on_r9(golden):
    V = int(golden["ids"].size)
    count, deg = _both(V, golden["src"], golden["dst"])
    assert tc_ref.summary(count, deg) == dict(n_triangles=2834, simple_edges=7606, wedges=492280,
                                              n_in_triangle=749, max_count=226, max_count_id=3447)
    assert int(deg.max()) == 521


def test_references_agree_on_degree_mix():
    V, s, d = degree_mix()
    count, deg = _both(V, s, d)
    assert tc_ref.summary(count, deg) == dict(n_triangles=13736, simple_edges=23002, wedges=3368604,
                                              n_in_triangle=2673, max_count=11868, max_count_id=616)


def test_references_agree_on_random_multigraph():
    V, s, d = random_multigraph(2000, 60000, 7)
    count, deg = _both(V, s, d)
    summ = tc_ref.summary(count, deg)
    assert summ["n_triangles"] == 34233 and summ["n_in_triangle"] == V


def test_reference_small_cases():
    # direction, duplicates and self-loops make no difference
    s = np.array([0, 1, 2, 0, 1, 1, 3, 3], np.int32)
    d = np.array([1, 2, 0, 1, 0, 1, 3, 0], np.int32)
    for f in (tc_ref.triangles, tc_ref.triangles_oriented):
        count, deg = f(5, s, d)
        assert count.tolist() == [1, 1, 1, 0, 0] and deg.tolist() == [3, 2, 2, 1, 0]
        count, deg = f(3, s[:0], d[:0])
        assert count.tolist() == [0, 0, 0] and deg.tolist() == [0, 0, 0]
        count, deg = f(0, s[:0], d[:0])
        assert count.size == 0 and deg.size == 0
    assert tc_ref.summary(*tc_ref.triangles(5, s, d)) == dict(
        n_triangles=1, simple_edges=4, wedges=5, n_in_triangle=3, max_count=1, max_count_id=0)
    assert tc_ref.summary(np.zeros(0, np.int64), np.zeros(0, np.int64)) == dict(
        n_triangles=0, simple_edges=0, wedges=0, n_in_triangle=0, max_count=0, max_count_id=-1)
    # K6: every vertex in C(5, 2) triangles; a regular graph, the id alone orients it
    iu, ju = np.triu_indices(6, 1)
    for f in (tc_ref.triangles, tc_ref.triangles_oriented):
        assert f(6, iu, ju)[0].tolist() == [10] * 6
