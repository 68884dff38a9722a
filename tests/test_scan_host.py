"""SCAN structural clustering, the part that needs no GPU: the C-ABI boundary of lpa_scan, the
exported names, the argument checks of Graph.scan, GraphFrame.scan and the function form (they
run before any device work), and the CPU restatement tests/scan_ref.py on the closed forms of
the specification (tests/scan_cases.py)."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import graphframes_amd as gfa
import scan_cases
import scan_ref
from graphframes_amd import _lib


def test_null_handle_is_einval():
    lib = _lib.load()
    assert lib.lpa_scan(None, 0.7, 2, None, None, None, None, 0, None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_abi_version_has_scan():
    assert _lib.load().lpa_abi_version() >= 23


def test_struct_layout():
    s = _lib.LpaScanSummary(*range(1, 11))
    assert tuple(s.to_dict()) == scan_ref.SUMMARY_KEYS
    assert list(s.to_dict().values()) == list(range(1, 11))
    assert ctypes.sizeof(_lib.LpaScanSummary) == 80


def test_exported():
    for name in ("scan", "structural_similarity"):
        assert name in gfa.__all__ and callable(getattr(gfa, name))
    assert callable(gfa.GraphFrame.scan) and callable(gfa.GraphFrame.structuralSimilarity)
    assert callable(gfa.Graph.scan)
    assert "lpa_scan" in _lib.SIGNATURES


# ---- argument checks: none of them reaches the device ----
@pytest.fixture()
def gf():
    v = pd.DataFrame({"id": np.array([30, 10, 20], np.int64), "name": ["c", "a", "b"]})
    e = pd.DataFrame({"src": np.array([10, 20], np.int64), "dst": np.array([20, 30], np.int64)})
    f = gfa.GraphFrame(v, e)
    yield f
    assert f._graph is None   # no handle was ever built


@pytest.mark.parametrize("bad", ["0.5", None, True, np.bool_(False), [0.5], 1j])
def test_epsilon_must_be_a_number(gf, bad):
    with pytest.raises(TypeError, match="epsilon must be a real number"):
        gf.scan(bad, 2)
    with pytest.raises(TypeError, match="epsilon must be a real number"):
        gfa.scan(gf.vertices, gf.edges, epsilon=bad)
    with pytest.raises(TypeError, match="eps must be a real number"):
        gfa.Graph.scan(None, bad, 2)


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), np.float64("nan")])
def test_epsilon_must_belong_to_the_interval(gf, bad):
    with pytest.raises(ValueError, match=r"epsilon must belong to \(0, 1\], but got"):
        gf.scan(bad, 2)
    with pytest.raises(ValueError, match=r"epsilon must belong to \(0, 1\]"):
        gfa.scan(gf.vertices, gf.edges, bad, 2)
    with pytest.raises(ValueError, match=r"eps must belong to \(0, 1\]"):
        gfa.Graph.scan(None, bad, 2)


@pytest.mark.parametrize("bad", [2.0, "2", None, True, np.float64(3), np.bool_(True), [2]])
def test_mu_must_be_an_int(gf, bad):
    with pytest.raises(TypeError, match="mu must be an int"):
        gf.scan(0.7, bad)
    with pytest.raises(TypeError, match="mu must be an int"):
        gfa.scan(gf.vertices, gf.edges, 0.7, bad)
    with pytest.raises(TypeError, match="mu must be an int"):
        gfa.Graph.scan(None, 0.7, mu=bad)


@pytest.mark.parametrize("bad", [0, -1, np.int64(-5)])
def test_mu_must_be_positive(gf, bad):
    with pytest.raises(ValueError, match=f"mu must be at least 1, but got {bad}"):
        gf.scan(0.7, bad)
    with pytest.raises(ValueError, match="mu must be at least 1"):
        gfa.scan(gf.vertices, gf.edges, mu=bad)
    with pytest.raises(ValueError, match="mu must be at least 1"):
        gfa.Graph.scan(None, 0.7, bad)


def test_accepted_extremes(gf):
    """1.0 and the smallest positive double are legal eps; numpy scalars are accepted."""
    from graphframes_amd.graph import _check_scan

    assert _check_scan(1, 1) == (1.0, 1)
    assert _check_scan(np.float32(0.5), np.int32(3)) == (0.5, 3)
    assert _check_scan(5e-324, 2 ** 40) == (5e-324, 2 ** 31 - 1)


# ---- the reference on the closed forms ----
@pytest.mark.parametrize("name", list(scan_cases.CLOSED))
def test_reference_closed_forms(name):
    V, edges, eps, mu, labels, letters = scan_cases.CLOSED[name]
    s, d = scan_cases.arrays(edges)
    label, role, nsim, summ = scan_ref.scan(scan_ref.prepare(V, s, d), eps, mu)
    assert label.tolist() == labels
    assert role.tolist() == scan_cases.roles(letters).tolist()
    assert label.dtype == np.int32 and role.dtype == np.uint8 and nsim.dtype == np.int32
    assert summ["n_cores"] == letters.count("c") and summ["n_borders"] == letters.count("b")
    assert summ["n_hubs"] == letters.count("h") and summ["n_outliers"] == letters.count("o")
    assert summ["n_clusters"] == len({l for l, x in zip(labels, letters) if x in "cb"})
    assert tuple(summ) == scan_ref.SUMMARY_KEYS


def test_reference_tie_is_exact():
    """sigma(0, 1) of the double star is exactly 0.5: similar at eps = 0.5, not one ulp above."""
    assert scan_ref.similar(0, 3, 3, 0.5)
    assert not scan_ref.similar(0, 3, 3, np.nextafter(0.5, 1))
    assert abs(2 / np.sqrt(4 * 2) - 0.7071) < 1e-4 and scan_ref.similar(0, 3, 1, 0.7)


def test_reference_rows_and_multigraph():
    """common per input row: both directions and duplicates agree, self-loops and rows with an
    end outside the vertex range get -1; the result is the simple graph's."""
    V, edges, eps, mu, labels, letters = scan_cases.CLOSED["bridged-0.75"]
    s, d = scan_cases.arrays(edges)
    p = scan_ref.prepare(V, s, d)
    assert p.common_rows.tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0]
    s2 = np.concatenate([s, d, [2, 4, 9, -1]]).astype(np.int32)
    d2 = np.concatenate([d, s, [2, 4, 0, 3]]).astype(np.int32)
    p2 = scan_ref.prepare(V, s2, d2)
    assert p2.common_rows.tolist() == p.common_rows.tolist() * 2 + [-1] * 4
    a, b = scan_ref.scan(p, eps, mu), scan_ref.scan(p2, eps, mu)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert a[3] == dict(simple_edges=9, triangles=2, similar_edges=6, n_clusters=2, n_cores=6, n_borders=0,
                        n_hubs=1, n_outliers=1, largest_cluster=3, largest_cluster_label=0)
