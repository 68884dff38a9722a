"""Motif finding without a GPU: the C-ABI boundary of lpa_motif, the pattern parser and its
refusals (each before any device work), the planner's order, and the two CPU references of
tests/motif_ref.py against each other."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import graphframes_amd as gfa
from graphframes_amd import _lib

import motif_ref


def test_abi_version_has_motif():
    assert _lib.load().lpa_abi_version() >= 19


def test_motif_symbols_exported():
    lib = _lib.load()
    names = ["lpa_motif", "lpa_motif_rows", "lpa_motif_vertex_column", "lpa_motif_edge_column",
             "lpa_motif_result_destroy"]
    for name in names:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES or name in _lib.WIDE_SIGNATURES, name
    assert ctypes.sizeof(_lib.LpaMotifTerm) == 16
    assert ctypes.sizeof(_lib.LpaMotifSummary) == 8 * (7 + 16)


def test_null_handle_and_null_result():
    lib = _lib.load()
    term = (_lib.LpaMotifTerm * 1)(_lib.LpaMotifTerm(0, 1, 0, 0))
    res = ctypes.c_void_p()
    assert lib.lpa_motif(None, 2, None, term, 1, 0, 0, ctypes.byref(res), None) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()
    assert not res
    lib.lpa_motif_result_destroy(None)   # no-op
    assert lib.lpa_motif_rows(None) == 0
    assert lib.lpa_motif_vertex_column(None, 0, None) == _lib.LPA_EINVAL
    assert lib.lpa_motif_edge_column(None, 0, None) == _lib.LPA_EINVAL


# ---- parser ----
@pytest.mark.parametrize("term", ["(a)-[e]->(b)", "(a)-[]->(b)", "()-[e]->(b)", "(a)-[e]->()", "()-[e]->()",
                                  "(a)-[e]->(a)", "(x_1)-[E9]->(Y)"])
def test_positive_term_round_trips(term):
    p = gfa.parse_motif(term)
    assert len(p.terms) == 1 and str(p.terms[0]) == term and not p.terms[0].negated


def test_negated_and_lone_round_trip():
    p = gfa.parse_motif("(a)-[e]->(b);!(b)-[]->(a);(a)")
    assert [str(t) for t in p.terms] == ["(a)-[e]->(b)", "!(b)-[]->(a)"]
    assert p.terms[1].negated and p.lone == ("a",)
    assert p.names == (("a", "v"), ("e", "e"), ("b", "v"))


def test_whitespace_and_repeated_names():
    p = gfa.parse_motif("  (a) - [e] -> (b) ;\n\t(b)-[ e2 ]->(a)  ")
    q = gfa.parse_motif("(a)-[e]->(b);(b)-[e2]->(a)")
    assert p == q
    assert p.n_vars == 2 and p.var_names == ("a", "b")
    assert (p.terms[0].src_var, p.terms[0].dst_var) == (0, 1)
    assert (p.terms[1].src_var, p.terms[1].dst_var) == (1, 0)
    assert p.names == (("a", "v"), ("e", "e"), ("b", "v"), ("e2", "e"))


def test_anonymous_elements_are_fresh_variables():
    p = gfa.parse_motif("(a)-[]->(); (a)-[]->(); ()-[]->(a)")
    assert p.n_vars == 4 and p.var_names == ("a", None, None, None)
    assert [(t.src_var, t.dst_var) for t in p.terms] == [(0, 1), (0, 2), (3, 0)]
    assert all(t.edge is None for t in p.terms)
    assert p.names == (("a", "v"),)


def test_first_appearance_order_of_names():
    p = gfa.parse_motif("(b)-[x]->(c); (a)-[]->(b); !(c)-[]->(a)")
    assert p.names == (("b", "v"), ("x", "e"), ("c", "v"), ("a", "v"))


NINE = "; ".join(f"(a)-[]->(b{i})" for i in range(9))
NINE_NEG = "(a)-[]->(b); " + "; ".join("!(b)-[]->(a)" for _ in range(9))
REFUSED = [
    ("", "empty"),
    (" ;", "does not parse"),
    ("(a)-[e]->(b);", "does not parse"),
    ("(a)->(b)", r"'\(a\)->\(b\)' does not parse"),
    ("(a)-[e]-(b)", "does not parse"),
    ("(a b)-[e]->(c)x", "does not parse"),
    ("()", r"'\(\)' does not parse"),
    ("!(a)", "does not parse"),
    ("(a)-[a]->(b)", r"'\(a\)-\[a\]->\(b\)'.*both for a vertex and for an edge"),
    ("(a)-[e]->(b); (e)-[]->(a)", "both for a vertex and for an edge"),
    ("(a)-[e]->(b); (b)-[e]->(c)", r"'\(b\)-\[e\]->\(c\)'.*already used"),
    ("(a)-[]->(b); !(b)-[e]->(a)", r"'!\(b\)-\[e\]->\(a\)'.*negated term cannot name its edge"),
    ("(a)-[]->(b); !(b)-[]->()", r"'!\(b\)-\[\]->\(\)'.*anonymous vertex"),
    ("(a)-[]->(b); !()-[]->(a)", "anonymous vertex"),
    ("(a)-[]->(b); !(b)-[]->(c)", r"'!\(b\)-\[\]->\(c\)'.*no positive term binds the vertex 'c'"),
    ("!(a)-[]->(b)", "no positive term binds"),
    ("(a)-[]->(b); (c)-[]->(d)", r"'\(c\)-\[\]->\(d\)' is not connected"),
    ("(a)-[]->(b); (c)-[]->(d); (d)-[]->(e)", "not connected"),
    ("(a)-[]->(b); (c)", r"lone term '\(c\)'"),
    ("(a); (b)", "lone term"),
    ("()-[]->()", "names nothing"),
    ("()-[]->(); ()-[]->()", "names nothing|not connected"),
    (NINE, "9 positive"),
    (NINE_NEG, "9 negated"),
]


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_gpu_frame(monkeypatch):
    """A GraphFrame whose handle must not be asked for."""
    gf = gfa.GraphFrame(pd.DataFrame({"id": [0, 1, 2]}), pd.DataFrame({"src": [0, 1], "dst": [1, 2]}))

    def boom():
        raise _NoDevice("the pattern reached the device")

    monkeypatch.setattr(gf, "_gpu_graph", boom)
    return gf


@pytest.mark.parametrize("pattern,match", REFUSED, ids=[f"r{i}" for i in range(len(REFUSED))])
def test_refusals_before_device_work(no_gpu_frame, pattern, match):
    with pytest.raises(ValueError, match=match):
        gfa.parse_motif(pattern)
    with pytest.raises(ValueError, match=match):
        no_gpu_frame.find(pattern)
    with pytest.raises(ValueError, match=match):
        no_gpu_frame.motifCount(pattern)
    # the function forms refuse before they build a handle (which needs a device)
    v, e = no_gpu_frame.vertices, no_gpu_frame.edges
    with pytest.raises(ValueError, match=match):
        gfa.find(v, e, pattern)
    with pytest.raises(ValueError, match=match):
        gfa.motif_count(v, e, pattern)


def test_a_good_pattern_does_reach_the_device(no_gpu_frame):
    with pytest.raises(_NoDevice):
        no_gpu_frame.find("(a)-[]->(b)")
    with pytest.raises(TypeError):
        no_gpu_frame.find(7)
    with pytest.raises(ValueError, match="maxRows"):
        no_gpu_frame.find("(a)-[]->(b)", maxRows=0)


def test_lone_vertex_is_host_only(no_gpu_frame):
    out = no_gpu_frame.find("(a)")
    assert list(out.columns) == [("a", "id")] and out["a"]["id"].tolist() == [0, 1, 2]
    assert out.attrs == {"rows": 3, "plan": []}
    assert no_gpu_frame.motifCount("(a)") == 3
    # a lone term whose name an edge term binds is a no-op
    assert gfa.plan_motif(gfa.parse_motif("(a); (a)-[]->(b)")) == [0]


# ---- planner ----
PLAN_PATTERNS = motif_ref.PATTERNS + [
    "()-[]->(x); (a)-[]->(b); (b)-[]->(x); (a)-[]->(x)",
    "(a)-[]->(b); (b)-[]->(c); (c)-[]->(d); (a)-[]->(c); !(d)-[]->(a); !(b)-[]->(a); (d)-[]->(e)",
    "(a)-[]->(); (a)-[]->(b); (b)-[]->(a); !(a)-[]->(a)",
]


@pytest.mark.parametrize("pattern", PLAN_PATTERNS)
def test_plan_order(pattern):
    p = gfa.parse_motif(pattern)
    plan = gfa.plan_motif(p)
    assert sorted(plan) == list(range(len(p.terms)))
    named = lambda t: len({v for v in (t.src_var, t.dst_var) if p.var_names[v] is not None})  # noqa: E731
    pos = [i for i in plan if not p.terms[i].negated]
    assert named(p.terms[pos[0]]) == max(named(t) for t in p.terms if not t.negated)
    bound, left = set(), set(range(len(p.terms)))
    for k, i in enumerate(plan):
        t = p.terms[i]
        ends = {t.src_var, t.dst_var}
        left.discard(i)
        if t.negated:
            assert ends <= bound
            continue
        if k > 0:
            assert ends & bound, f"term {i} shares nothing with the earlier ones"
            if not ends <= bound:   # an extend: no close was available
                assert not any(not p.terms[j].negated and {p.terms[j].src_var, p.terms[j].dst_var} <= bound
                               for j in left)
        bound |= ends
        # every negation that is bound by now has run or runs next, before any positive term
        ready = [j for j in left if p.terms[j].negated and {p.terms[j].src_var, p.terms[j].dst_var} <= bound]
        assert plan[k + 1:k + 1 + len(ready)] == sorted(ready)


def test_plan_examples():
    plan = lambda s: gfa.plan_motif(gfa.parse_motif(s))  # noqa: E731
    assert plan("()-[]->(x); (a)-[]->(b); (b)-[]->(x); (a)-[]->(x)") == [1, 2, 3, 0]
    assert plan("(a)-[]->(b); (b)-[]->(c); !(b)-[]->(a); (c)-[]->(a)") == [0, 2, 1, 3]
    assert plan("(a)-[]->(b); (a)-[]->(c); (b)-[]->(a)") == [0, 2, 1]


# ---- the references against each other ----
@pytest.mark.parametrize("pattern", motif_ref.PATTERNS)
def test_literal_equals_merge_chain(pattern):
    sp = motif_ref.spec(gfa.parse_motif(pattern))
    total = 0
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        V, m = 6, 14
        s, d = rng.integers(0, V, m), rng.integers(0, V, m)
        s[:2], d[:2] = [1, 1], [1, 4]          # a self-loop for sure
        s[2:5], d[2:5] = s[5], d[5]            # and a triple edge
        d[13] = V                              # and a dangling one
        a = motif_ref.literal(V, s, d, *sp)
        b = motif_ref.merge_chain(V, s, d, *sp)
        assert a == b, (pattern, seed)
        total += len(a)
    assert total > 0
