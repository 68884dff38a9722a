"""Message aggregation without a GPU: the C-ABI boundary of lpa_aggregate_messages (its program
validation runs before the handle is looked at), the expression layer and compile_message, every
refusal of GraphFrame.aggregateMessages (each before a handle exists), the column names, and the
two CPU references of tests/am_ref.py against each other."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import graphframes_amd as gfa
from graphframes_amd import AggregateMessages as AM
from graphframes_amd import _lib
from graphframes_amd import graphframe as gf_mod

import am_ref
from graphs import random_multigraph

OP = {name: i for i, name in enumerate(_lib.AM_OPCODES)}


def program(ops, consts=()):
    p = _lib.LpaAmProgram()
    p.n_ops, p.n_consts = len(ops), len(consts)
    for i, (op, arg) in enumerate(ops):
        p.ops[i] = (OP[op] if isinstance(op, str) else op) | (arg << 16)
    for i, c in enumerate(consts):
        p.consts[i] = c
    return p


def call(to_src, to_dst, n_vcols=0, n_ecols=0, handle=None):
    lib = _lib.load()
    return lib.lpa_aggregate_messages(handle, None if to_src is None else ctypes.byref(to_src),
                                      None if to_dst is None else ctypes.byref(to_dst), None, n_vcols, None, n_ecols,
                                      None, None, None, None, None)


# ---- the C ABI ----
def test_abi_version_has_aggregate_messages():
    assert _lib.load().lpa_abi_version() >= 20


def test_symbol_and_struct_sizes():
    assert hasattr(_lib.load(), "lpa_aggregate_messages")
    assert "lpa_aggregate_messages" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.LpaAmProgram) == 392 == 8 + 4 * 64 + 8 * 16
    assert ctypes.sizeof(_lib.LpaAmSummary) == 72
    assert len(_lib.AM_OPCODES) == 21


def test_null_handle():
    assert call(None, program([("const", 0)], [1.0])) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error()


def test_both_programs_null():
    assert call(None, None) == _lib.LPA_EINVAL
    assert "both programs are null" in _lib.last_error()


MALFORMED = [
    ([], (), 0, 0, "has 0 ops"),
    ([(99, 0)], (), 0, 0, "unknown opcode 99"),
    ([("add", 0)], (), 0, 0, "underflows the stack"),
    ([("const", 0), ("when_else", 0)], (1.0,), 0, 0, "underflows the stack"),
    ([("const", 0)] * 9 + [("add", 0)] * 8, (1.0,), 0, 0, "overflows the stack of 8"),
    ([("const", 1)], (1.0,), 0, 0, "reads constant 1 of 1"),
    ([("src", 2)], (), 2, 0, "reads vertex column 2 of 2"),
    ([("dst", 0)], (), 0, 3, "reads vertex column 0 of 0"),
    ([("edge", 1)], (), 4, 1, "reads edge column 1 of 1"),
    ([("const", 0), ("const", 0)], (1.0,), 0, 0, "leaves 2 values"),
]


@pytest.mark.parametrize("ops,consts,nv,ne,text", MALFORMED)
def test_malformed_program(ops, consts, nv, ne, text):
    good = program([("const", 0)], [1.0])
    for to_src, to_dst, name in ((program(ops, consts), None, "to_src"), (good, program(ops, consts), "to_dst")):
        assert call(to_src, to_dst, nv, ne) == _lib.LPA_EINVAL
        assert text in _lib.last_error() and name in _lib.last_error(), _lib.last_error()


def test_counts_out_of_range():
    good = program([("const", 0)], [1.0])
    assert call(good, None, 9, 0) == _lib.LPA_EINVAL and "n_vcols" in _lib.last_error()
    bad = program([("const", 0)], [1.0])
    bad.n_consts = 17
    assert call(bad, None) == _lib.LPA_EINVAL and "17 constants" in _lib.last_error()
    bad.n_consts, bad.n_ops = 1, 65
    assert call(bad, None) == _lib.LPA_EINVAL and "65 ops" in _lib.last_error()


def test_deepest_legal_program_reaches_the_handle_check():
    p = program([("const", 0)] * 8 + [("add", 0)] * 7, (1.0,))
    assert call(p, p) == _lib.LPA_EINVAL and "null handle" in _lib.last_error()
    p = program([("const", 0), ("src", 7), ("edge", 7), ("when_else", 0)], (0.0,))
    assert call(None, p, 8, 8) == _lib.LPA_EINVAL and "null handle" in _lib.last_error()


# ---- the expression layer ----
X, Y, W = AM.src["x"], AM.dst["y"], AM.edge["w"]
ROUND_TRIPS = [
    ("lit", AM.lit(2.5), ["const"]),
    ("src", X, ["src"]),
    ("dst", Y, ["dst"]),
    ("edge", W, ["edge"]),
    ("add", X + Y, ["src", "dst", "add"]),
    ("radd", 1 + X, ["const", "src", "add"]),
    ("sub", X - W, ["src", "edge", "sub"]),
    ("rsub", 1.5 - X, ["const", "src", "sub"]),
    ("mul", X * 3, ["src", "const", "mul"]),
    ("rmul", 3 * X, ["const", "src", "mul"]),
    ("div", X / Y, ["src", "dst", "div"]),
    ("rdiv", 1 / X, ["const", "src", "div"]),
    ("neg", -X, ["src", "neg"]),
    ("abs", abs(X - Y), ["src", "dst", "sub", "abs"]),
    ("eq", X == Y, ["src", "dst", "eq"]),
    ("ne", X != 0, ["src", "const", "ne"]),
    ("lt", X < Y, ["src", "dst", "lt"]),
    ("le", X <= Y, ["src", "dst", "le"]),
    ("gt", X > Y, ["src", "dst", "gt"]),
    ("ge", X >= Y, ["src", "dst", "ge"]),
    ("and", (X < Y) & (W > 0), ["src", "dst", "lt", "edge", "const", "gt", "and"]),
    ("or", (X < Y) | (W > 0), ["src", "dst", "lt", "edge", "const", "gt", "or"]),
    ("not", ~(X < Y), ["src", "dst", "lt", "not"]),
    ("when", AM.when(X < Y, W), ["src", "dst", "lt", "edge", "when"]),
    ("when_else", AM.when(X < Y, W).otherwise(-1), ["src", "dst", "lt", "edge", "const", "when_else"]),
    ("bool_lit", AM.when(AM.lit(True) & (X > 1), 2), ["const", "src", "const", "gt", "and", "const", "when"]),
]


@pytest.mark.parametrize("name,expr,names", ROUND_TRIPS, ids=[r[0] for r in ROUND_TRIPS])
def test_compile_round_trip(name, expr, names):
    c = gfa.compile_message(expr)
    assert isinstance(c, gfa.CompiledMessage)
    assert [_lib.AM_OPCODES[op] for op, _ in c.ops] == names
    assert c.decode().same(expr) and str(c.decode()) == str(expr)
    assert all(0 <= arg < 2 ** 16 for _, arg in c.ops)
    assert set(c.vertex_columns) <= {"x", "y"} and set(c.edge_columns) <= {"w"}


def test_compile_tables():
    c = gfa.compile_message(X * 2 + AM.src["y"] * 2 - W * 0.5 + AM.edge["k"] * -0.0 + 0.0)
    assert c.consts == (2.0, 0.5, -0.0, 0.0) and np.signbit(c.consts[2]) and not np.signbit(c.consts[3])
    assert c.vertex_columns == ("x", "y") and c.edge_columns == ("w", "k")
    assert c.depth == 3   # the running sum, a column, its factor
    d =gfa.compile_message(AM.dst["z"] + AM.src["y"], c.vertex_columns, c.edge_columns)
    assert d.vertex_columns == ("x", "y", "z") and d.edge_columns == ("w", "k")
    assert d.ops == ((1 + 1, 2), (1, 1), (4, 0))   # dst z = column 2, src y = column 1, add
    assert gfa.compile_message(5).ops == ((0, 0),) and gfa.compile_message(5).consts == (5.0,)
    right_deep = X + (X + (X + (X + (X + (X + (X + X))))))
    assert gfa.compile_message(right_deep).depth == gf_mod.AM_MAX_STACK


def test_limits_are_named_constants():
    assert (gf_mod.AM_MAX_OPS, gf_mod.AM_MAX_STACK, gf_mod.AM_MAX_CONSTS) == (64, 8, 16)
    assert (gf_mod.AM_MAX_VERTEX_COLUMNS, gf_mod.AM_MAX_EDGE_COLUMNS) == (8, 8)


def chain(n):
    e = X
    for _ in range(n):
        e = e + X
    return e


def deep(n):
    e = X
    for _ in range(n):
        e = X + e
    return e


def many_consts(n):
    e = X
    for i in range(n):
        e = e + (i + 0.5)
    return e


def many_columns(kind, n):
    e = AM.lit(0)
    for i in range(n):
        e = e + getattr(AM, kind)[f"c{i}"]
    return e


def test_limits_at_and_above():
    assert len(gfa.compile_message(chain(31)).ops) == 63
    assert len(gfa.compile_message(-chain(31)).ops) == 64
    with pytest.raises(ValueError, match="65 ops, more than AM_MAX_OPS"):
        gfa.compile_message(-(-chain(31)))
    assert gfa.compile_message(deep(7)).depth == 8
    with pytest.raises(ValueError, match="stack of 9 values, more than AM_MAX_STACK"):
        gfa.compile_message(deep(8))
    assert len(gfa.compile_message(many_consts(16)).consts) == 16
    with pytest.raises(ValueError, match="17 constants, more than AM_MAX_CONSTS"):
        gfa.compile_message(many_consts(17))
    assert len(gfa.compile_message(many_columns("src", 8)).vertex_columns) == 8
    with pytest.raises(ValueError, match="9 vertex columns .* more than AM_MAX_VERTEX_COLUMNS"):
        gfa.compile_message(many_columns("dst", 9))
    with pytest.raises(ValueError, match="9 edge columns .* more than AM_MAX_EDGE_COLUMNS"):
        gfa.compile_message(many_columns("edge", 9))


def test_expression_misuse():
    with pytest.raises(ValueError, match="takes comparison results"):
        X & (Y > 0)
    with pytest.raises(ValueError, match="takes comparison results"):
        ~X
    with pytest.raises(ValueError, match="condition"):
        AM.when(X, 1)
    with pytest.raises(ValueError, match="otherwise"):
        (X + 1).otherwise(2)
    with pytest.raises(ValueError, match="otherwise"):
        AM.when(X > 0, 1).otherwise(2).otherwise(3)
    with pytest.raises(TypeError, match="truth value"):
        bool(X > 0)
    with pytest.raises(TypeError, match="operand"):
        X + "1"
    with pytest.raises(ValueError, match="not finite"):
        X + float("inf")
    with pytest.raises(ValueError, match="2\\^53"):
        X + (2 ** 53 + 1)
    with pytest.raises(ValueError, match="aggregate"):
        X + AM.sum(AM.msg)


# ---- refusals of aggregateMessages, before a handle exists ----
@pytest.fixture()
def frames(monkeypatch):
    """Frames for the refusals; building a GPU handle fails the test."""
    def no_handle(self):
        raise AssertionError("a handle was created before the host checks were done")

    monkeypatch.setattr(gfa.GraphFrame, "_gpu_graph", no_handle)
    v = pd.DataFrame({"id": [0, 1, 2], "x": [1.0, 2.0, 3.0], "name": ["a", "b", "c"], "n": [1.0, np.nan, 2.0],
                      "inf": [1.0, -np.inf, 2.0], "big": [1, 2 ** 53 + 1, 3], "ok53": [2 ** 53, -2 ** 53, 0],
                      "ubig": np.array([1, 2 ** 63, 3], dtype=np.uint64), "flag": [True, False, True],
                      "obj": pd.Series([1.0, None, 2.0], dtype=object), "none": [1.0, None, 2.0], "na": pd.array([1, None, 3], dtype="Int64"),
                      "z": [1 + 1j, 2, 3]})
    e = pd.DataFrame({"src": [0, 1], "dst": [1, 2], "w": [0.5, 1.5], "kind": ["p", "q"], "n": [np.nan, 1.0]})
    return v, e


REFUSED = [
    (lambda: dict(aggCol=AM.sum(AM.msg)), "Either `sendToSrc`, `sendToDst`, or both have to be provided"),
    (lambda: dict(aggCol=AM.msg, sendToDst=X), "aggCol must be AM.sum"),
    (lambda: dict(aggCol="sum(MSG)", sendToDst=X), "aggCol must be AM.sum"),
    (lambda: dict(aggCol=AM.sum(AM.msg + 1), sendToDst=X), "exactly AM.msg"),
    (lambda: dict(aggCol=AM.sum(3), sendToDst=X), "exactly AM.msg"),
    (lambda: dict(aggCol=AM.max(AM.src["x"]), sendToDst=X), r"reads AM.src\['x'\]"),
    (lambda: dict(aggCol=AM.min(AM.msg * AM.edge["w"]), sendToDst=X), r"reads AM.edge\['w'\]"),
    (lambda: dict(aggCol=AM.avg(AM.dst["x"] + AM.msg), sendToDst=X), r"reads AM.dst\['x'\]"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.msg + 1), "AM.msg appears inside the message"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToSrc=AM.when(X > 0, AM.msg)), "AM.msg appears inside the message"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.src["nope"]), "vertex frame has no column 'nope'"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToSrc=AM.dst["w"]), "vertex frame has no column 'w'"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.edge["x"]), "edge frame has no column 'x'"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.src["name"]), "'name' of the vertex frame is not numeric or bool"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.edge["kind"]), "'kind' of the edge frame is not numeric or bool"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.src["obj"]), "'obj' of the vertex frame is not numeric or bool"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.src["z"]), "'z' of the vertex frame is not numeric or bool"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.src["n"]), "'n' of the vertex frame holds NaN, None or an inf"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.edge["n"]), "'n' of the edge frame holds NaN, None or an inf"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.dst["inf"]), "'inf' of the vertex frame holds NaN, None or an inf"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.dst["none"]), "'none' of the vertex frame holds NaN, None or an inf"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.dst["na"]), "'na' of the vertex frame holds NaN, None or an inf"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.src["big"]), r"'big' of the vertex frame holds an integer beyond \+-2\^53"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=AM.src["ubig"]), r"'ubig' of the vertex frame holds an integer beyond"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToDst=chain(64)), "more than AM_MAX_OPS"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToSrc=deep(8)), "more than AM_MAX_STACK"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToSrc=many_consts(17)), "more than AM_MAX_CONSTS"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToSrc=many_columns("src", 5), sendToDst=many_columns("dst", 9)),
     "more than AM_MAX_VERTEX_COLUMNS"),
    (lambda: dict(aggCol=AM.sum(AM.msg), sendToSrc=many_columns("edge", 5),
                  sendToDst=AM.edge["c0"] + AM.edge["c1"] + AM.edge["d0"] + AM.edge["d1"] + AM.edge["d2"] + AM.edge["d3"]),
     "9 edge columns .* more than AM_MAX_EDGE_COLUMNS"),
]


@pytest.mark.parametrize("make,text", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refused_before_any_handle(frames, make, text):
    v, e = frames
    with pytest.raises(ValueError, match=text):
        gfa.GraphFrame(v, e).aggregateMessages(**make())
    with pytest.raises(ValueError, match=text):
        gfa.aggregate_messages(v, e, **make())


def test_prepare_accepts(frames):
    """What is NOT refused: a bare comparison as the message, a bool column, integers of exactly
    +-2^53, the id column, a numeric constant; the directions share one column table."""
    v, e = frames
    agg, to_src, to_dst, vcols, ecols = gf_mod._am_prepare(v, e, AM.sum(AM.msg), AM.src["x"] > AM.dst["x"], None)
    assert [_lib.AM_OPCODES[op] for op, _ in to_src.ops] == ["src", "dst", "gt"] and to_dst is None
    _, to_src, to_dst, vcols, ecols = gf_mod._am_prepare(
        v, e, AM.count(AM.msg), AM.src["flag"] + AM.src["ok53"] + AM.edge["w"], AM.dst["id"] * AM.src["flag"] + 1)
    assert to_src.vertex_columns == ("flag", "ok53") and to_dst.vertex_columns == ("flag", "ok53", "id")
    assert to_dst.edge_columns == ("w",) and len(vcols) == 3 and len(ecols) == 1
    assert vcols[0].tolist() == [1.0, 0.0, 1.0] and vcols[1].tolist() == [2.0 ** 53, -2.0 ** 53, 0.0]
    assert all(c.dtype == np.float64 for c in vcols + ecols)
    _, to_src, _, vcols, ecols = gf_mod._am_prepare(v, e, AM.max(AM.msg), 1, None)
    assert to_src.ops == ((0, 0),) and vcols == [] and ecols == []


def test_column_names():
    for kind in ("sum", "min", "max", "avg", "count"):
        a = getattr(AM, kind)(AM.msg)
        assert a.name == f"{kind}(MSG)" and a.alias("t").name == "t" and a.alias("t").kind == kind
    assert AM.mean(AM.msg).name == "avg(MSG)" and AM.mean(AM.msg).alias("m").kind == "avg"
    assert str(AM.msg) == "MSG"


# ---- the two references against each other ----
def _case(seed):
    V, s, d = random_multigraph(50, 400, seed)
    rng = np.random.default_rng(seed + 100)
    s[:20], d[:20] = rng.integers(0, V, 20), 0              # a hub
    d[20:30] = s[20:30]                                      # self-loops
    s[30:40], d[30:40] = s[40:50], d[40:50]                  # duplicates
    vcols = {"x": rng.integers(-3, 4, V).astype(np.float64), "y": rng.standard_normal(V),
             "c": rng.integers(0, 3, V).astype(np.float64)}
    ecols = {"w": rng.standard_normal(s.size), "k": rng.integers(0, 3, s.size).astype(np.float64)}
    return V, s, d, vcols, ecols


SX, DX, SY, DY, SC, DC = (AM.src["x"], AM.dst["x"], AM.src["y"], AM.dst["y"], AM.src["c"], AM.dst["c"])
EW, EK = AM.edge["w"], AM.edge["k"]
PAIRS = [
    (None, AM.lit(1)),
    (SX, None),
    (SY * EW, DY - EW),
    (AM.when(SC != DC, 1.0), AM.when(SC != DC, 1.0)),
    (SY / DX, EW / EK),                                                # zero divisors: null
    (AM.when(SY / DX > 0, EW), AM.when(SY / DX > 0, EW).otherwise(-EW)),   # a null condition
    (AM.when((SC == 0) & (DC > 0) | ~(EK >= 1), abs(SY)), -SX * 0),    # -0.0 messages
    (AM.when(EK == 7, 1.0), SX < DX),                                  # all null one way; a bare comparison
    ((SX / DX == 1) | (EK == 0), AM.when(EK > 0, SY / SX).otherwise(DY / SX)),   # null through | and both branches
]


@pytest.mark.parametrize("k", range(len(PAIRS)))
@pytest.mark.parametrize("seed", [1, 2])
def test_vectorised_reference_against_the_loop(seed, k):
    V, s, d, vcols, ecols = _case(seed)
    to_src, to_dst = PAIRS[k]
    a = am_ref.aggregate(V, s, d, to_src, to_dst, vcols, ecols)
    b = am_ref.aggregate_loop(V, s, d, to_src, to_dst, vcols, ecols)
    assert np.array_equal(a["count"], b["count"])
    for key in ("min", "max", "fsum"):
        assert am_ref.same_bits(a[key], b[key]), key
    indeg, outdeg = np.bincount(d, minlength=V), np.bincount(s, minlength=V)
    assert np.array_equal(a["rows"], (indeg if to_dst is not None else 0) + (outdeg if to_src is not None else 0))
    n_eval = s.size * ((to_src is not None) + (to_dst is not None))
    assert a["messages_to_src"] + a["messages_to_dst"] + a["nulls"] == n_eval == a["rows"].sum()
    assert a["count"].sum() == n_eval - a["nulls"]


def test_reference_drops_out_of_range_edges():
    s, d = np.array([0, 1, 5, -1, 2]), np.array([1, 2, 0, 1, 7])
    a = am_ref.aggregate(3, s, d, AM.lit(1), AM.lit(1))
    b = am_ref.aggregate_loop(3, s, d, AM.lit(1), AM.lit(1))
    assert a["count"].tolist() == b["count"].tolist() == [1, 2, 1] and a["edges"] == 2


def test_reference_null_rules_by_hand():
    """One edge 0 -> 1 with x = (2, 0): the rules of the issue, one at a time."""
    s, d, vc = np.array([0]), np.array([1]), {"x": np.array([2.0, 0.0])}
    sx, dx = AM.src["x"], AM.dst["x"]
    for expr, want in [(sx / dx, None), (sx / dx + 1, None), (AM.when(dx > 1, sx), None),
                       (AM.when(dx > 1, sx).otherwise(5), 5.0), (AM.when(sx / dx > 1, sx).otherwise(7), 7.0),
                       (AM.when(sx / dx > 1, sx), None), ((sx / dx > 1) | (sx > 1), None),
                       ((sx / dx > 1) & (sx < 1), None), (~(sx / dx > 1), None),
                       (AM.when(sx > 1, sx / dx).otherwise(3), None), (AM.when(sx < 1, sx / dx).otherwise(3), 3.0),
                       (sx > dx, 1.0), (sx < dx, 0.0), (-dx, -0.0), (abs(-sx), 2.0), (dx / sx, 0.0)]:
        a = am_ref.aggregate(2, s, d, None, expr, vc)
        b = am_ref.aggregate_loop(2, s, d, None, expr, vc)
        assert a["count"].tolist() == b["count"].tolist() == [0, 0 if want is None else 1], str(expr)
        if want is not None:
            assert am_ref.same_bits(a["min"][1:], [want]) and am_ref.same_bits(b["max"][1:], [want]), str(expr)
