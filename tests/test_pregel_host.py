"""Pregel without a GPU: the C-ABI boundary of lpa_pregel (every count and program is validated
before the handle is looked at), the vertex-program compiler, every refusal of the Pregel builder
(each before a handle exists), and the two CPU references of tests/pregel_ref.py against each
other."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import graphframes_amd as gfa
from graphframes_amd import AggregateMessages as AM
from graphframes_amd import Pregel, _lib

import pregel_ref
from graphs import random_multigraph

AOP = {name: i for i, name in enumerate(_lib.AM_OPCODES)}
VOP = {name: i for i, name in enumerate(_lib.VP_OPCODES)}


def programs(struct, table, progs):
    """[(ops, consts)] as a C array of the struct."""
    arr = (struct * max(len(progs), 1))()
    for k, (ops, consts) in enumerate(progs):
        arr[k].n_ops, arr[k].n_consts = len(ops), len(consts)
        for i, (op, arg) in enumerate(ops):
            arr[k].ops[i] = (table[op] if isinstance(op, str) else op) | (arg << 16)
        for i, c in enumerate(consts):
            arr[k].consts[i] = c
    return arr


ONE = ([("const", 0)], (1.0,))


def call(to_src=(), to_dst=(ONE,), init=(ONE,), update=(ONE,), max_iter=1, agg=0, n_vcols=0, n_ecols=0, n_pcols=None,
         n_to_src=None, n_to_dst=None):
    lib = _lib.load()
    return lib.lpa_pregel(None, max_iter, agg, programs(_lib.LpaAmProgram, AOP, to_src),
                          len(to_src) if n_to_src is None else n_to_src, programs(_lib.LpaAmProgram, AOP, to_dst),
                          len(to_dst) if n_to_dst is None else n_to_dst, programs(_lib.LpaVpProgram, VOP, init),
                          programs(_lib.LpaVpProgram, VOP, update), len(init) if n_pcols is None else n_pcols, None,
                          n_vcols, None, n_ecols, None, None)


# ---- the C ABI ----
def test_abi_version_has_pregel():
    assert _lib.load().lpa_abi_version() >= 21


def test_symbol_struct_sizes_and_tables():
    assert hasattr(_lib.load(), "lpa_pregel") and "lpa_pregel" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.LpaVpProgram) == 392 == ctypes.sizeof(_lib.LpaAmProgram)
    assert ctypes.sizeof(_lib.LpaPregelSummary) == 96
    assert len(_lib.VP_OPCODES) == 22 and len(set(_lib.VP_OPCODES)) == 22
    assert _lib.VP_OPCODES[:3] == ("const", "col", "msg") and _lib.VP_OPCODES[-2:] == ("coalesce", "isnull")
    assert len(_lib.AM_OPCODES) == 21 and "coalesce" not in _lib.AM_OPCODES
    assert _lib.PG_AGGREGATES == ("sum", "min", "max", "avg", "count")
    assert (_lib.LPA_PG_MAX_COLUMNS, _lib.LPA_PG_MAX_MESSAGES) == (4, 4)


def test_header_states_the_values():
    import os
    import re

    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lpa.h")).read()
    for i, name in enumerate(_lib.VP_OPCODES):
        assert re.search(rf"LPA_VP_{name.upper()} = {i}\b", txt), name
    for i, name in enumerate(_lib.PG_AGGREGATES):
        assert re.search(rf"LPA_PG_{name.upper()} = {i}\b", txt), name
    assert "LPA_VP_NOPS = 22" in txt and "LPA_AM_NOPS = 21" in txt


def test_a_good_call_reaches_the_handle_check():
    assert call() == _lib.LPA_EINVAL and "null handle" in _lib.last_error()


@pytest.mark.parametrize("kwargs,text", [
    (dict(max_iter=0), "max_iter"),
    (dict(max_iter=-3), "max_iter"),
    (dict(agg=5), "aggregate 5"),
    (dict(agg=-1), "aggregate -1"),
    (dict(n_pcols=0), "n_pcols"),
    (dict(n_pcols=5), "n_pcols"),
    (dict(to_dst=()), "no message program"),
    (dict(n_to_dst=5), "n_to_dst"),
    (dict(n_to_src=-1), "n_to_src"),
    (dict(n_vcols=8), "n_vcols"),
    (dict(n_vcols=-1), "n_vcols"),
    (dict(n_ecols=9), "n_ecols"),
])
def test_counts_out_of_range(kwargs, text):
    assert call(**kwargs) == _lib.LPA_EINVAL
    assert text in _lib.last_error(), _lib.last_error()


MALFORMED_VERTEX = [
    ([], (), "has 0 ops"),
    ([(22, 0)], (), "unknown opcode 22"),
    ([(99, 0)], (), "unknown opcode 99"),
    ([("add", 0)], (), "underflows the stack"),
    ([("const", 0), ("coalesce", 0)], (1.0,), "underflows the stack"),
    ([("isnull", 0)], (), "underflows the stack"),
    ([("const", 0), ("const", 0), ("when_else", 0)], (1.0,), "underflows the stack"),
    ([("const", 0)] * 9 + [("add", 0)] * 8, (1.0,), "overflows the stack of 8"),
    ([("const", 1)], (1.0,), "reads constant 1 of 1"),
    ([("col", 3)], (), "reads vertex column 3 of 3"),
    ([("const", 0), ("msg", 0)], (1.0,), "leaves 2 values"),
]


@pytest.mark.parametrize("ops,consts,text", MALFORMED_VERTEX)
def test_malformed_update_program(ops, consts, text):
    # 2 static + 1 Pregel column: an update may read columns 0 .. 2
    assert call(update=((ops, consts),), n_vcols=2) == _lib.LPA_EINVAL
    assert text in _lib.last_error() and "update[0]" in _lib.last_error(), _lib.last_error()
    assert call(init=(ONE, ONE), update=(ONE, (ops, consts)), n_vcols=1) == _lib.LPA_EINVAL
    assert text in _lib.last_error() and "update[1]" in _lib.last_error(), _lib.last_error()


def test_initial_program_reads_static_columns_only():
    assert call(init=(([("msg", 0)], ()),)) == _lib.LPA_EINVAL
    assert "init[0]" in _lib.last_error() and "message" in _lib.last_error()
    assert call(init=(([("col", 2)], ()),), n_vcols=2) == _lib.LPA_EINVAL   # column 2 is the Pregel column
    assert "init[0]" in _lib.last_error() and "reads vertex column 2 of 2" in _lib.last_error()
    assert call(init=(([("col", 1)], ()),), n_vcols=2) == _lib.LPA_EINVAL and "null handle" in _lib.last_error()
    assert call(init=(([], ()),)) == _lib.LPA_EINVAL and "init[0] has 0 ops" in _lib.last_error()


def test_malformed_message_programs():
    bad = ([("src", 3)], ())
    assert call(to_dst=(ONE, bad), n_vcols=2) == _lib.LPA_EINVAL   # 2 static + 1 Pregel: columns 0 .. 2
    assert "to_dst[1]" in _lib.last_error() and "reads vertex column 3 of 3" in _lib.last_error()
    assert call(to_src=(bad,), n_vcols=2) == _lib.LPA_EINVAL and "to_src[0]" in _lib.last_error()
    assert call(to_dst=(([("src", 2)], ()),), n_vcols=2) == _lib.LPA_EINVAL and "null handle" in _lib.last_error()
    assert call(to_dst=(([(21, 0)], ()),)) == _lib.LPA_EINVAL and "unknown opcode 21" in _lib.last_error()
    assert call(to_dst=(([("edge", 0)], ()),)) == _lib.LPA_EINVAL and "reads edge column 0 of 0" in _lib.last_error()
    assert "lpa_pregel" in _lib.last_error()


def test_deepest_legal_programs_reach_the_handle_check():
    deep_v = ([("msg", 0)] + [("col", 7)] * 7 + [("coalesce", 0)] * 7, ())
    deep_m = ([("const", 0)] * 8 + [("add", 0)] * 7, (1.0,))
    long_v = ([("const", 15)] + [("isnull", 0)] * 63, tuple(range(16)))
    init = ([("const", 0), ("col", 3), ("const", 0), ("when_else", 0)], (0.5,))
    assert call(to_src=(deep_m,) * 4, to_dst=(deep_m,) * 4, init=(init,) * 4, update=(deep_v, long_v, deep_v, long_v),
                n_vcols=4, n_ecols=8, max_iter=2 ** 31 - 1, agg=4) == _lib.LPA_EINVAL
    assert "null handle" in _lib.last_error(), _lib.last_error()


# ---- compile_vertex_program ----
C, D, M = Pregel.col("c"), Pregel.col("d"), Pregel.msg()
ROUND_TRIPS = [
    ("lit", Pregel.lit(2.5), ["const"]),
    ("col", C, ["col"]),
    ("msg", M, ["msg"]),
    ("coalesce", Pregel.coalesce(M, 0.0), ["msg", "const", "coalesce"]),
    ("coalesce_cols", Pregel.coalesce(M * C, D), ["msg", "col", "mul", "col", "coalesce"]),
    ("isnull", Pregel.isnull(M), ["msg", "isnull"]),
    ("isnull_when", Pregel.when(Pregel.isnull(M), C).otherwise(M), ["msg", "isnull", "col", "msg", "when_else"]),
    ("not_isnull", Pregel.when(~Pregel.isnull(M) & (M < C), M), ["msg", "isnull", "not", "msg", "col", "lt", "and",
                                                                  "msg", "when"]),
    ("arith", (C + 1) * D - M / 2, ["col", "const", "add", "col", "mul", "msg", "const", "div", "sub"]),
    ("neg_abs", -abs(C - D), ["col", "col", "sub", "abs", "neg"]),
    ("cmp", (C == D) | (C != 0) | (C <= D) | (C >= D) | (C > D), None),
    ("pagerank", Pregel.coalesce(M, 0.0) * 0.85 + 0.15, ["msg", "const", "coalesce", "const", "mul", "const", "add"]),
]


@pytest.mark.parametrize("name,expr,names", ROUND_TRIPS, ids=[r[0] for r in ROUND_TRIPS])
def test_vertex_program_round_trip(name, expr, names):
    c = gfa.compile_vertex_program(expr, ["c", "d"])
    assert isinstance(c, gfa.CompiledVertexProgram) and c.columns == ("c", "d")
    if names is not None:
        assert [_lib.VP_OPCODES[op] for op, _ in c.ops] == names
    assert c.decode().same(gfa.MessageExpr.of(expr)) and str(c.decode()) == str(gfa.MessageExpr.of(expr))
    assert all(0 <= arg < 2 ** 16 for _, arg in c.ops) and 1 <= c.depth <= 8


def test_vertex_program_column_indices_and_constants():
    c = gfa.compile_vertex_program(C * 2 + D * 2 - 0.0 + (-0.0), ["w", "c", "d"], 1)
    assert c.consts == (2.0, 0.0, -0.0) and str(c.consts[2]) == "-0.0"
    assert [arg for op, arg in c.ops if _lib.VP_OPCODES[op] == "col"] == [1, 2]


def test_vertex_program_refusals():
    with pytest.raises(ValueError, match="Pregel.col"):
        gfa.compile_vertex_program(Pregel.src("c") + 1, ["c"])
    with pytest.raises(ValueError, match="Pregel.col"):
        gfa.compile_vertex_program(Pregel.edge("w"), ["c"])
    with pytest.raises(ValueError, match="none of"):
        gfa.compile_vertex_program(Pregel.col("zz"), ["c"])
    with pytest.raises(ValueError, match="reads the message"):
        gfa.compile_vertex_program(Pregel.coalesce(M, 1), ["c"], initial=True)
    with pytest.raises(ValueError, match="Pregel column 'd'"):
        gfa.compile_vertex_program(C + D, ["c", "d"], 1, initial=True)
    assert gfa.compile_vertex_program(C + 1, ["c", "d"], 1, initial=True).ops[0] == (VOP["col"], 0)
    deep = C
    for _ in range(8):
        deep = C + (deep)      # right-nested: the stack grows
    with pytest.raises(ValueError, match="AM_MAX_STACK"):
        gfa.compile_vertex_program(deep, ["c"])
    long = C
    for _ in range(32):
        long = long + 1
    with pytest.raises(ValueError, match="AM_MAX_OPS"):
        gfa.compile_vertex_program(long, ["c"])
    many = C
    for k in range(17):
        many = many + float(k)
    with pytest.raises(ValueError, match="AM_MAX_CONSTS"):
        gfa.compile_vertex_program(many, ["c"])
    with pytest.raises(ValueError, match="comparison"):
        Pregel.when(M, 1.0)


def test_messages_refuse_the_vertex_vocabulary():
    for expr in (Pregel.col("c"), Pregel.coalesce(Pregel.src("c"), 0.0), Pregel.isnull(Pregel.src("c")),
                 Pregel.when(Pregel.isnull(Pregel.edge("w")), 1.0)):
        with pytest.raises(ValueError, match="vertex expression"):
            gfa.compile_message(expr)
    with pytest.raises(ValueError, match="AM.msg"):
        gfa.compile_message(Pregel.msg() + 1)
    assert gfa.compile_message(Pregel.src("c") * Pregel.edge("w")).ops == gfa.compile_message(
        AM.src["c"] * AM.edge["w"]).ops


# ---- the builder's refusals: all before a handle exists (this machine has no device) ----
@pytest.fixture
def g():
    v = pd.DataFrame({"id": [0, 1, 2, 3], "x": [1.0, 2.0, 3.0, 4.0], "name": list("abcd"),
                      "bad": [1.0, np.nan, 2.0, 3.0], **{f"s{k}": np.arange(4.0) for k in range(8)}})
    e = pd.DataFrame({"src": [0, 1, 2], "dst": [1, 2, 3], "w": [1, 2, 3], "tag": list("pqr"),
                      **{f"e{k}": np.arange(3.0) for k in range(9)}})
    return gfa.GraphFrame(v, e)


def good(g):
    return (g.pregel.withVertexColumn("r", Pregel.col("x"), Pregel.coalesce(Pregel.msg(), 0.0))
            .sendMsgToDst(Pregel.src("r")).aggMsgs(Pregel.sum(Pregel.msg())))


def test_builder_compiles_and_orders_columns(g):
    b = (g.pregel.setMaxIter(3).setCheckpointInterval(2)
         .withVertexColumn("a", Pregel.col("x") * 2, Pregel.col("b") + Pregel.col("s1"))
         .withVertexColumn("b", Pregel.lit(0), Pregel.coalesce(Pregel.msg(), Pregel.col("a")))
         .sendMsgToSrc(Pregel.dst("b") * Pregel.edge("w")).sendMsgToDst(Pregel.src("a") + Pregel.src("s0"))
         .sendMsgToDst(Pregel.edge("e0")).aggMsgs(AM.max(AM.msg)))
    assert g.pregel is not g.pregel and b._max_iter == 3
    agg, to_src, to_dst, init, update, names, vcols, ecols = b._prepare()
    assert agg == "max" and names == ["a", "b"] and len(to_src) == 1 and len(to_dst) == 2
    order = ("s0", "x", "s1", "a", "b")   # static in first-seen order (messages first), then the Pregel ones
    assert all(p.vertex_columns == order for p in to_src + to_dst) and all(p.columns == order for p in init + update)
    assert to_dst[1].edge_columns == ("w", "e0") and len(vcols) == 3 and len(ecols) == 2
    assert np.array_equal(vcols[1], [1.0, 2.0, 3.0, 4.0]) and np.array_equal(ecols[0], [1.0, 2.0, 3.0])
    assert to_src[0].ops == ((AOP["dst"], 4), (AOP["edge"], 0), (AOP["mul"], 0))
    assert init[0].ops[0] == (VOP["col"], 1) and update[0].ops[:2] == ((VOP["col"], 4), (VOP["col"], 2))
    assert g.pregel._max_iter == 10


def test_builder_refusals(g):
    P = Pregel
    good(g)._prepare()
    cases = [
        ("no vertex column", lambda: g.pregel.sendMsgToDst(P.lit(1)).aggMsgs(P.sum(P.msg()))._prepare()),
        ("no message", lambda: g.pregel.withVertexColumn("r", 1.0, P.coalesce(P.msg(), 0)).aggMsgs(
            P.sum(P.msg()))._prepare()),
        ("no aggregate", lambda: g.pregel.withVertexColumn("r", 1.0, P.coalesce(P.msg(), 0)).sendMsgToDst(
            P.lit(1))._prepare()),
        ("maxIter", lambda: g.pregel.setMaxIter(0)),
        ("maxIter", lambda: g.pregel.setMaxIter(-1)),
        ("would replace", lambda: g.pregel.withVertexColumn("id", 1.0, 1.0)),
        ("would replace", lambda: g.pregel.withVertexColumn("x", 1.0, 1.0)),
        ("defined twice", lambda: g.pregel.withVertexColumn("r", 1.0, 1.0).withVertexColumn("r", 1.0, 1.0)),
        ("PREGEL_MAX_COLUMNS", lambda: [b := g.pregel] and [b.withVertexColumn(f"c{k}", 1.0, 1.0) for k in range(5)]),
        ("PREGEL_MAX_MESSAGES", lambda: [b := g.pregel] and [b.sendMsgToDst(1.0) for k in range(5)]),
        ("PREGEL_MAX_MESSAGES", lambda: [b := g.pregel] and [b.sendMsgToSrc(1.0) for k in range(5)]),
        ("Pregel column 'r'", lambda: good(g).withVertexColumn("q", P.col("r"), 1.0)._prepare()),
        ("reads the message", lambda: good(g).withVertexColumn("q", P.coalesce(P.msg(), 1.0), 1.0)._prepare()),
        ("Pregel.col", lambda: good(g).withVertexColumn("q", 1.0, P.src("x") + 1)._prepare()),
        ("Pregel.col", lambda: good(g).withVertexColumn("q", P.edge("w"), 1.0)._prepare()),
        ("vertex expression", lambda: good(g).sendMsgToSrc(P.col("x"))._prepare()),
        ("vertex expression", lambda: good(g).sendMsgToSrc(P.coalesce(P.src("x"), 1.0))._prepare()),
        ("no column 'nope'", lambda: good(g).sendMsgToSrc(P.src("nope"))._prepare()),
        ("no column 'nope'", lambda: good(g).withVertexColumn("q", 1.0, P.col("nope"))._prepare()),
        ("no column 'nope'", lambda: good(g).sendMsgToSrc(P.edge("nope"))._prepare()),
        ("not numeric", lambda: good(g).sendMsgToSrc(P.dst("name"))._prepare()),
        ("not numeric", lambda: good(g).sendMsgToSrc(P.edge("tag"))._prepare()),
        ("holds NaN", lambda: good(g).withVertexColumn("q", P.col("bad"), 1.0)._prepare()),
        ("aggCol", lambda: good(g).aggMsgs(P.msg())),
        ("aggCol", lambda: good(g).aggMsgs(P.sum(P.msg() + 1))),
        ("AM_MAX_VERTEX_COLUMNS", lambda: good(g).sendMsgToSrc(
            sum((P.src(f"s{k}") for k in range(7)), P.src("x")))._prepare()),   # 8 static + r
        ("AM_MAX_EDGE_COLUMNS", lambda: good(g).sendMsgToSrc(
            sum((P.edge(f"e{k}") for k in range(1, 9)), P.edge("e0")))._prepare()),
        ("AM_MAX_STACK", lambda: good(g).withVertexColumn(
            "q", 1.0, P.col("x") + (P.col("x") + (P.col("x") + (P.col("x") + (P.col("x") + (P.col("x") + (
                P.col("x") + (P.col("x") + (P.col("x") + 1)))))))))._prepare()),
    ]
    for text, build in cases:
        with pytest.raises(ValueError, match=text):
            build()
    with pytest.raises(TypeError):
        g.pregel.setMaxIter(2.5)
    with pytest.raises(TypeError):
        Pregel.col(3)
    # exactly the limits pass: 7 static columns + r, 8 edge columns
    good(g).sendMsgToSrc(sum((P.src(f"s{k}") for k in range(6)), P.src("x")))._prepare()
    good(g).sendMsgToSrc(sum((P.edge(f"e{k}") for k in range(1, 8)), P.edge("e0")))._prepare()


# ---- the references against each other ----
def _programs():
    P = Pregel
    return [
        ("sum", [P.dst("a") - P.edge("k")], [P.src("a") * P.edge("k"), P.when(P.src("x") > P.dst("x"), P.src("b"))],
         [("a", P.col("x"), P.coalesce(P.msg(), P.col("b")) - P.col("a")),
          ("b", P.lit(1), P.when(P.isnull(P.msg()), P.col("b") + 1).otherwise(P.col("a")))]),
        ("min", [P.dst("a") + 1], [P.src("a") + 1],
         [("a", P.col("x"), P.when(P.msg() < P.col("a"), P.msg()).otherwise(P.col("a")))]),
        ("max", [], [P.src("a") / P.dst("x")], [("a", P.col("x"), P.coalesce(P.msg() * 0.5, -P.col("a")))]),
        ("avg", [P.when(P.edge("k") > 0, P.dst("a"))], [], [("a", P.col("x") * 4, P.coalesce(P.msg(), 0.0))]),
        ("count", [P.lit(1)], [P.when(P.src("a") > 0, 1)], [("a", P.col("x"), P.coalesce(P.msg(), 0) - P.col("x"))]),
    ]


@pytest.mark.parametrize("k", range(5))
def test_loop_reference_equals_numpy_reference(k):
    V, s, d = random_multigraph(24, 90, 3)
    s, d = s.copy(), d.copy()
    d[:4] = s[:4]                      # self-loops
    s[4:8], d[4:8] = s[8:12], d[8:12]  # duplicates
    s[12], d[13] = -1, V               # no edges
    rng = np.random.default_rng(5)
    vcols = {"x": rng.integers(-3, 4, V).astype(np.float64)}
    ecols = {"k": rng.integers(0, 3, s.size).astype(np.float64)}
    agg, to_src, to_dst, columns = _programs()[k]
    trace, tot = pregel_ref.run(V, s, d, 3, agg, to_src, to_dst, columns, vcols, ecols)
    loop = pregel_ref.run_loop(V, s, d, 3, agg, to_src, to_dst, columns, vcols, ecols)
    assert len(trace) == 4 and tot["edges"] == s.size - 2 and tot["iterations"] == 3
    for name, _, _ in columns:
        assert am_ref_same(trace[-1]["cols"][name], loop[name]), name
    n_prog = len(to_src) + len(to_dst)
    assert tot["messages_to_src"] + tot["messages_to_dst"] + tot["nulls"] == 3 * n_prog * tot["edges"]


def am_ref_same(a, b):
    import am_ref

    return am_ref.same_bits(a, b)


def test_references_raise_on_a_null_update():
    V, s, d = 3, np.array([0]), np.array([1])
    columns = [("a", Pregel.lit(1.0), Pregel.coalesce(Pregel.msg(), 0.0)), ("b", Pregel.lit(1.0), Pregel.msg() * 2.0)]
    for fn in (pregel_ref.run, pregel_ref.run_loop):
        with pytest.raises(pregel_ref.NullUpdate) as err:
            fn(V, s, d, 2, "sum", [], [Pregel.src("a")], columns)
        assert (err.value.iteration, err.value.column, err.value.vertex) == (1, "b", 0)
    with pytest.raises(pregel_ref.NullUpdate) as err:
        pregel_ref.run(V, s, d, 1, "sum", [], [Pregel.lit(1)],
                       [("a", Pregel.col("x") / Pregel.col("x"), Pregel.lit(0))], {"x": np.array([1.0, 0.0, 2.0])})
    assert (err.value.iteration, err.value.vertex) == (0, 1)


def test_reference_exactness_assertion_fires():
    V, s, d = 3, np.array([0, 1]), np.array([2, 2])
    cols = [("a", Pregel.col("x"), Pregel.coalesce(Pregel.msg(), 0.0))]
    pregel_ref.run(V, s, d, 2, "sum", [], [Pregel.src("a")], cols, {"x": np.array([0.5, 0.25, 1.0])}, q=0.25)
    with pytest.raises(AssertionError):
        pregel_ref.run(V, s, d, 2, "sum", [], [Pregel.src("a")], cols, {"x": np.array([0.5, 0.1, 1.0])}, q=0.25)
    with pytest.raises(AssertionError):
        pregel_ref.run(V, s, d, 2, "sum", [], [Pregel.src("a") * 2.0 ** 60], cols, {"x": np.array([1.0, 1.0, 1.0])},
                       q=1.0)
