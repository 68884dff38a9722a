"""Pregel on the GPU (lpa_pregel, csrc/lpa_pregel.hip) against the CPU references of
tests/pregel_ref.py, which walk the expression trees and never see the compiled programs, and
against the calls the library already had.

Everything but the PageRank program is compared bit for bit.  That is sound where the result does
not depend on the order of a sum: min, max and count always; sum and avg where every message is an
integer multiple of one q = 2^-n and every vertex's sum of magnitudes stays below 2^53 q, which
the reference asserts per iteration on the CPU (pregel_ref.run(q=...)) for the inputs chosen here.
The PageRank program is held to pr_ref.bound, the bound of a sum's shape."""
import numpy as np
import pandas as pd
import pytest

import am_ref
import pr_ref
import pregel_ref
from graphs import random_multigraph

pytestmark = pytest.mark.gpu

K_AM_SHORT, K_AM_WAVE = 32, 1024   # lpa_internal.h kAmShort / kAmWave
LENGTHS = [0, 1, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025]
AM_OVERRIDES = [{}, {"LPA_AM_SHORT": "0"}, {"LPA_AM_WAVE": "0"}, {"LPA_AM_SHORT": "0", "LPA_AM_WAVE": "0"},
                {"LPA_AM_SHORT": "100000"}]
AGGS = ("sum", "min", "max", "avg", "count")


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


@pytest.fixture(scope="module")
def P(gfa):
    return gfa.Pregel


def _i32(x):
    return np.ascontiguousarray(np.asarray(x), dtype=np.int32)


def run(gfa, g, max_iter, agg, to_src, to_dst, columns, vcols=None, ecols=None, stats=False):
    """Graph.pregel of expression trees over named columns; columns: [(name, init, update)].
    Returns name -> [V] (and the summary)."""
    vcols, ecols = vcols or {}, ecols or {}
    names = list(vcols) + [name for name, _, _ in columns]
    edge_names, cs, cd = (), [], []
    for exprs, out in ((to_src, cs), (to_dst, cd)):
        for x in exprs:
            out.append(gfa.compile_message(x, names, edge_names))
            edge_names = out[-1].edge_columns
    init = [gfa.compile_vertex_program(i, names, len(vcols), initial=True) for _, i, _ in columns]
    upd = [gfa.compile_vertex_program(u, names, len(vcols)) for _, _, u in columns]
    vc = np.stack(list(vcols.values())) if vcols else None
    ec = np.stack([ecols[n] for n in edge_names]) if edge_names else None
    res = g.pregel(max_iter, agg, cs, cd, init, upd, vc, ec, stats=stats)
    cols, summ = res if stats else (res, None)
    assert cols.dtype == np.float64 and cols.shape == (len(columns), g.num_vertices)
    out = {name: cols[j] for j, (name, _, _) in enumerate(columns)}
    return (out, summ) if stats else out


def same(got, trace, what=""):
    for name, want in trace[-1]["cols"].items():
        assert am_ref.same_bits(got[name], want), (what, name, np.flatnonzero(got[name] != want)[:5])


def check_summary(summ, tot, V, short=K_AM_SHORT, wave=K_AM_WAVE):
    L = tot["rows"]
    n_wave = int(((L > short) & (L <= wave)).sum())
    n_block = int(((L > short) & (L > wave)).sum())
    assert summ == dict(edges=tot["edges"], messages_to_src=tot["messages_to_src"],
                        messages_to_dst=tot["messages_to_dst"], nulls=tot["nulls"], rows_short=V - n_wave - n_block,
                        rows_wave=n_wave, rows_block=n_block, max_row=int(L.max(initial=0)),
                        iterations=tot["iterations"])


@pytest.fixture(scope="module")
def mixed():
    """The `mixed` shape of the aggregateMessages tests: ~300 vertices, a wave-form row,
    self-loops, duplicates; columns in multiples of 1/4 (vertices) and 1/2 (edges)."""
    V, s, d = random_multigraph(300, 4000, 5)
    s[:600], d[:600] = np.random.default_rng(6).integers(0, V, 600), 17      # a wave-form row
    d[600:620] = s[600:620]                                                   # self-loops
    s[620:700], d[620:700] = s[700:780], d[700:780]                           # duplicates
    rng = np.random.default_rng(8)
    vcols = {"x": rng.integers(-8, 9, V) / 4.0, "y": rng.integers(-8, 9, V) / 4.0}
    ecols = {"w": rng.integers(-3, 4, s.size) / 2.0, "k": rng.integers(0, 3, s.size).astype(np.float64)}
    return V, s, d, vcols, ecols


# ---- 1. one iteration is aggregateMessages ----
@pytest.mark.parametrize("agg", AGGS)
def test_one_iteration_agrees_with_aggregate_messages(gfa, P, mixed, agg):
    V, s, d, vcols, ecols = mixed
    V, vcols = V + 5, {k: np.concatenate([c, np.arange(5.0)]) for k, c in vcols.items()}   # five isolated vertices
    sentinel = -12345.5
    msg_d = P.src("a") * P.edge("w") + P.dst("y")
    msg_s = P.when(P.edge("k") > 0, P.dst("a") - P.src("y") / P.edge("k"))
    columns = [("a", P.col("x"), P.coalesce(P.msg(), sentinel))]
    with gfa.Graph(s, d, V) as g:
        for to_src, to_dst in ((None, msg_d), (msg_s, None), (msg_s, msg_d)):
            names = ["y", "a"]
            cs = None if to_src is None else gfa.compile_message(to_src, names)
            cd = None if to_dst is None else gfa.compile_message(to_dst, names, () if cs is None else cs.edge_columns)
            en = (cd if cd is not None else cs).edge_columns
            am = g.aggregate_messages(cs, cd, np.stack([vcols["y"], vcols["x"]]), np.stack([ecols[n] for n in en]))
            with np.errstate(all="ignore"):
                val = am["sum"] / am["count"] if agg == "avg" else am[agg].astype(np.float64)
            want = np.where(am["count"] > 0, val, sentinel)
            assert (am["count"][-5:] == 0).all() and (am["count"] > 0).any()
            got = run(gfa, g, 1, agg, [x for x in (to_src,) if x is not None], [x for x in (to_dst,) if x is not None],
                      columns, {"y": vcols["y"], "x": vcols["x"]}, ecols)
            assert am_ref.same_bits(got["a"], want), (agg, to_src is not None, to_dst is not None)


# ---- 2. the row forms at their edges ----
def _row_graph(split):
    """Vertex i < len(LENGTHS) has a message list of LENGTHS[i] rows: all in-edges (split False),
    or L // 2 in-edges and L - L // 2 out-edges (split True); the other ends are drawn, with
    repeats, from 300 further vertices and, unsplit, the listed ones (a self-loop among them)."""
    rng = np.random.default_rng(11)
    n = len(LENGTHS)
    V = n + 300
    src, dst = [], []
    for i, L in enumerate(LENGTHS):
        n_in = L // 2 if split else L
        others = rng.integers(n, V, L)
        if not split and L:
            others[0] = i                                # a self-loop
        src += [others[:n_in], np.full(L - n_in, i)]
        dst += [np.full(n_in, i), others[n_in:]]
    return V, _i32(np.concatenate(src)), _i32(np.concatenate(dst))


def _row_program(P, way):
    to_dst = [P.when(P.edge("k") > 0, P.src("a") + P.edge("k"))]
    to_src = [P.dst("a") - P.src("x"), P.lit(1)]
    columns = [("a", P.col("x"), P.when(P.msg() > 100, P.msg() - P.col("a") * 3).otherwise(
        P.coalesce(P.msg(), P.col("a")) + 1))]
    return ([] if way == "to_dst" else to_src), ([] if way == "to_src" else to_dst), columns


@pytest.fixture(scope="module")
def row_cases(P):
    out = {}
    for way in ("to_dst", "to_src", "both"):
        V, s, d = _row_graph(way == "both")
        if way == "to_src":
            s, d = d, s   # the transposed graph: the lists are out-lists
        rng = np.random.default_rng(3)
        vcols = {"x": rng.integers(-3, 4, V).astype(np.float64)}
        ecols = {"k": rng.integers(0, 3, s.size).astype(np.float64)}
        to_src, to_dst, columns = _row_program(P, way)
        trace, tot = pregel_ref.run(V, s, d, 3, "sum", to_src, to_dst, columns, vcols, ecols, q=1.0)
        assert np.array_equal(tot["rows"][:len(LENGTHS)], LENGTHS) and tot["rows"][len(LENGTHS):].max() <= 32
        out[way] = (V, s, d, vcols, ecols, trace, tot)
    return out


@pytest.mark.parametrize("env", AM_OVERRIDES, ids=lambda e: ",".join(f"{k[7:]}={v}" for k, v in e.items()) or "defaults")
@pytest.mark.parametrize("way", ["to_dst", "to_src", "both"])
def test_form_boundaries(gfa, P, monkeypatch, row_cases, way, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)   # read when the handle is created
    short = int(env.get("LPA_AM_SHORT", K_AM_SHORT))
    wave = int(env.get("LPA_AM_WAVE", K_AM_WAVE))
    V, s, d, vcols, ecols, trace, tot = row_cases[way]
    to_src, to_dst, columns = _row_program(P, way)
    with gfa.Graph(s, d, V) as g:
        got, summ = run(gfa, g, 3, "sum", to_src, to_dst, columns, vcols, ecols, stats=True)
    same(got, trace, (way, env))
    check_summary(summ, tot, V, short, wave)
    if way != "to_src":
        assert summ["nulls"] > 0
    if not env:
        assert (summ["rows_wave"], summ["rows_block"]) == (3, 1)   # 33, 1023, 1024 | 1025


# ---- 3. buffer discipline ----
@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_a_value_walks_a_path(gfa, P, k):
    V = 40
    s, d = _i32(np.arange(V - 1)), _i32(np.arange(1, V))
    head = np.zeros(V)
    head[0] = 1.0
    with gfa.Graph(s, d, V) as g:
        got = run(gfa, g, k, "sum", [], [P.src("x")], [("x", P.col("head"), P.coalesce(P.msg(), 0.0))], {"head": head})
    want = np.zeros(V)
    want[k] = 1.0
    assert np.array_equal(got["x"], want)


def test_hub_and_leaves_ping_pong(gfa, P):
    """The hub is a block row, every leaf a short one: each form reads what the other wrote one
    iteration earlier, never in the same one."""
    n = 1100
    V = n + 1
    s, d = _i32(np.arange(1, V)), _i32(np.zeros(n))
    x0 = np.zeros(V)
    x0[0] = 7.0
    columns = [("x", P.col("x0"), P.coalesce(P.msg(), -1.0))]
    with gfa.Graph(s, d, V) as g:
        for k in (1, 2, 3, 4):
            got, summ = run(gfa, g, k, "max", [P.dst("x")], [P.src("x")], columns, {"x0": x0}, stats=True)
            want = np.full(V, 7.0 if k % 2 else 0.0)
            want[0] = 0.0 if k % 2 else 7.0
            assert np.array_equal(got["x"], want), k
            assert summ["rows_block"] == 1 and summ["rows_short"] == n and summ["iterations"] == k
            assert summ["messages_to_dst"] == summ["messages_to_src"] == n * k


def test_two_columns_swap(gfa, P):
    V, s, d = random_multigraph(50, 200, 1)
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(V), rng.standard_normal(V)
    columns = [("a", P.col("x"), P.col("b")), ("b", P.col("y"), P.col("a"))]
    with gfa.Graph(s, d, V) as g:
        for k in (1, 2, 5):
            got = run(gfa, g, k, "count", [], [P.lit(1)], columns, {"x": x, "y": y})
            assert np.array_equal(got["a"], y if k % 2 else x) and np.array_equal(got["b"], x if k % 2 else y)


# ---- 4. algorithms end to end ----
def _blocks(seed=4):
    """~200 vertices: four blocks of random edges, one isolated vertex."""
    rng = np.random.default_rng(seed)
    src, dst, lo = [], [], 0
    for size, m in ((60, 70), (50, 120), (45, 40), (44, 90)):
        src.append(lo + rng.integers(0, size, m)), dst.append(lo + rng.integers(0, size, m))
        lo += size
    return lo + 1, np.concatenate(src), np.concatenate(dst)


def test_min_label_components(gfa, P):
    V, s, d = _blocks()
    perm = np.random.default_rng(1).permutation(V)
    v = pd.DataFrame({"id": np.arange(V), "rank": np.arange(V, dtype=np.float64)})
    e = pd.DataFrame({"src": perm[s], "dst": perm[d]})
    gf = gfa.GraphFrame(v, e)
    want = gf.connectedComponents()
    assert 4 < want["component"].nunique() < V
    got = (gf.pregel.setMaxIter(V)
           .withVertexColumn("c", P.col("rank"), P.when(P.msg() < P.col("c"), P.msg()).otherwise(P.col("c")))
           .sendMsgToDst(P.src("c")).sendMsgToSrc(P.dst("c")).aggMsgs(P.min(P.msg())).run())
    gf.close()
    assert list(got.columns) == ["id", "rank", "c"] and got["c"].dtype == np.float64
    assert np.array_equal(got["id"].to_numpy(), want["id"].to_numpy())
    assert np.array_equal(got["c"].to_numpy(), want["component"].to_numpy().astype(np.float64))


def test_hop_counts(gfa, P):
    V, s, d = _blocks(7)
    s, d = _i32(s), _i32(d)
    source, far = int(s[75]), 1.0e9
    is_source = np.zeros(V)
    is_source[source] = 1.0
    columns = [("d", P.when(P.col("is_source") > 0, 0.0).otherwise(far),
                P.when(P.msg() < P.col("d"), P.msg()).otherwise(P.col("d")))]
    with gfa.Graph(s, d, V) as g:
        got = run(gfa, g, 60, "min", [], [P.src("d") + 1], columns, {"is_source": is_source})
    with gfa.Graph(d, s, V) as rev:   # the reversed graph: from v to the landmark there = from the source to v here
        dist = rev.shortest_paths([source])[0]
    assert 1 < dist.max() < 60 and (dist == -1).any()
    assert np.array_equal(got["d"], np.where(dist >= 0, dist, far).astype(np.float64))


# ---- 5. PageRank as a Pregel program ----
@pytest.fixture(scope="module")
def rmat10(gfa):
    s, d = gfa.gen_rmat(10, 16, seed=1)
    return 1024, _i32(s.cpu().numpy()), _i32(d.cpu().numpy())


@pytest.mark.parametrize("k", [1, 10])
def test_pagerank_program(gfa, P, rmat10, k):
    V, s, d = rmat10
    assert 1.0 - 0.15 == 0.85   # the spec's (1.0 - a) is the constant of the program
    outdeg, indeg = pr_ref.degrees(V, s, d)
    w = np.zeros(V)
    np.divide(1.0, outdeg, out=w, where=outdeg > 0)
    columns = [("rank", P.lit(1.0), 0.15 + 0.85 * P.coalesce(P.msg(), 0.0))]
    with gfa.Graph(s, d, V) as g:
        got = run(gfa, g, k, "sum", [], [P.src("rank") * P.src("w")], columns, {"w": w})["rank"]
        lib = g.pagerank(k)
    got = got * (float(V) / float(got.sum()))
    ref = pr_ref.pagerank(V, s, d, k)[0]
    b = pr_ref.bound(k, int(indeg.max()), V)
    err, err_lib = np.abs(got - ref) / ref, np.abs(got - lib) / lib
    print(f"pagerank program k={k}: worst error / bound vs pr_ref {err.max() / b:.3g}, vs pagerank() "
          f"{err_lib.max() / b:.3g}")
    assert (err <= b).all() and (err_lib <= b).all()


# ---- 6. real-valued programs, exact by construction ----
def _exact_cases(P):
    return {
        "sum": ("sum", [P.dst("a") - P.edge("w")], [P.src("a") * P.edge("w"), P.src("x") + 0.5],
                [("a", P.col("x"), P.coalesce(P.msg(), P.col("a")) * 0.5)], ()),
        "avg": ("avg", [P.dst("a") * 0.5, P.edge("w")], [P.src("a") + P.edge("w")],
                [("a", P.col("y"), P.when(P.msg() > P.col("a"), P.col("a") + 0.5).otherwise(P.col("a") - 0.25)),
                 # nothing reads b: the average itself, one IEEE division of an exact sum by a count
                 ("b", P.lit(0.0), P.coalesce(P.msg(), -1.0))], ("b",)),
    }


@pytest.fixture(scope="module")
def exact_refs(P, mixed):
    V, s, d, vcols, ecols = mixed
    return {key: pregel_ref.run(V, s, d, 3, agg, to_src, to_dst, columns, vcols, ecols, q=2.0 ** -10, free=free)
            for key, (agg, to_src, to_dst, columns, free) in _exact_cases(P).items()}


@pytest.mark.parametrize("key", ["sum", "avg"])
def test_real_valued_exact_by_construction(gfa, P, mixed, exact_refs, key):
    V, s, d, vcols, ecols = mixed
    agg, to_src, to_dst, columns, _ = _exact_cases(P)[key]
    trace, tot = exact_refs[key]
    assert any(np.any(c != np.rint(c)) for c in trace[-1]["cols"].values())   # real values, not integers
    with gfa.Graph(s, d, V) as g:
        got, summ = run(gfa, g, 3, agg, to_src, to_dst, columns, vcols, ecols, stats=True)
    same(got, trace, key)
    check_summary(summ, tot, V)
    assert summ["rows_wave"] >= 1


# ---- 7. determinism ----
def test_bit_identical_across_calls_handles_and_edge_orders(gfa, P, mixed):
    V, s, d, _, _ = mixed
    rng = np.random.default_rng(9)
    vcols = {"x": rng.standard_normal(V), "y": rng.random(V) + 0.5}
    columns = [("a", P.col("x"), P.coalesce(P.msg(), 0.0) / 64 + P.col("a") * 0.25)]
    args = (3, "sum", [P.dst("a") / P.src("y")], [P.src("a") * P.src("y") + P.dst("x")], columns, vcols)
    perm = rng.permutation(s.size)
    with gfa.Graph(s, d, V) as g, gfa.Graph(s, d, V) as g2, gfa.Graph(s[perm], d[perm], V) as gp:
        a, sa = run(gfa, g, *args, stats=True)
        b, sb = run(gfa, g, *args, stats=True)
        c, sc = run(gfa, g2, *args, stats=True)
        p, sp = run(gfa, gp, *args, stats=True)
    assert sa == sb == sc == sp and np.isfinite(a["a"]).all() and np.unique(a["a"]).size > V // 2
    for other in (b, c, p):
        assert am_ref.same_bits(a["a"], other["a"])


# ---- 8. a null update ----
def test_null_update_is_an_error(gfa, P):
    v = pd.DataFrame({"id": [10, 20, 30, 40]})
    e = pd.DataFrame({"src": [10, 20, 20], "dst": [20, 30, 40]})   # 10 receives nothing
    gf = gfa.GraphFrame(v, e)

    def build(update):
        return (gf.pregel.setMaxIter(3).withVertexColumn("keep", P.lit(2.0), P.col("keep"))
                .withVertexColumn("twice", P.lit(1.0), update).sendMsgToDst(P.src("twice"))
                .aggMsgs(P.sum(P.msg())))

    with pytest.raises(ValueError, match=r"'twice'.*iteration 1.*coalesce") as err:
        build(P.msg() * 2.0).run()
    assert "10" in str(err.value)
    got = build(P.coalesce(P.msg() * 2.0, 1.0)).run()   # the handle stays usable
    assert got["twice"].tolist() == [1.0, 2.0, 4.0, 4.0] and got["keep"].tolist() == [2.0] * 4
    with gfa.Graph(_i32([0]), _i32([1]), 3) as g:
        with pytest.raises(gfa.PregelNullError) as low:
            run(gfa, g, 2, "sum", [], [P.src("a")], [("a", P.lit(1.0), P.coalesce(P.msg(), 0.0)),
                                                     ("b", P.lit(1.0), P.when(P.msg() > 5, 1.0))])
        assert (low.value.iteration, low.value.column, low.value.vertex) == (1, 1, 0)
        with pytest.raises(gfa.PregelNullError) as low:
            run(gfa, g, 2, "sum", [], [P.lit(1)], [("a", P.col("x") / P.col("x"), P.lit(0.0))],
                {"x": np.array([1.0, 0.0, 0.0])})
        assert (low.value.iteration, low.value.column, low.value.vertex) == (0, 0, 1)
        assert run(gfa, g, 2, "sum", [], [P.src("a")], [("a", P.lit(1.0), P.coalesce(P.msg(), 0.0))])["a"].tolist() == [
            0.0, 0.0, 0.0]
    gf.close()


# ---- 9. edge cases ----
def test_no_vertices(gfa, P):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        got, summ = run(gfa, g, 3, "sum", [], [P.lit(1)], [("a", P.lit(1.0), P.coalesce(P.msg(), 0.0))], stats=True)
    assert got["a"].shape == (0,) and summ["edges"] == 0 and summ["rows_short"] == 0


def test_edgeless(gfa, P):
    e = np.empty(0, np.int32)
    x = np.arange(70.0)
    with gfa.Graph(e, e, 70) as g:
        got, summ = run(gfa, g, 3, "count", [P.dst("a")], [P.src("a")],
                        [("a", P.col("x"), P.coalesce(P.msg(), P.col("a") + 1)),
                         ("n", P.lit(0.0), P.col("n") + P.isnull(P.msg()))], {"x": x}, stats=True)
    assert np.array_equal(got["a"], x + 3) and np.array_equal(got["n"], np.full(70, 3.0))
    assert summ == dict(edges=0, messages_to_src=0, messages_to_dst=0, nulls=0, rows_short=70, rows_wave=0,
                        rows_block=0, max_row=0, iterations=3)


def test_dangling_edges_through_the_builder(gfa, P):
    """ids 0, 2, 4, ...: odd and out-of-range ends name no vertex; string-free, unsorted vertex rows."""
    rng = np.random.default_rng(4)
    V, m = 40, 600
    ids = np.arange(V) * 2
    s, d = rng.integers(-6, 2 * V + 6, m), rng.integers(-6, 2 * V + 6, m)
    order = rng.permutation(V)
    x = rng.integers(-3, 4, V).astype(np.float64)
    v = pd.DataFrame({"id": ids[order], "x": x[order]})
    e = pd.DataFrame({"src": s, "dst": d, "w": rng.integers(1, 5, m)})
    ok = (s % 2 == 0) & (d % 2 == 0) & (s >= 0) & (s < 2 * V) & (d >= 0) & (d < 2 * V)
    to_src, to_dst = [P.dst("a") - P.edge("w")], [P.src("a") * P.edge("w")]
    columns = [("a", P.col("x"), P.coalesce(P.msg(), 0.0) - P.col("a"))]
    trace, tot = pregel_ref.run(V, np.where(ok, s // 2, -1), np.where(ok, d // 2, -1), 3, "sum", to_src, to_dst,
                                columns, {"x": x}, {"w": e["w"].to_numpy()}, q=1.0)
    assert 0 < tot["edges"] == ok.sum() < m
    gf = gfa.GraphFrame(v, e)
    got = (gf.pregel.setMaxIter(3).withVertexColumn("a", *columns[0][1:]).sendMsgToSrc(to_src[0])
           .sendMsgToDst(to_dst[0]).aggMsgs(P.sum(P.msg())).run())
    gf.close()
    assert np.array_equal(got["id"].to_numpy(), ids) and np.array_equal(got["x"].to_numpy(), x)
    assert np.array_equal(got["a"].to_numpy(), trace[-1]["cols"]["a"])


def test_self_loops_with_both_directions(gfa, P):
    z = _i32([0, 0, 0])
    with gfa.Graph(z, z, 1) as g:
        got, summ = run(gfa, g, 2, "sum", [P.dst("a") * 2], [P.src("a")], [("a", P.lit(1.0), P.coalesce(P.msg(), 0.0))],
                        stats=True)
    assert got["a"].tolist() == [81.0] and summ["max_row"] == 6 and summ["messages_to_src"] == 6


def test_the_maximum_configuration(gfa, P, mixed):
    """4 Pregel columns, 4 programs per direction, 8 vertex columns, 8 edge columns."""
    V, s, d, _, _ = mixed
    rng = np.random.default_rng(13)
    vcols = {f"s{k}": rng.integers(-2, 3, V).astype(np.float64) for k in range(4)}
    ecols = {f"e{k}": rng.integers(0, 3, s.size).astype(np.float64) for k in range(8)}
    to_dst = [P.src(f"p{k}") + P.edge(f"e{k}") - P.dst(f"s{k}") for k in range(4)]
    to_src = [P.when(P.edge(f"e{k + 4}") > 0, P.dst(f"p{k}") * P.edge(f"e{k + 4}") + P.src(f"s{3 - k}"))
              for k in range(4)]
    columns = [(f"p{k}", P.col(f"s{k}") + k,
                P.when(P.msg() > P.col(f"p{(k + 1) % 4}"), P.col(f"p{(k + 1) % 4}") + P.col(f"s{k}")).otherwise(
                    P.coalesce(P.msg(), 1.0) - P.col(f"p{k}"))) for k in range(4)]
    trace, tot = pregel_ref.run(V, s, d, 3, "sum", to_src, to_dst, columns, vcols, ecols, q=1.0)
    with gfa.Graph(s, d, V) as g:
        got, summ = run(gfa, g, 3, "sum", to_src, to_dst, columns, vcols, ecols, stats=True)
    same(got, trace)
    check_summary(summ, tot, V)
    assert summ["nulls"] > 0 and len({tuple(c) for c in got.values()}) == 4


def test_only_rank_zero_of_a_partitioned_job(gfa, P):
    V, s, d = random_multigraph(64, 300, 2)
    args = (2, "max", [], [P.src("a") + 1], [("a", P.lit(0.0), P.coalesce(P.msg(), 0.0))])
    with gfa.Graph(s, d, V) as g:
        single = run(gfa, g, *args)
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        assert np.array_equal(run(gfa, ranks[0], *args)["a"], single["a"])
        with pytest.raises(ValueError, match="rank 0"):
            run(gfa, ranks[1], *args)
    finally:
        for g in ranks:
            g.close()
        lb.close()
