"""Message aggregation on the GPU (lpa_aggregate_messages, csrc/lpa_agg.hip) against the CPU
references of tests/am_ref.py, which walk the expression tree and never see the compiled program.

count, min and max are compared bit for bit: that pins every message's bits, division included.
sum is compared bit for bit where the messages are integers with |sum| < 2^53, and otherwise
within |gpu - fsum| <= gamma(L) * sum |m| per vertex, L the vertex's message-list length and
gamma(L) = L u / (1 - L u), u = 2^-53: the bound of a sum of at most L terms in any order
(am_ref.gamma), derived from each case's own lists.  The worst ratio to that bound is printed.

A graph handle accepts in-range edges only (lpa_graph_create refuses any other), so edges with an
endpoint that is no vertex reach the call through GraphFrame's indexing, which drops them."""
import numpy as np
import pandas as pd
import pytest

import am_ref
import pr_ref
from graphs import degree_mix, random_multigraph

pytestmark = pytest.mark.gpu

K_AM_SHORT, K_AM_WAVE = 32, 1024   # lpa_internal.h kAmShort / kAmWave
LENGTHS = sorted(set(range(11)) | {31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048,
                                   2049, 4095, 4096, 4097, 8193}
                 | {K_AM_SHORT - 1, K_AM_SHORT + 1, K_AM_WAVE - 1, K_AM_WAVE + 1})
AM_OVERRIDES = [{}, {"LPA_AM_SHORT": "0"}, {"LPA_AM_WAVE": "0"}, {"LPA_AM_SHORT": "0", "LPA_AM_WAVE": "0"},
                {"LPA_AM_SHORT": "100000"}]


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


@pytest.fixture(scope="module")
def AM(gfa):
    return gfa.AggregateMessages


def _i32(x):
    return np.ascontiguousarray(np.asarray(x), dtype=np.int32)


def columns(V, m, seed):
    """Two vertex columns and two edge columns of each kind: small integers (x, c; k), reals (y; w)."""
    rng = np.random.default_rng(seed)
    vcols = {"x": rng.integers(-3, 4, V).astype(np.float64), "y": rng.standard_normal(V),
             "c": rng.integers(0, 3, V).astype(np.float64)}
    ecols = {"w": rng.standard_normal(m), "k": rng.integers(0, 3, m).astype(np.float64)}
    return vcols, ecols


def run(gfa, g, to_src, to_dst, vcols=None, ecols=None, stats=False):
    """Graph.aggregate_messages of two expressions over named columns."""
    vcols, ecols = vcols or {}, ecols or {}
    cs = None if to_src is None else gfa.compile_message(to_src)
    cd = None if to_dst is None else gfa.compile_message(
        to_dst, *(() if cs is None else (cs.vertex_columns, cs.edge_columns)))
    last = cd if cd is not None else cs
    vc = np.stack([vcols[n] for n in last.vertex_columns]) if last.vertex_columns else None
    ec = np.stack([ecols[n] for n in last.edge_columns]) if last.edge_columns else None
    return g.aggregate_messages(cs, cd, vc, ec, stats=stats)


def check(got, ref, exact_sum, what=""):
    """count, min, max bit-equal; sum bit-equal (exact_sum) or within the bound.  Returns the
    worst |gpu - fsum| / (gamma(L) * sum |m|)."""
    assert got["count"].dtype == np.int64 and all(got[k].dtype == np.float64 for k in ("sum", "min", "max"))
    assert np.array_equal(got["count"], ref["count"]), what
    assert am_ref.same_bits(got["min"], ref["min"]), what
    assert am_ref.same_bits(got["max"], ref["max"]), what
    assert np.array_equal(got["sum"][ref["count"] == 0], np.zeros(int((ref["count"] == 0).sum()))), what
    if exact_sum:
        assert np.abs(ref["fsum"]).max(initial=0.0) < 2.0 ** 53
        assert np.array_equal(got["sum"], ref["fsum"]), what
        return 0.0
    bound = am_ref.gamma(ref["rows"]) * ref["abs_sum"]
    err = np.abs(got["sum"] - ref["fsum"])
    assert (err <= bound).all(), (what, float(err.max()))
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def check_summary(summ, ref, V, short=K_AM_SHORT, wave=K_AM_WAVE):
    L = ref["rows"]
    n_wave = int(((L > short) & (L <= wave)).sum())
    n_block = int(((L > short) & (L > wave)).sum())
    assert summ == dict(edges=ref["edges"], messages_to_src=ref["messages_to_src"],
                        messages_to_dst=ref["messages_to_dst"], nulls=ref["nulls"],
                        receivers=int((ref["count"] > 0).sum()), rows_short=V - n_wave - n_block, rows_wave=n_wave,
                        rows_block=n_block, max_row=int(L.max(initial=0)))


# ---- 1. degenerate graphs ----
def test_no_vertices(gfa, AM):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        got, summ = run(gfa, g, AM.lit(1), AM.lit(2), stats=True)
        assert all(got[k].size == 0 for k in ("count", "sum", "min", "max")) and got["count"].dtype == np.int64
        assert summ == dict(edges=0, messages_to_src=0, messages_to_dst=0, nulls=0, receivers=0, rows_short=0,
                            rows_wave=0, rows_block=0, max_row=0)


def test_one_vertex_three_self_loops(gfa, AM):
    z = _i32([0, 0, 0])
    w = {"w": np.array([1.5, -2.0, 4.0])}
    with gfa.Graph(z, z, 1) as g:
        got, summ = run(gfa, g, AM.edge["w"], -AM.edge["w"], ecols=w, stats=True)
        assert got["count"].tolist() == [6] and got["sum"].tolist() == [0.0]
        assert got["min"].tolist() == [-4.0] and got["max"].tolist() == [4.0]
        assert summ["edges"] == 3 and summ["messages_to_src"] == 3 and summ["messages_to_dst"] == 3
        assert summ["max_row"] == 6 and summ["receivers"] == 1 and summ["nulls"] == 0
        got = run(gfa, g, None, AM.when(AM.edge["w"] > 0, AM.edge["w"]), ecols=w)
        assert got["count"].tolist() == [2] and got["sum"].tolist() == [5.5]


def test_edgeless(gfa, AM):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 70) as g:
        got, summ = run(gfa, g, AM.src["x"], None, vcols={"x": np.arange(70.0)}, stats=True)
        assert not got["count"].any() and not got["sum"].any()
        assert np.isnan(got["min"]).all() and np.isnan(got["max"]).all()
        assert summ["edges"] == 0 and summ["receivers"] == 0 and summ["rows_short"] == 70


def test_edges_with_an_endpoint_that_is_no_vertex(gfa, AM):
    """Through GraphFrame's indexing (ids 0, 2, 4, ...: odd and negative ends name no vertex)."""
    rng = np.random.default_rng(4)
    V, m = 40, 600
    ids = np.arange(V) * 2
    s, d = rng.integers(-6, 2 * V + 6, m), rng.integers(-6, 2 * V + 6, m)
    v = pd.DataFrame({"id": ids, "x": rng.integers(-3, 4, V).astype(np.float64)})
    e = pd.DataFrame({"src": s, "dst": d, "w": rng.integers(1, 5, m)})
    ok = (s % 2 == 0) & (d % 2 == 0) & (s >= 0) & (s < 2 * V) & (d >= 0) & (d < 2 * V)
    assert 0 < ok.sum() < m
    ref = am_ref.aggregate(V, np.where(ok, s // 2, -1), np.where(ok, d // 2, -1), AM.src["x"] * AM.edge["w"],
                           AM.dst["x"] - AM.edge["w"], {"x": v["x"].to_numpy()}, {"w": e["w"].to_numpy()})
    assert ref["edges"] == ok.sum()
    out = gfa.GraphFrame(v, e).aggregateMessages(AM.sum(AM.msg), sendToSrc=AM.src["x"] * AM.edge["w"],
                                                 sendToDst=AM.dst["x"] - AM.edge["w"])
    assert np.array_equal(out["id"].to_numpy(), ids[ref["count"] > 0])
    assert np.array_equal(out["sum(MSG)"].to_numpy(), ref["fsum"][ref["count"] > 0])


# ---- 2. every boundary of the row forms ----
def _row_graph(split):
    """Vertex i < len(LENGTHS) has a message list of LENGTHS[i] entries: all in-edges (split
    False), or L // 2 in-edges and L - L // 2 out-edges (split True); the other ends are drawn,
    with repeats, from 700 further vertices and the listed ones (self-loops among them)."""
    rng = np.random.default_rng(11)
    n = len(LENGTHS)
    V = n + 700
    src, dst = [], []
    for i, L in enumerate(LENGTHS):
        n_in = L // 2 if split else L
        others = rng.integers(n if split else 0, V, L)   # split: the far ends add nothing to a listed row
        if not split and L:
            others[0] = i                                # a self-loop
        src += [others[:n_in], np.full(L - n_in, i)]
        dst += [np.full(n_in, i), others[n_in:]]
    return V, _i32(np.concatenate(src)), _i32(np.concatenate(dst))


@pytest.fixture(scope="module")
def row_cases(AM):
    """way -> (V, src, dst, to_src, to_dst, vcols, ecols, reference of the real-valued message,
    reference of the integer-valued one)."""
    real = lambda: AM.src["y"] * AM.edge["w"] + AM.dst["y"]
    whole = lambda: AM.when(AM.edge["k"] > 0, AM.src["x"] - AM.dst["x"] * AM.edge["k"])
    out = {}
    for way in ("to_dst", "to_src", "both"):
        V, s, d = _row_graph(way == "both")
        if way == "to_src":
            s, d = d, s   # the transposed graph
        vcols, ecols = columns(V, s.size, 3)
        dirs = {"to_dst": (None, 1), "to_src": (1, None), "both": (1, 1)}[way]
        prog = [tuple(f() if x else None for x in dirs) for f in (real, whole)]
        refs = [am_ref.aggregate(V, s, d, p[0], p[1], vcols, ecols) for p in prog]
        assert np.array_equal(refs[0]["rows"][:len(LENGTHS)], LENGTHS)
        out[way] = (V, s, d, prog, vcols, ecols, refs)
    assert 30_000 < out["to_dst"][1].size < 40_000
    return out


@pytest.mark.parametrize("env", AM_OVERRIDES, ids=lambda e: ",".join(f"{k[7:]}={v}" for k, v in e.items()) or "defaults")
@pytest.mark.parametrize("way", ["to_dst", "to_src", "both"])
def test_form_boundaries(gfa, monkeypatch, row_cases, way, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)   # read when the handle is created
    short = int(env.get("LPA_AM_SHORT", K_AM_SHORT))
    wave = int(env.get("LPA_AM_WAVE", K_AM_WAVE))
    V, s, d, prog, vcols, ecols, refs = row_cases[way]
    with gfa.Graph(s, d, V) as g:
        got, summ = run(gfa, g, *prog[0], vcols, ecols, stats=True)
        worst = check(got, refs[0], False, (way, env))
        check_summary(summ, refs[0], V, short, wave)
        got, summ = run(gfa, g, *prog[1], vcols, ecols, stats=True)
        check(got, refs[1], True, (way, env))
        check_summary(summ, refs[1], V, short, wave)
        assert summ["nulls"] > 0
    print(f"form boundaries {way} {env}: worst |gpu - fsum| / bound = {worst:.3g}")


# ---- 3. every opcode and the null rules ----
def _programs(AM):
    sx, dx, sy, dy, sc, dc = (AM.src["x"], AM.dst["x"], AM.src["y"], AM.dst["y"], AM.src["c"], AM.dst["c"])
    ew, ek = AM.edge["w"], AM.edge["k"]
    # (name, to_src, to_dst, the messages are integers)
    return [
        ("when without otherwise", AM.when(sc != dc, 1.0), AM.when(sc != dc, 1.0), True),
        ("all null one way", AM.when(ek == 7, 1.0), sx < dx, True),
        ("divide by zero", sy / dx, ew / ek, False),
        ("divide, every comparison", AM.when((sx / dx >= 1) | (sx / dx <= -1), sy / dx),
         AM.when((ew > 0) & (ek < 2), dy / ek).otherwise(AM.when(sx == dx, ew)), False),
        ("null condition", AM.when(sy / dx > 0, ew), AM.when(sy / dx > 0, ew).otherwise(-ew), False),
        ("and or not abs", AM.when((sc == 0) & (dc > 0) | ~(ek >= 1), abs(sy)), abs(sx - dx) * AM.lit(2), False),
        ("negative zero", -sx * 0, AM.when(sx > 0, -dx * 0).otherwise(dx * 0), True),
        ("null through or, both branches", (sx / dx == 1) | (ek == 0),
         AM.when(ek > 0, sy / sx).otherwise(dy / sx), False),
        ("constants", AM.lit(0.1) + 0.2 - sx * 1e-3 + 3, AM.lit(7), False),
        ("four columns", sx * ew + sc * ek, dy * ew - dc / (ek + 1) + sy, False),
    ]


@pytest.fixture(scope="module")
def mixed():
    V, s, d = random_multigraph(300, 4000, 5)
    s[:600], d[:600] = np.random.default_rng(6).integers(0, V, 600), 17      # a wave-form row
    d[600:620] = s[600:620]                                                   # self-loops
    s[620:700], d[620:700] = s[700:780], d[700:780]                           # duplicates
    vcols, ecols = columns(V, s.size, 8)
    return V, s, d, vcols, ecols


@pytest.mark.parametrize("k", range(10))
def test_opcodes_and_null_rules(gfa, AM, mixed, k):
    V, s, d, vcols, ecols = mixed
    name, to_src, to_dst, whole = _programs(AM)[k]
    ref = am_ref.aggregate(V, s, d, to_src, to_dst, vcols, ecols)
    with gfa.Graph(s, d, V) as g:
        got, summ = run(gfa, g, to_src, to_dst, vcols, ecols, stats=True)
    worst = check(got, ref, whole, name)
    check_summary(summ, ref, V)
    if k < 5:
        assert ref["nulls"] > 0, name
    print(f"{name}: nulls {ref['nulls']}, worst |gpu - fsum| / bound = {worst:.3g}")


def test_vertex_without_a_message_is_absent(gfa, AM):
    """Vertex 2 only receives nulls: count 0 in the arrays, no row in the frame."""
    v = pd.DataFrame({"id": [0, 1, 2, 3], "x": [1.0, 2.0, 0.0, 4.0]})
    e = pd.DataFrame({"src": [0, 1, 3, 0], "dst": [2, 2, 2, 1]})
    msg = AM.when(AM.dst["x"] > 0, AM.src["x"])
    with gfa.Graph(_i32(e["src"]), _i32(e["dst"]), 4) as g:
        got, summ = run(gfa, g, None, msg, {"x": v["x"].to_numpy()}, stats=True)
    assert got["count"].tolist() == [0, 1, 0, 0] and np.isnan(got["min"][2]) and got["sum"][2] == 0.0
    assert summ["nulls"] == 3 and summ["receivers"] == 1 and summ["messages_to_dst"] == 1
    out = gfa.GraphFrame(v, e).aggregateMessages(AM.count(AM.msg), sendToDst=msg)
    assert out["id"].tolist() == [1] and out["count(MSG)"].tolist() == [1] and out["count(MSG)"].dtype == np.int64
    out = gfa.GraphFrame(v, e).aggregateMessages(AM.sum(AM.msg), sendToDst=AM.dst["x"] > 0)   # a bare comparison
    assert out["id"].tolist() == [1, 2] and out["sum(MSG)"].tolist() == [1.0, 0.0]


# ---- 4. determinism ----
def test_bit_identical_across_calls_handles_and_edge_orders(gfa, AM, mixed):
    V, s, d, vcols, ecols = mixed
    free = (AM.src["y"] / AM.dst["x"], AM.src["y"] * AM.dst["y"] + AM.src["x"])    # no edge column
    tied = (AM.src["y"] * AM.edge["w"], AM.when(AM.edge["k"] > 0, AM.edge["w"] - AM.dst["y"]))
    perm = np.random.default_rng(9).permutation(s.size)
    pcols = {k: c[perm] for k, c in ecols.items()}
    with gfa.Graph(s, d, V) as g, gfa.Graph(s, d, V) as g2, gfa.Graph(s[perm], d[perm], V) as gp:
        for prog in (free, tied):
            a, sa = run(gfa, g, *prog, vcols, ecols, stats=True)
            b, sb = run(gfa, g, *prog, vcols, ecols, stats=True)
            c, sc = run(gfa, g2, *prog, vcols, ecols, stats=True)
            p, sp = run(gfa, gp, *prog, vcols, pcols, stats=True)
            assert sa == sb == sc == sp
            for key in ("sum", "min", "max"):
                assert am_ref.same_bits(a[key], b[key]) and am_ref.same_bits(a[key], c[key]), key
            assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["count"], c["count"])
            assert np.array_equal(a["count"], p["count"])
            assert am_ref.same_bits(a["min"], p["min"]) and am_ref.same_bits(a["max"], p["max"])
            ref = am_ref.aggregate(V, s[perm], d[perm], *prog, vcols, pcols)
            worst = check(p, ref, False, "permuted")
            if prog is free:
                assert am_ref.same_bits(a["sum"], p["sum"])
            print(f"permuted edge order: worst |gpu - fsum| / bound = {worst:.3g}")


# ---- 5. cross-checks against calls the library already had ----
def test_count_of_one_is_the_in_degree(gfa, AM):
    V, s, d = degree_mix()
    v = pd.DataFrame({"id": np.arange(V)})
    e = pd.DataFrame({"src": s, "dst": d})
    gf = gfa.GraphFrame(v, e)
    indeg = gf.inDegrees()
    out = gf.aggregateMessages(AM.count(AM.msg), sendToDst=AM.lit(1))
    want = indeg[indeg["inDegree"] > 0]
    assert np.array_equal(out["id"].to_numpy(), want["id"].to_numpy())
    assert np.array_equal(out["count(MSG)"].to_numpy(), want["inDegree"].to_numpy())
    gf.close()


def test_one_pagerank_superstep(gfa, AM):
    V, s, d = degree_mix()
    outdeg, indeg = pr_ref.degrees(V, s, d)
    w = np.zeros(V)
    np.divide(1.0, outdeg, out=w, where=outdeg > 0)
    r = np.random.default_rng(2).random(V) + 0.5
    want = np.bincount(d, weights=(r * w)[s], minlength=V)   # s[v] of one superstep of pr_ref._run
    with gfa.Graph(s, d, V) as g:
        got = run(gfa, g, None, AM.src["r"] * AM.src["w"], {"r": r, "w": w})
    assert np.array_equal(got["count"], indeg)
    assert (np.abs(got["sum"] - want) <= pr_ref.bound(1, int(indeg.max()), V) * want).all()


def test_cross_community_edge_ends(gfa, AM):
    V, s, d = degree_mix()
    v = pd.DataFrame({"id": np.arange(V)})
    e = pd.DataFrame({"src": s, "dst": d})
    gf = gfa.GraphFrame(v, e)
    lab = gf.labelPropagation(5)
    gf.close()
    label = lab.sort_values("id")["label"].to_numpy()
    cross = label[s] != label[d]
    want = np.bincount(s[cross], minlength=V) + np.bincount(d[cross], minlength=V)
    assert want.max() > 0 and (want == 0).any()
    msg = AM.when(AM.src["label"] != AM.dst["label"], 1.0)
    out = gfa.aggregate_messages(lab, e, AM.sum(AM.msg), sendToSrc=msg, sendToDst=msg)
    assert np.array_equal(out["id"].to_numpy(), np.flatnonzero(want))
    assert np.array_equal(out["sum(MSG)"].to_numpy(), want[want > 0].astype(np.float64))


# ---- 6. drop-in ----
def test_graphframe_drop_in(gfa, AM):
    """String ids, a dangling edge, a repeated vertex id (its first row stands), an extra column."""
    v = pd.DataFrame({"id": ["d", "a", "c", "a", "b"], "x": [4.0, 1.0, 3.0, 100.0, 2.0], "note": list("pqrst")})
    e = pd.DataFrame({"src": ["a", "a", "b", "zz", "c", "c", "a"], "dst": ["b", "c", "c", "a", "c", "nope", "b"],
                      "w": [1, 2, 3, 4, 5, 6, 7], "tag": list("abcdefg")})
    gf = gfa.GraphFrame(v, e)
    # kept edges: a->b (1), a->c (2), b->c (3), c->c (5), a->b (7); x: a 1, b 2, c 3, d 4
    out = gf.aggregateMessages(AM.avg(AM.msg).alias("mean_in"), sendToDst=AM.src["x"] * AM.edge["w"])
    assert list(out.columns) == ["id", "mean_in"] and out["mean_in"].dtype == np.float64
    assert out["id"].tolist() == ["b", "c"]
    assert out["mean_in"].tolist() == [(1.0 + 7.0) / 2, (2.0 + 6.0 + 15.0) / 3]
    out = gf.aggregateMessages(AM.mean(AM.msg), sendToDst=AM.src["x"] * AM.edge["w"])
    assert list(out.columns) == ["id", "avg(MSG)"] and out["avg(MSG)"].tolist() == [4.0, 23.0 / 3]
    both = dict(sendToSrc=AM.dst["x"] + AM.edge["w"], sendToDst=AM.src["x"] - AM.edge["w"])
    # a: 3, 5, 9 | b: 0, -6, 6 | c: -1, -1, 8 (its loop's to-src), -2 (its loop's to-dst)
    want = {"sum": [17.0, 0.0, 4.0], "min": [3.0, -6.0, -2.0], "max": [9.0, 6.0, 8.0], "count": [3, 3, 4]}
    for kind, col in want.items():
        out = gf.aggregateMessages(getattr(AM, kind)(AM.msg), **both)
        assert out["id"].tolist() == ["a", "b", "c"] and out[f"{kind}(MSG)"].tolist() == col, kind
        assert out[f"{kind}(MSG)"].dtype == (np.int64 if kind == "count" else np.float64)
        fn = gfa.aggregate_messages(v, e, getattr(AM, kind)(AM.msg).alias("t"), **both)
        assert fn["id"].tolist() == ["a", "b", "c"] and fn["t"].tolist() == col
    gf.close()


def test_graphframe_integral_ids_sorted(gfa, AM):
    rng = np.random.default_rng(12)
    ids = rng.permutation(np.arange(1000, 1400, 3))
    v = pd.DataFrame({"id": ids, "x": rng.integers(0, 5, ids.size)})
    e = pd.DataFrame({"src": rng.choice(ids, 900), "dst": rng.choice(ids, 900)})
    out = gfa.aggregate_messages(v, e, AM.max(AM.msg), sendToSrc=AM.dst["x"])
    x = dict(zip(v["id"], v["x"]))
    want = e.assign(m=e["dst"].map(x)).groupby("src")["m"].max()
    assert out["id"].is_monotonic_increasing and out["id"].tolist() == want.index.tolist()
    assert out["max(MSG)"].tolist() == want.astype(np.float64).tolist()


# ---- 7. partitioned job: rank 0 keeps the edge list ----
def test_two_loopback_ranks(gfa, AM):
    V, s, d = degree_mix()
    vcols, ecols = columns(V, s.size, 1)
    prog = (AM.src["y"] * AM.edge["w"], AM.when(AM.edge["k"] > 0, AM.dst["x"]))
    with gfa.Graph(s, d, V) as g:
        single = run(gfa, g, *prog, vcols, ecols, stats=True)
    lb = gfa.Loopback(2)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(2)]
    try:
        got, summ = run(gfa, ranks[0], *prog, vcols, ecols, stats=True)
        assert summ == single[1] and np.array_equal(got["count"], single[0]["count"])
        for key in ("sum", "min", "max"):
            assert am_ref.same_bits(got[key], single[0][key])
        with pytest.raises(ValueError, match="rank 0"):
            run(gfa, ranks[1], *prog, vcols, ecols)
    finally:
        for g in ranks:
            g.close()
        lb.close()
