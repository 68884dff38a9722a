"""Motif finding on the GPU (lpa_motif, csrc/lpa_motif.hip) against the CPU references of
tests/motif_ref.py and against closed forms: exact integer equality of every row, every row
count and every summary field.  Graph.motif under every legal execution order of the positive
terms; table sizes around the scan tile; hub lists around the fill's boundaries; closes with
multiplicity; negation; the 3-cycle count against triangle counting; max_rows; determinism; the
drop-in calls GraphFrame.find / motifCount, find, motif_count.

The fill that is kept (k_motif_fill) is a lane per child row, a block per 2048 consecutive child
rows, 256 rows a trip.  The list lengths of test_hub_lists are the issue's (1, 8, 9, 64, 65,
1024, 1025, 4097) plus that fill's own boundaries: 255 / 256 / 257 (a trip of the block) and
2047 / 2048 / 2049 (a parent that ends just before, at, and just after a block's stretch)."""
import itertools

import numpy as np
import pandas as pd
import pytest

import motif_ref
from graphs import degree_mix, random_multigraph

pytestmark = pytest.mark.gpu

RECIPROCAL = "(a)-[e]->(b); (b)-[e2]->(a)"
ONE_WAY = "(a)-[]->(b); !(b)-[]->(a)"
CYCLE3 = "(a)-[]->(b); (b)-[]->(c); (c)-[]->(a)"


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _i32(x):
    return np.ascontiguousarray(np.asarray(x), dtype=np.int32)


def orders(parsed):
    """Every legal execution order of the pattern's terms: a permutation of the positive terms
    in which each one after the first shares a variable with the earlier ones, every negated
    term at the earliest point at which both its variables are bound."""
    terms = parsed.terms
    pos = [i for i, t in enumerate(terms) if not t.negated]
    out = []
    for perm in itertools.permutations(pos):
        bound, plan, neg = set(), [], [i for i, t in enumerate(terms) if t.negated]
        for k, i in enumerate(perm):
            ends = {terms[i].src_var, terms[i].dst_var}
            if k > 0 and not ends & bound:
                plan = None
                break
            bound |= ends
            plan.append(i)
            for j in list(neg):
                if {terms[j].src_var, terms[j].dst_var} <= bound:
                    plan.append(j)
                    neg.remove(j)
        if plan is not None:
            out.append(plan)
    assert 1 <= len(out) <= 24
    return out


def run_plan(g, parsed, plan, **kw):
    """Graph.motif of the pattern's terms in the order `plan`; (vcols, ecols[, summary]) with the
    edge columns keyed by PATTERN term."""
    terms = [(parsed.terms[i].src_var, parsed.terms[i].dst_var, int(parsed.terms[i].negated),
              int(parsed.terms[i].edge is not None)) for i in plan]
    named = [v for v, nm in enumerate(parsed.var_names) if nm is not None]
    got = g.motif(parsed.n_vars, terms, var_out=named, **kw)
    if kw.get("count_only"):
        return got
    ecols = {plan[k]: col for k, col in got[1].items()}
    return (got[0], ecols) + tuple(got[2:])


def sorted_rows(g, gfa, pattern, plan=None):
    parsed = gfa.parse_motif(pattern)
    plan = gfa.plan_motif(parsed) if plan is None else plan
    vcols, ecols = run_plan(g, parsed, plan)
    return motif_ref.rows_of(vcols, ecols, motif_ref.spec(parsed)[2])


def check_all_orders(gfa, V, s, d, pattern, want):
    parsed = gfa.parse_motif(pattern)
    columns = motif_ref.spec(parsed)[2]
    with gfa.Graph(_i32(s), _i32(d), V) as g:
        for plan in orders(parsed):
            vcols, ecols, summ = run_plan(g, parsed, plan, stats=True)
            got = motif_ref.rows_of(vcols, ecols, columns)
            assert got == want, (pattern, plan, len(got), len(want))
            assert summ["rows"] == len(want) and summ["overflow_step"] == -1
            assert run_plan(g, parsed, plan, count_only=True) == len(want)


# ---- 1. degenerate graphs ----
def test_no_vertices(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 0) as g:
        vcols, ecols, summ = g.motif(2, [(0, 1, 0, 1), (1, 0, 0, 1)], stats=True)
        assert set(vcols) == {0, 1} and set(ecols) == {0, 1}
        assert all(c.size == 0 for c in vcols.values()) and all(c.size == 0 for c in ecols.values())
        assert vcols[0].dtype == np.int32 and ecols[0].dtype == np.int64
        assert summ["rows"] == 0 and summ["edges"] == 0 and summ["overflow_step"] == -1
        assert g.motif(2, [(0, 1, 0, 0)], count_only=True) == 0


def test_edgeless(gfa):
    e = np.empty(0, np.int32)
    with gfa.Graph(e, e, 70) as g:
        vcols, ecols = g.motif(2, [(0, 1, 0, 1)])
        assert vcols[0].size == 0 and vcols[1].size == 0 and ecols[0].size == 0
        assert g.motif(3, [(0, 1, 0, 0), (1, 2, 0, 0), (2, 0, 1, 0)], count_only=True) == 0


def test_only_self_loops(gfa):
    s = _i32([3, 5, 3, 9, 5])
    with gfa.Graph(s, s, 12) as g:
        for pattern, want in [("(a)-[e]->(b)", [(int(x), i, int(x)) for i, x in enumerate(s)]),
                              ("(a)-[e]->(a)", [(int(x), i) for i, x in enumerate(s)])]:
            assert sorted_rows(g, gfa, pattern) == sorted(want)
        # a loop is reciprocated by itself and by its duplicates
        got = sorted_rows(g, gfa, RECIPROCAL)
        assert len(got) == 2 * 2 + 2 * 2 + 1 and all(r[0] == r[2] for r in got)
        assert g.motif(2, [(0, 1, 0, 0), (1, 0, 1, 0)], count_only=True) == 0


def test_single_edge_pattern_is_the_edge_list(gfa):
    V, s, d = random_multigraph(50, 400, 7)
    s[10:14], d[10:14] = 4, 4            # loops, duplicated
    s[20:23], d[20:23] = 6, 9            # a triple edge
    ok = np.arange(s.size)               # (a handle takes in-range edges only: every row is an edge)
    with gfa.Graph(s, d, V) as g:
        vcols, ecols, summ = g.motif(2, [(0, 1, 0, 1)], stats=True)
        assert np.array_equal(ecols[0], ok)          # library order: the edge rows ascending
        assert np.array_equal(vcols[0], s[ok]) and np.array_equal(vcols[1], d[ok])
        assert summ["edges"] == ok.size == summ["rows"] and summ["self_loops"] == int((s[ok] == d[ok]).sum())
        assert summ["steps"] == 1 and summ["table_rows"] == [ok.size] and summ["peak_rows"] == ok.size
        vcols, ecols = g.motif(1, [(0, 0, 0, 1)])
        loops = ok[s[ok] == d[ok]]
        assert np.array_equal(ecols[0], loops) and np.array_equal(vcols[0], s[loops])


# ---- 2. literal parity, every execution order ----
def _small_graph(V, m, seed):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, V, m), rng.integers(0, V, m)
    s[0], d[0] = 1, 1                      # a loop
    s[1:4], d[1:4] = s[4], d[4]            # a quadruple edge
    s[5], d[5] = d[4], s[4]                # and its reverse
    return _i32(s), _i32(d)


@pytest.mark.parametrize("pattern", motif_ref.PATTERNS)
@pytest.mark.parametrize("V,m", [(6, 14), (40, 30)])
def test_literal_parity(gfa, pattern, V, m):
    parsed = gfa.parse_motif(pattern)
    sp = motif_ref.spec(parsed)
    if sum(not t.negated for t in parsed.terms) > 3:
        m = min(m, 24)
    for seed in range(10):
        s, d = _small_graph(V, m, 50 + seed)
        check_all_orders(gfa, V, s, d, pattern, motif_ref.literal(V, s, d, *sp))


@pytest.mark.parametrize("pattern", motif_ref.PATTERNS)
def test_merge_chain_parity(gfa, pattern):
    V, m = 300, 3000
    s, d = _small_graph(V, m, 99)
    sp = motif_ref.spec(gfa.parse_motif(pattern))
    check_all_orders(gfa, V, s, d, pattern, motif_ref.merge_chain(V, s, d, *sp))


# ---- 3. table sizes at the scan / sort tile (4096 = 256 x 16) ----
# k disjoint directed 2-paths (3 i -> 3 i + 1 -> 3 i + 2) and `extra` lone edges: 2 k + extra rows
# after the first term, k after the second
@pytest.mark.parametrize("k,extra", [(0, 1), (1, 0), (2047, 1), (2048, 0), (2048, 1), (4095, 0), (4096, 0), (4096, 1),
                                     (4097, 0), (8192, 0), (8193, 0)])
def test_table_sizes_at_the_tile(gfa, k, extra):
    i = np.arange(k)
    s = np.empty(2 * k + extra, np.int32)
    d = np.empty(2 * k + extra, np.int32)
    s[0:2 * k:2], d[0:2 * k:2] = 3 * i, 3 * i + 1
    s[1:2 * k:2], d[1:2 * k:2] = 3 * i + 1, 3 * i + 2
    s[2 * k:], d[2 * k:] = 3 * k, 3 * k + 1
    V = 3 * k + 2
    with gfa.Graph(s, d, V) as g:
        vcols, ecols, summ = g.motif(3, [(0, 1, 0, 1), (1, 2, 0, 1)], stats=True)
        assert summ["table_rows"] == [2 * k + extra, k] and summ["steps"] == 2
        assert summ["rows"] == k and summ["peak_rows"] == 2 * k + extra and summ["edges"] == 2 * k + extra
        # library order: the seed in edge-row order, one child each
        assert np.array_equal(vcols[0], 3 * i) and np.array_equal(vcols[1], 3 * i + 1)
        assert np.array_equal(vcols[2], 3 * i + 2)
        assert np.array_equal(ecols[0], 2 * i) and np.array_equal(ecols[1], 2 * i + 1)
        # the same through the in-lists: (b)-[e2]->(c) first, then (a)-[e]->(b)
        vcols, ecols, summ = g.motif(3, [(1, 2, 0, 1), (0, 1, 0, 1)], stats=True)
        assert summ["table_rows"] == [2 * k + extra, k]
        assert np.array_equal(vcols[0], 3 * i) and np.array_equal(vcols[2], 3 * i + 2)
        assert np.array_equal(ecols[0], 2 * i + 1) and np.array_equal(ecols[1], 2 * i)


# ---- 4. list-length forms ----
@pytest.mark.parametrize("dgr", [1, 8, 9, 64, 65, 255, 256, 257, 1024, 1025, 2047, 2048, 2049, 4097])
def test_hub_lists(gfa, dgr):
    # an out-hub 0 -> 1 .. dgr, and an in-hub: dgr + 1 .. 2 dgr -> 2 dgr + 1
    t = np.arange(1, dgr + 1)
    hub_in = 2 * dgr + 1
    s = _i32(np.concatenate([np.zeros(dgr, np.int64), t + dgr]))
    d = _i32(np.concatenate([t, np.full(dgr, hub_in)]))
    V = 2 * dgr + 2
    n2 = dgr * dgr

    def hub_rows(hub, lst, got, at):
        """The hub's dgr^2 rows (hub, repeat(lst), tile(lst)) at got[at : at + n2]: all of them up
        to 2049, above that the count (the caller's) and the first and last 64."""
        if dgr <= 2049:
            want = (np.full(n2, hub), np.repeat(lst, dgr), np.tile(lst, dgr))
            return all(np.array_equal(got[i][at:at + n2], want[i]) for i in range(3))
        head = (np.full(64, hub), np.full(64, lst[0]), lst[:64])
        tail = (np.full(64, hub), np.full(64, lst[-1]), lst[-64:])
        return all(np.array_equal(got[i][at:at + 64], head[i]) and np.array_equal(got[i][at + n2 - 64:at + n2], tail[i])
                   for i in range(3))

    with gfa.Graph(s, d, V) as g:
        # (a)-[]->(b); (a)-[]->(c): dgr^2 rows from the out-hub, then one per in-hub source
        vcols, _, summ = g.motif(3, [(0, 1, 0, 0), (0, 2, 0, 0)], stats=True)
        assert summ["table_rows"] == [2 * dgr, n2 + dgr] and vcols[0].size == n2 + dgr
        assert hub_rows(0, t, (vcols[0], vcols[1], vcols[2]), 0)
        assert np.array_equal(vcols[0][n2:], t + dgr)
        assert (vcols[1][n2:] == hub_in).all() and (vcols[2][n2:] == hub_in).all()
        # (b)-[]->(a); (c)-[]->(a): one row per out-hub target, then dgr^2 from the in-hub
        vcols, _, summ = g.motif(3, [(1, 0, 0, 0), (2, 0, 0, 0)], stats=True)
        assert summ["table_rows"] == [2 * dgr, n2 + dgr] and vcols[0].size == n2 + dgr
        assert hub_rows(hub_in, t + dgr, (vcols[0], vcols[1], vcols[2]), dgr)
        assert np.array_equal(vcols[0][:dgr], t)
        assert (vcols[1][:dgr] == 0).all() and (vcols[2][:dgr] == 0).all()


# ---- 5. close with multiplicity ----
def test_close_multiplicity(gfa):
    V = 40
    rng = np.random.default_rng(11)
    mult = rng.choice([0, 1, 3], size=(V, V))
    mult[0, 1] = mult[1, 0] = 3
    mult[2, 2] = 3
    a, b = np.nonzero(mult)
    s, d = np.repeat(a, mult[a, b]), np.repeat(b, mult[a, b])
    perm = rng.permutation(s.size)
    s, d = _i32(s[perm]), _i32(d[perm])
    sp = motif_ref.spec(gfa.parse_motif(RECIPROCAL))
    want = motif_ref.merge_chain(V, s, d, *sp)
    check_all_orders(gfa, V, s, d, RECIPROCAL, want)
    for x, y in ((0, 1), (1, 0)):
        assert sum(1 for r in want if r[0] == x and r[2] == y) == 9
    assert sum(1 for r in want if r[0] == 2 and r[2] == 2) == 9


def test_close_equal_range_at_the_list_ends(gfa):
    # u's out-list: 1300 distinct targets from 10 to 2899 and 200 more edges to 700
    V, u = 3000, 1500
    rng = np.random.default_rng(5)
    pool = np.setdiff1d(np.arange(11, 2899), [u, 700, 1200])
    tg = np.concatenate([[10, 2899, 700], rng.choice(pool, 1297, replace=False), np.full(200, 700)])
    assert tg.size == 1500
    back = np.array([10, 2899, 5, 2950, 700, 1200])   # first, last, below, above, the run, absent inside
    s = np.concatenate([np.full(tg.size, u), back])
    d = np.concatenate([tg, np.full(back.size, u)])
    perm = rng.permutation(s.size)
    s, d = _i32(s[perm]), _i32(d[perm])
    sp = motif_ref.spec(gfa.parse_motif(RECIPROCAL))
    want = motif_ref.merge_chain(V, s, d, *sp)
    assert sum(1 for r in want if r[0] == 700 and r[2] == u) == 201 == sum(1 for r in want if r[0] == u and r[2] == 700)
    assert {r[0] for r in want} == {u, 10, 2899, 700}
    check_all_orders(gfa, V, s, d, RECIPROCAL, want)


# ---- 6. negation ----
def _negation_graphs():
    rng = np.random.default_rng(21)
    a, b = rng.integers(0, 200, 1500), rng.integers(0, 200, 1500)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    up = lo < hi
    return {
        "reciprocal": (200, np.concatenate([a, b]), np.concatenate([b, a])),
        "one_way": (200, lo[up], hi[up]),
        "mixed": random_multigraph(300, 3000, 17),
    }


@pytest.mark.parametrize("name", ["reciprocal", "one_way", "mixed"])
def test_negation(gfa, name):
    V, s, d = _negation_graphs()[name]
    s, d = _i32(s), _i32(d)
    sp = motif_ref.spec(gfa.parse_motif(ONE_WAY))
    want = motif_ref.merge_chain(V, s, d, *sp)
    if name == "reciprocal":
        assert want == []
    if name == "one_way":
        assert len(want) == s.size
    check_all_orders(gfa, V, s, d, ONE_WAY, want)
    last = "(a)-[]->(b); (b)-[]->(c); !(c)-[]->(a)"
    want3 = motif_ref.merge_chain(V, s, d, *motif_ref.spec(gfa.parse_motif(last)))
    check_all_orders(gfa, V, s, d, last, want3)
    v = pd.DataFrame({"id": np.arange(V)})
    e = pd.DataFrame({"src": s, "dst": d})
    gf = gfa.GraphFrame(v, e)
    try:
        for pattern, rows in ((ONE_WAY, want), (last, want3)):
            m = gf.find(pattern)
            assert len(m) == len(rows) == m.attrs["rows"] == gf.motifCount(pattern)
            names = ["a", "b", "c"][:len(m.columns)]
            assert list(zip(*(m[nm]["id"].tolist() for nm in names))) == rows
        if name == "reciprocal":
            # an empty table ends the call: the third term never runs
            _, _, summ = gf._gpu_graph().motif(3, [(0, 1, 0, 0), (1, 0, 1, 0), (1, 2, 0, 0)], stats=True)
            assert summ["steps"] == 2 and summ["table_rows"] == [s.size, 0] and summ["rows"] == 0
    finally:
        gf.close()


# ---- 7. the 3-cycle count against triangle counting ----
def test_cycle_count_against_triangle_count(gfa):
    V, s, d = degree_mix(seed=3, hubs=(300, 900, 1500, 2500), n_low=1500, extra=8000)
    lo, hi = np.minimum(s, d).astype(np.int64), np.maximum(s, d).astype(np.int64)
    key = np.unique(lo[lo < hi] * V + hi[lo < hi])          # canonical: simple, loop-free
    lo, hi = key // V, key % V
    s, d = _i32(np.concatenate([lo, hi])), _i32(np.concatenate([hi, lo]))   # symmetrised
    deg = np.bincount(s, minlength=V).astype(np.int64)
    wedges = int((deg * deg).sum())
    assert s.size < wedges < 2 * 10 ** 7
    with gfa.Graph(s, d, V) as g:
        tri = g.triangle_count()
        n, summ = g.motif(3, [(0, 1, 0, 0), (1, 2, 0, 0), (2, 0, 0, 0)], count_only=True, stats=True)
        assert summ["table_rows"] == [s.size, wedges, n]
        assert n == 2 * int(tri.sum()) and n > 0
    gf = gfa.GraphFrame(pd.DataFrame({"id": np.arange(V)}), pd.DataFrame({"src": s, "dst": d}))
    try:
        assert gf.motifCount(CYCLE3) == n
    finally:
        gf.close()


# ---- 8. max_rows ----
def test_max_rows(gfa):
    dgr = 100
    s = _i32(np.concatenate([np.zeros(dgr), [1]]))
    d = _i32(np.concatenate([np.arange(1, dgr + 1), [2]]))
    V = dgr + 1
    terms = [(0, 1, 0, 0), (0, 2, 0, 0), (1, 2, 0, 0)]     # (a)-[]->(b); (a)-[]->(c); (b)-[]->(c)
    peak = dgr * dgr + 1
    with gfa.Graph(s, d, V) as g:
        vcols, _, summ = g.motif(3, terms, max_rows=peak, stats=True)
        assert summ["table_rows"] == [dgr + 1, peak, 1] and summ["peak_rows"] == peak
        assert [int(vcols[i][0]) for i in range(3)] == [0, 1, 2]
        # the final table has one row; the wedge table before it does not fit
        with pytest.raises(ValueError, match=rf"step 1 needs {peak} rows, more than max_rows = {peak - 1}"):
            g.motif(3, terms, max_rows=peak - 1)
        with pytest.raises(ValueError, match=rf"step 1 needs {peak} rows"):
            g.motif(3, terms, max_rows=dgr + 1, count_only=True)
        with pytest.raises(ValueError, match=rf"step 0 needs {dgr + 1} rows"):
            g.motif(3, terms, max_rows=dgr)
        assert g.motif(3, terms, max_rows=peak, count_only=True) == 1
        # the handle works as before
        F = np.zeros(V, bool)
        T = np.zeros(V, bool)
        F[0], T[2] = True, True
        assert g.bfs(F, T)[0] == 1
        again, _ = g.motif(3, terms)
        assert all(np.array_equal(again[i], vcols[i]) for i in range(3))
    gf = gfa.GraphFrame(pd.DataFrame({"id": np.arange(V)}), pd.DataFrame({"src": s, "dst": d}))
    try:
        pattern = "(a)-[]->(b); (a)-[]->(c); (b)-[]->(c)"
        assert len(gf.find(pattern, maxRows=peak)) == 1
        with pytest.raises(ValueError, match=rf"step 1 needs {peak} rows"):
            gf.find(pattern, maxRows=peak - 1)
    finally:
        gf.close()


# ---- 9. determinism and invariance ----
def test_determinism_and_invariance(gfa):
    V, s, d = random_multigraph(500, 6000, 31)
    parsed = gfa.parse_motif("(a)-[e]->(b); (b)-[e2]->(c); (a)-[e3]->(c)")
    plan = gfa.plan_motif(parsed)
    columns = motif_ref.spec(parsed)[2]
    with gfa.Graph(s, d, V) as g, gfa.Graph(s, d, V) as h:
        lab = g.run(3)
        first = run_plan(g, parsed, plan)
        assert np.array_equal(g.labels(), lab)
        assert np.array_equal(g.run(3), lab)
        for other in (run_plan(g, parsed, plan), run_plan(h, parsed, plan)):
            for mine, theirs in zip(first, other):
                assert mine.keys() == theirs.keys()
                assert all(mine[k].tobytes() == theirs[k].tobytes() for k in mine)
    assert first[0][0].size > 0
    perm = np.random.default_rng(2).permutation(s.size)     # new row j holds old row perm[j]
    with gfa.Graph(s[perm], d[perm], V) as g:
        vcols, ecols = run_plan(g, parsed, plan)
    mapped = {k: perm[col] for k, col in ecols.items()}
    assert motif_ref.rows_of(vcols, mapped, columns) == motif_ref.rows_of(first[0], first[1], columns)


# ---- 10. drop-in ----
def test_drop_in(gfa):
    v = pd.DataFrame({"id": ["u", "v", "w", "x", "u"], "kind": [1, 2, 3, 4, 5]})
    e = pd.DataFrame({"src": ["u", "v", "u", "q", "w", "v"], "dst": ["v", "u", "w", "u", "w", "u"],
                      "weight": [10, 20, 30, 40, 50, 60]})
    gf = gfa.GraphFrame(v, e)
    try:
        m = gf.find(RECIPROCAL)
        assert list(m.columns) == [("a", "id"), ("a", "kind"), ("e", "src"), ("e", "dst"), ("e", "weight"),
                                   ("b", "id"), ("b", "kind"), ("e2", "src"), ("e2", "dst"), ("e2", "weight")]
        assert m["a"]["id"].tolist() == ["u", "u", "v", "v", "w"] and m["a"]["kind"].tolist() == [1, 1, 2, 2, 3]
        assert m["b"]["id"].tolist() == ["v", "v", "u", "u", "w"]
        assert m["e"]["weight"].tolist() == [10, 10, 20, 60, 50]
        assert m["e2"]["weight"].tolist() == [20, 60, 10, 10, 50]
        assert (m["e"]["src"] == m["a"]["id"]).all() and (m["e2"]["dst"] == m["a"]["id"]).all()
        assert m.attrs == {"rows": 5, "plan": ["(a)-[e]->(b)", "(b)-[e2]->(a)"]}
        assert gf.motifCount(RECIPROCAL) == 5
        assert len(m[m["a"]["id"] != m["b"]["id"]]) == 4        # the usual post-filter
        # anonymous elements multiply rows and have no columns
        anon = gf.find("(a)-[]->()")
        assert list(anon.columns) == [("a", "id"), ("a", "kind")] and anon["a"]["id"].tolist() == ["u", "u", "v", "v", "w"]
        # the vertices, the first row of a repeated id
        only = gf.find("(a)")
        assert only["a"]["id"].tolist() == ["u", "v", "w", "x"] and only["a"]["kind"].tolist() == [1, 2, 3, 4]
        # an empty result keeps its columns
        none = gf.find("(a)-[e]->(b); !(a)-[]->(b)")
        assert len(none) == 0 and none.attrs["rows"] == 0
        assert list(none.columns) == [("a", "id"), ("a", "kind"), ("e", "src"), ("e", "dst"), ("e", "weight"),
                                      ("b", "id"), ("b", "kind")]
        assert gf.motifCount("(a)-[e]->(b); !(a)-[]->(b)") == 0
    finally:
        gf.close()
    assert gfa.find(v, e, RECIPROCAL).equals(m)
    assert gfa.motif_count(v, e, RECIPROCAL) == 5 and gfa.motif_count(v, e, "(a)") == 4
