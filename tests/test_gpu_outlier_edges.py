"""The outlier stage (lpa_outlier / lpa_outlier_device) at its engineered edges.

The threshold rule is one strict comparison at one index of a sorted order (k_seg_threshold:
k = n // 10, the k-th smallest size or the largest when k == 0, flag iff size < thr), the
L2 sub-graph runs a schedule of its own (build_graph_l2: rows unsorted, out-edges before
in-edges, every refresh a rebuild, no frontier, no captured graphs), and BlockHist's
overflow path is reached only by chance on organic labels.  tests/graphs.py outlier_groups
chooses the communities directly as an input labelling, each a disjoint union of cliques of
prescribed sizes plus lone vertices, so every community's multiset of sub-group sizes, its
threshold and its flagged groups are known in closed form.  The oracle is first checked
against the closed form and a numpy restatement on the CPU (module fixture `fx`, so no case
passes vacuously); then every GPU result is compared bit-exactly (integers, no tolerance).

Measured on the fixture (oracle and numpy; the fixture `fx` asserts them):
  V 8,192 (7,674 catalogue vertices + 518 edgeless padding vertices as one more community)
  5,394,169 edges, 5,386,169 of them distinct and inside a community (E'), 4,500 distinct
  edges between communities, 3,500 duplicates, 10 self-loops, 13 label-swapping pairs
  sub-groups per community: 1, 1, 2, 9, 9, 10, 10, 10, 11, 19, 20, 20, 20, 20, 21, 29, 30,
  31, 100, 100, 100, 100 and 518 (the padding); 1,191 sub-groups in all
  mode L2, sub_iter >= 2: 86 vertices flagged in 10 communities
  mode L2, sub_iter = 1: 1,818 sub-groups, 3 vertices flagged in 2 communities (oracle only)
  E' degrees (arcs per row of the sub-graph): 541 rows of 0, 26 of 1, 222 of 2, 1,148 in
  (2, 4], 964 in (4, 8], 55 in (8, 16], 68 in (16, 32], 101 in (32, 64], 66 in (64, 128],
  386 in (128, 256], 901 in (256, 512], 514 in (512, 1024], 1,100 in (1024, 4096] (1,099
  arcs each), 2,100 above 4,096 (4,198 arcs each)

Not reached by this file: an L2 arena of more than one 256 MB block; the second LPA's
giant-code refresh and settles on engineered ties (they need a sub-graph of >= 4 M slots:
only the R-MAT-22 case runs them, on organic labels, at sub_iter 1, 2, 3 here and 4 in
test_gpu_parity.py).  The size sort's top bit (a community of V = 2^13 members) cannot
decide anything: a group of V members is the only group of its segment.
"""
import ctypes

import numpy as np
import pytest

from graphs import (adversarial_hub, bh_home_slot, bh_saturating_labels, coarse_family, coarse_labels, degree_mix,
                    giant_hub, outlier_groups, outlier_l1_np, random_multigraph, star, sub_edges)

pytestmark = pytest.mark.gpu

SUB_ITERS = (1, 2, 3, 4, 5, 6, 7, 8, 12)
FIXTURE_V = 8192
DEGREE_BINS = (0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 4096, 1 << 30)
COARSE = coarse_family(FIXTURE_V)


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


class Fx:
    pass


@pytest.fixture(scope="module")
def fx(oracle):
    """The fixture, the oracle's results and the CPU preconditions, once per module."""
    x = Fx()
    f = x.f = outlier_groups()
    V = f.V
    assert V == FIXTURE_V and V & (V - 1) == 0
    assert (f.labels == V - 1).any()
    assert {len(sz) for sz in f.sizes} >= {1, 2, 9, 10, 11, 19, 20, 21, 29, 30, 31, 100}
    x.flags, x.summ = f.closed_form()
    assert (x.summ["n_flagged"], x.summ["n_communities_flagged"]) == (86, 10)
    x.l2 = {}
    for t in SUB_ITERS:
        sub, fl, sm = oracle.outlier_l2(V, f.src, f.dst, f.labels, t)
        if t >= 2:
            assert np.array_equal(sub, f.sub_labels(t)), t
            assert np.array_equal(fl, x.flags) and sm == x.summ, (t, sm)
        for a in (sub, fl):
            a.setflags(write=False)
        x.l2[t] = (sub, fl, sm)
    assert x.l2[1][2]["n_subgroups"] > x.summ["n_subgroups"]     # superstep 1 alone is another answer
    x.l1 = outlier_l1_np(V, f.src, f.dst, f.labels)
    size, inc, fl1, s1 = oracle.outlier_l1(V, f.src, f.dst, f.labels)
    assert np.array_equal(size, x.l1[0]) and np.array_equal(inc, x.l1[1])
    assert np.array_equal(fl1, x.l1[2]) and s1 == x.l1[3]
    # the sub-graph has rows in every degree bin (an independent degree count of E')
    ds, dd = sub_edges(f.src, f.dst, f.labels, V)
    deg = np.bincount(ds, minlength=V) + np.bincount(dd, minlength=V)
    assert (deg == 0).sum() > 0
    for lo, hi in zip(DEGREE_BINS, DEGREE_BINS[1:]):
        assert ((deg > lo) & (deg <= hi)).sum() > 0, (lo, hi)
    assert deg.max() > 4096 and ((deg > 1024) & (deg <= 4096)).sum() >= 1000
    key = x.key = np.unique(f.src.astype(np.int64) * V + f.dst)
    x.ks, x.kd = (key // V).astype(np.int32), (key % V).astype(np.int32)   # the distinct edges
    assert key.size - ds.size >= 4000                              # edges between communities
    assert f.src.size - key.size >= 3000 and int((ds == dd).sum()) >= 10   # duplicates, self-loops
    return x


@pytest.fixture(scope="module")
def fx_graph(gfa, fx):
    with gfa.Graph(fx.f.src, fx.f.dst, fx.f.V) as g:
        yield g


def _l2_summary(o):
    s = o["summary"]
    return dict(n_communities=s["n_communities"], n_subgroups=s["n_groups"], n_flagged=s["n_flagged"],
                n_communities_flagged=s["n_communities_flagged"])


def _l1_summary(o):
    s = o["summary"]
    return dict(n_groups=s["n_groups"], k=s["k"], thr=s["threshold"], n_flagged=s["n_flagged"])


def _same_on_device(dv, h):
    assert dv["summary"] == h["summary"]
    for k in ("size", "incident", "flags", "sub_labels"):
        if h[k] is None:
            assert dv[k] is None
        else:
            assert np.array_equal(dv[k].cpu().numpy(), h[k]), k


def _check_l1(o, V, s, d, lab, oracle, what="", key=None):
    size, inc, flags, summ = outlier_l1_np(V, s, d, lab, key)
    assert np.array_equal(o["size"], size), what
    assert np.array_equal(o["incident"], inc), what
    assert np.array_equal(o["flags"], flags), what
    assert _l1_summary(o) == summ, what
    osize, oinc, oflags, osumm = oracle.outlier_l1(V, s, d, lab)
    assert np.array_equal(o["size"], osize) and np.array_equal(o["incident"], oinc), what
    assert np.array_equal(o["flags"], oflags) and _l1_summary(o) == osumm, what
    assert o["summary"]["n_communities"] == summ["n_groups"], what


def _check_l2(o, V, s, d, lab, t, oracle, what=""):
    sub, flags, summ = oracle.outlier_l2(V, s, d, lab, t)
    assert np.array_equal(o["sub_labels"], sub), (what, int((o["sub_labels"] != sub).sum()))
    assert np.array_equal(o["flags"], flags), what
    assert _l2_summary(o) == summ, what
    size, inc, _, _ = outlier_l1_np(V, s, d, lab)
    assert np.array_equal(o["size"], size) and np.array_equal(o["incident"], inc), what


# ---- a. mode L2 on the fixture ----
def test_l2_fixture_every_sub_iter(fx, fx_graph):
    """sub_iter 1..8 and 12 on one handle: sub-labels, flags and summary against the oracle,
    from sub_iter 2 on against the closed form too; host form equal to the device form."""
    import torch

    f, g = fx.f, fx_graph
    dl = torch.from_numpy(f.labels).cuda()
    for t in SUB_ITERS:
        o = g.outlier(f.labels, "L2", sub_iter=t)
        sub, flags, summ = fx.l2[t]
        bad = np.flatnonzero(o["sub_labels"] != sub)
        assert bad.size == 0, f"sub_iter {t}: {bad.size} sub-labels differ, first {bad[:5].tolist()} " \
                              f"in communities {[f.names[c] for c in f.comm[bad[:5]]]}"
        assert np.array_equal(o["flags"], flags), t
        assert _l2_summary(o) == summ, t
        if t >= 2:
            assert np.array_equal(o["sub_labels"], f.sub_labels(t)), t
            assert np.array_equal(o["flags"], fx.flags) and _l2_summary(o) == fx.summ, t
        assert np.array_equal(o["size"], fx.l1[0]) and np.array_equal(o["incident"], fx.l1[1]), t
        assert o["summary"]["distinct_edges"] == fx.key.size
        _same_on_device(g.outlier(dl, "L2", sub_iter=t), o)


# ---- b. mode L1's decision edges on the same handle ----
def test_l1_fixture_labelling(fx, fx_graph, oracle):
    import torch

    f = fx.f
    o = fx_graph.outlier(f.labels, "L1")
    _check_l1(o, f.V, f.src, f.dst, f.labels, oracle)
    assert o["summary"]["n_groups"] == len(f.sizes)
    _same_on_device(fx_graph.outlier(torch.from_numpy(f.labels).cuda(), "L1"), o)


@pytest.mark.parametrize("case", COARSE, ids=[c[0] for c in COARSE])
def test_l1_group_count_and_ties_at_k(fx, fx_graph, oracle, case):
    """n_groups on both sides of every multiple of 10 in reach, the sizes around position k
    tied or one apart: the hand-written summary, the numpy restatement and the oracle (both
    on the fixture's distinct edges, which `fx` has checked the oracle's own deduplication on).
    n1_all_one: one community of V = 2^13 members -- the size needs the sort's top bit."""
    name, sizes, want = case
    f = fx.f
    lab = coarse_labels(f, sizes)
    o = fx_graph.outlier(lab, "L1")
    assert _l1_summary(o) == want, name
    assert np.array_equal(np.sort(o["size"][o["size"] > 0]), np.sort(sizes)), name
    _check_l1(o, f.V, fx.ks, fx.kd, lab, oracle, name, fx.key)


def test_l1_every_label_in_use(fx, fx_graph, oracle):
    """labels = arange(V): V groups of one, no empty label (no sentinel segment behind the
    groups in the sorted keys), thr = 1, nothing flagged; in both orders of the ids."""
    import torch

    f = fx.f
    for lab in (np.arange(f.V, dtype=np.int32), np.arange(f.V, dtype=np.int32)[::-1].copy()):
        o = fx_graph.outlier(lab, "L1")
        assert _l1_summary(o) == dict(n_groups=f.V, k=f.V // 10, thr=1, n_flagged=0)
        assert (o["size"] == 1).all() and not o["flags"].any()
        _check_l1(o, f.V, fx.ks, fx.kd, lab, oracle, key=fx.key)
        _same_on_device(fx_graph.outlier(torch.from_numpy(lab).cuda(), "L1"), o)


# ---- c. per-superstep parity of the sub-graph's own schedule ----
PARITY_STEPS = 6


def _parity_graph(name, oracle):
    if name == "degree_mix":
        return degree_mix(4)
    if name == "giant_hub":
        return giant_hub()
    if name == "adversarial_hub":
        return adversarial_hub()
    if name == "star300":
        return star(300)
    s, d = oracle.gen_rmat(16, 16, seed=5)
    return 1 << 16, s, d


@pytest.mark.parametrize("split", ["one_community", "two_communities"])
@pytest.mark.parametrize("name", ["degree_mix", "giant_hub", "adversarial_hub", "star300", "rmat16"])
def test_l2_sub_graph_per_superstep(gfa, oracle, name, split):
    """Labels constant over all vertices: E' is every distinct edge and the second LPA is
    LPA on the deduplicated directed graph; two communities: the E' filter matters (the hub
    keeps seven eighths of its neighbours).  sub_iter = t against superstep t of the oracle's
    LPA on the numpy-filtered edge list, t = 1..6; the hub rows (bucketed combine, sub-bucket
    passes, spill) are tallied from rows in run order.  star: period 2."""
    V, s, d = _parity_graph(name, oracle)
    if split == "one_community":
        lab = np.full(V, V // 2, np.int32)
    else:
        lab = np.where(np.arange(V) % 8 == 7, V - 1, 3 % V).astype(np.int32)
    ds, dd = sub_edges(s, d, lab, V)
    assert 0 < ds.size < s.size or name == "star300"
    _, hist, _ = oracle.lpa(V, ds, dd, PARITY_STEPS, per_iter=True)
    if name.endswith("hub"):
        deg = np.bincount(ds, minlength=V) + np.bincount(dd, minlength=V)
        assert deg[0] > 8192 and np.unique(dd[ds == 0]).size == deg[0]    # one row of distinct arcs
    with gfa.Graph(s, d, V) as g:
        for t in range(1, PARITY_STEPS + 1):
            got = g.outlier(lab, "L2", sub_iter=t)["sub_labels"]
            bad = np.flatnonzero(got != hist[t - 1])
            assert bad.size == 0, f"{name} {split} sub_iter {t}: {bad.size} differ, first {bad[:5].tolist()}"
        if name == "star300":
            two = g.outlier(lab, "L2", sub_iter=2)
            twelve = g.outlier(lab, "L2", sub_iter=12)
            assert np.array_equal(twelve["sub_labels"], two["sub_labels"])
            assert np.array_equal(twelve["flags"], two["flags"]) and twelve["summary"] == two["summary"]
            assert not np.array_equal(two["sub_labels"], hist[0])


def test_l2_rmat22_first_supersteps(gfa, oracle):
    """The inputs of test_gpu_parity.py's rmat22_codes case (a sub-graph of >= 4 M slots: the
    second LPA takes the giant-code refresh after its superstep 1 and settles rows from codes
    in supersteps 2 and 3), which compares sub_iter 4 only: sub_iter 1, 2 and 3 against the
    oracle's per-superstep history on the numpy-filtered edge list."""
    ts, td = gfa.gen_rmat(22, 16, seed=9)
    V, s, d = 1 << 22, ts.cpu().numpy(), td.cpu().numpy()
    with gfa.Graph(ts, td, V) as g:
        lab = g.run(10)
        got = [g.outlier(lab, "L2", sub_iter=t)["sub_labels"] for t in (1, 2, 3)]
    ds, dd = sub_edges(s, d, lab, V)
    _, hist, _ = oracle.lpa(V, ds, dd, 3, per_iter=True)
    # measured: E' holds 65,236,697 edges; 2.39 M, 2.38 M and 2.12 M labels change in supersteps 1-3
    assert ds.size > 60_000_000
    prev = np.arange(V)
    for t in (1, 2, 3):
        assert int((hist[t - 1] != prev).sum()) > 1_000_000, t
        prev = hist[t - 1]
    for t in (1, 2, 3):
        bad = int((got[t - 1] != hist[t - 1]).sum())
        assert bad == 0, f"sub_iter {t}: {bad} sub-labels differ"


# ---- d. BlockHist saturation, engineered ----
def test_blockhist_overflow(gfa, oracle):
    """>= 12 labels of one BlockHist home slot inside one block's 256-element stretch of
    k_histogram (element = vertex) and of k_incident (element = distinct edge: a ring, so
    edge i starts at vertex i), more than the 8 probes reach: the overflow path (direct
    device atomics) and, after it, home-slot-only probing run whatever the thread order."""
    lab, coll, heavy = bh_saturating_labels()
    V = lab.size
    assert V == 65536 and coll.size >= 12 and np.unique(bh_home_slot(np.append(coll, heavy))).size == 1
    ring = np.arange(V, dtype=np.int32)
    dup = np.arange(0, V, 7, dtype=np.int32)                      # duplicates: same distinct edges
    s = np.concatenate([ring, dup])
    d = np.concatenate([(ring + 1) % V, (dup + 1) % V]).astype(np.int32)
    key = np.unique(s.astype(np.int64) * V + d)
    assert key.size == V and np.array_equal(key // V, ring)       # distinct edge i starts at vertex i
    with gfa.Graph(s, d, V) as g:
        o1 = g.outlier(lab, "L1")
        o2 = g.outlier(lab, "L2", sub_iter=3)
    _check_l1(o1, V, s, d, lab, oracle)
    assert (o1["size"][coll] >= 2).all() and o1["size"][heavy] >= 6 * 256
    _check_l2(o2, V, s, d, lab, 3, oracle)
    assert o2["summary"]["n_groups"] < V                            # the heavy stretch is a path in E'


# ---- e. edge inputs ----
def test_edgeless_graph(gfa, oracle):
    none = np.zeros(0, np.int32)
    with gfa.Graph(none, none, 4) as g:
        for lab in ([0, 1, 2, 3], [2, 2, 2, 2], [3, 0, 0, 3]):
            lab = np.array(lab, np.int32)
            o1 = g.outlier(lab, "L1")
            _check_l1(o1, 4, none, none, lab, oracle)
            assert not o1["incident"].any() and o1["summary"]["distinct_edges"] == 0
            for t in (1, 5):
                o2 = g.outlier(lab, "L2", sub_iter=t)
                _check_l2(o2, 4, none, none, lab, t, oracle)
                assert o2["sub_labels"].tolist() == [0, 1, 2, 3]
    # [2, 2, 2, 2] in L2: 4 sub-groups of one in one community, k = 0, thr = 1, none flagged


@pytest.mark.parametrize("loop", [False, True])
def test_single_vertex(gfa, oracle, loop):
    e = np.zeros(1 if loop else 0, np.int32)
    lab = np.zeros(1, np.int32)
    with gfa.Graph(e, e, 1) as g:
        o1 = g.outlier(lab, "L1")
        _check_l1(o1, 1, e, e, lab, oracle)
        assert _l1_summary(o1) == dict(n_groups=1, k=0, thr=1, n_flagged=0)
        assert o1["incident"].tolist() == [int(loop)]
        o2 = g.outlier(lab, "L2", sub_iter=2)
        _check_l2(o2, 1, e, e, lab, 2, oracle)
        assert o2["sub_labels"].tolist() == [0] and not o2["flags"].any()


def test_empty_sub_graph(gfa, oracle):
    """All-distinct labels and no self-loop: E' is empty (the graph itself is not)."""
    V, s, d = random_multigraph(5000, 20000, 12)
    keep = s != d
    s, d = s[keep], d[keep]
    lab = np.arange(V, dtype=np.int32)
    assert sub_edges(s, d, lab, V)[0].size == 0
    with gfa.Graph(s, d, V) as g:
        o1 = g.outlier(lab, "L1")
        o2 = g.outlier(lab, "L2", sub_iter=5)
    _check_l1(o1, V, s, d, lab, oracle)
    _check_l2(o2, V, s, d, lab, 5, oracle)
    assert np.array_equal(o2["sub_labels"], lab) and not o2["flags"].any() and not o1["flags"].any()
    assert o1["summary"]["n_groups"] == V and o2["summary"]["n_groups"] == V


OUTPUTS = ("size", "incident", "sub_labels", "flags", "summary")


def _raw_outlier(g, lab, mode, sub_iter, want):
    """lpa_outlier through ctypes with only the outputs in `want` given, the others NULL."""
    from graphframes_amd import _lib

    V = g.num_vertices
    size = np.full(V, -7, np.int64)
    inc = np.full(V, -7, np.int64)
    sub = np.full(V, -7, np.int32)
    flags = np.full(V, 7, np.uint8)
    summ = _lib.LpaOutlierSummary()
    i64p = ctypes.POINTER(ctypes.c_int64)
    rc = g._lib.lpa_outlier(
        g._handle(), lab.ctypes.data, 0, mode, sub_iter,
        size.ctypes.data_as(i64p) if "size" in want else None,
        inc.ctypes.data_as(i64p) if "incident" in want else None,
        sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if "sub_labels" in want else None,
        flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if "flags" in want else None,
        ctypes.byref(summ) if "summary" in want else None)
    _lib.check(rc)
    return dict(size=size, incident=inc, sub_labels=sub, flags=flags, summary=summ.to_dict())


@pytest.mark.parametrize("mode", [1, 2])
def test_omitted_outputs(gfa, oracle, mode):
    """Every output pointer NULL in turn, and all of them but the summary: the outputs that
    are given, and the summary, are those of the call with every output."""
    V, s, d = degree_mix(9, hubs=(700, 1500), n_low=1500, extra=6000)
    with gfa.Graph(s, d, V) as g:
        lab = g.run(3)
        full = _raw_outlier(g, lab, mode, 4, OUTPUTS)
        if mode == 1:
            _check_l1(dict(full, flags=full["flags"].astype(bool)), V, s, d, lab, oracle)
            assert (full["sub_labels"] == -7).all()                 # L1 writes no sub-labels
        else:
            _check_l2(dict(full, flags=full["flags"].astype(bool)), V, s, d, lab, 4, oracle)
        for want in [tuple(o for o in OUTPUTS if o != out) for out in OUTPUTS] + [("summary",)]:
            got = _raw_outlier(g, lab, mode, 4, want)
            for k in want:
                if k == "summary":
                    assert got[k] == full[k], want
                else:
                    assert np.array_equal(got[k], full[k]), (want, k)
            for k in set(OUTPUTS) - set(want) - {"summary"}:
                assert (got[k] == (7 if k == "flags" else -7)).all(), (want, k)


# ---- f. one handle, many calls ----
def test_one_handle_many_calls(gfa, oracle):
    """20 alternating L1 / L2 calls on one handle, E' going empty, full, small and empty
    again (cached distinct edges and transposed order, the sub-graph arena reset by every
    L2 call): each result equals a fresh handle's, and the handle's device memory does not
    grow after the call with the largest sub-graph."""
    V, s, d = degree_mix(3)
    keep = s != d
    s, d = s[keep], d[keep]
    labs = dict(empty=np.arange(V, dtype=np.int32), full=np.full(V, V - 1, np.int32),
                small=(np.arange(V) % 50).astype(np.int32))
    assert sub_edges(s, d, labs["empty"], V)[0].size == 0
    n_full = sub_edges(s, d, labs["full"], V)[0].size
    assert 0 < sub_edges(s, d, labs["small"], V)[0].size < n_full // 20
    plan = [("empty", "L2", 5), ("empty", "L1", 0), ("full", "L1", 0), ("full", "L2", 5), ("small", "L1", 0),
            ("small", "L2", 3), ("empty", "L2", 3), ("full", "L2", 3), ("empty", "L1", 0), ("small", "L2", 5),
            ("full", "L1", 0), ("empty", "L2", 5), ("small", "L1", 0), ("full", "L2", 5), ("small", "L2", 3),
            ("empty", "L1", 0), ("empty", "L2", 3), ("full", "L2", 3), ("small", "L1", 0), ("empty", "L2", 5)]
    fresh = {}
    for key in dict.fromkeys(plan):
        with gfa.Graph(s, d, V) as g:
            fresh[key] = g.outlier(labs[key[0]], key[1], sub_iter=max(key[2], 1))
        if key[1] == "L1":
            _check_l1(fresh[key], V, s, d, labs[key[0]], oracle, key)
        else:
            _check_l2(fresh[key], V, s, d, labs[key[0]], key[2], oracle, key)
    with gfa.Graph(s, d, V) as g:
        nbytes = []
        for key in plan:
            o = g.outlier(labs[key[0]], key[1], sub_iter=max(key[2], 1))
            ref = fresh[key]
            assert o["summary"] == ref["summary"], key
            for k in ("size", "incident", "flags", "sub_labels"):
                assert (o[k] is None and ref[k] is None) or np.array_equal(o[k], ref[k]), (key, k)
            nbytes.append(g.info()["device_bytes"])
    largest = plan.index(("full", "L2", 5))
    assert nbytes[-1] <= nbytes[largest], nbytes
    assert all(b == nbytes[largest] for b in nbytes[largest:]), nbytes
