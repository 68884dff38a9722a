"""CPU oracle pinning (no GPU): the C restatement vs the pure-Python one, the
upstream-suite-shaped known answers, and the facts of the reference's own
sample data (R9, /root/reference/CommunityDetection/data, restated per
Graphframes.py:16-73 into tests/golden/r9_golden.npz by make_golden.py)."""
import numpy as np
import pytest

from graphs import (bh_home_slot, bh_saturating_labels, coarse_family, coarse_labels, degree_mix, outlier_groups,
                    outlier_l1_np, random_multigraph, star, threshold_of, two_cliques)


def test_two_cliques_kat(oracle):
    V, s, d = two_cliques()
    lab = oracle.lpa(V, s, d, 20)
    # upstream LabelPropagationSuite: each clique one label, the two labels differ;
    # min-tie answer computed at survey time
    assert lab.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5, 5, 5]
    assert oracle.lpa_py(V, list(zip(s, d)), 20) == lab.tolist()


def test_star_period_two(oracle):
    V, s, d = star(10)
    _, hist, _ = oracle.lpa(V, s, d, 4, per_iter=True)
    assert hist[0][0] == 1 and (hist[0][1:] == 0).all()
    assert hist[1][0] == 0 and (hist[1][1:] == 1).all()
    assert np.array_equal(hist[2], hist[0])


def test_votes_semantics(oracle):
    # self-loop (u,u) = 2 votes for L[u]; duplicates counted; isolated keep label
    V = 5
    s = np.array([1, 1, 1, 3], np.int32)
    d = np.array([1, 0, 2, 4], np.int32)
    lab = oracle.lpa(V, s, d, 1)
    assert lab[1] == 1          # 2 votes for own label beat 1 each for 0 and 2
    assert lab[0] == 1 and lab[2] == 1
    assert lab[3] == 4 and lab[4] == 3
    s = np.array([0, 0, 0], np.int32)
    d = np.array([2, 2, 1], np.int32)
    assert oracle.lpa(3, s, d, 1)[0] == 2   # duplicate edge = 2 votes


def test_max_iter_must_be_positive(oracle):
    with pytest.raises(ValueError, match="greater than 0"):
        oracle.lpa(3, np.array([0], np.int32), np.array([1], np.int32), 0)
    with pytest.raises(ValueError):
        oracle.lpa_py(3, [(0, 1)], -1)


@pytest.mark.parametrize("V,m,seed", [(7, 20, 0), (30, 100, 1), (60, 400, 2), (200, 300, 3)])
def test_c_matches_python(oracle, V, m, seed):
    V, s, d = random_multigraph(V, m, seed)
    for it in (1, 2, 5):
        assert oracle.lpa(V, s, d, it).tolist() == oracle.lpa_py(V, list(zip(s.tolist(), d.tolist())), it)


def test_outlier_l1_matches_python(oracle):
    V, s, d = random_multigraph(300, 500, 9)
    lab = oracle.lpa(V, s, d, 3)
    size, inc, flags, summ = oracle.outlier_l1(V, s, d, lab)
    psize, pinc, pflags, pthr = oracle.outlier_l1_py(V, list(zip(s.tolist(), d.tolist())), lab.tolist())
    assert summ["thr"] == pthr
    assert flags.tolist() == pflags
    assert all(size[l] == c for l, c in psize.items()) and size.sum() == V
    assert all(inc[l] == c for l, c in pinc.items())


@pytest.mark.parametrize("labels", ["lpa", "arbitrary"])
@pytest.mark.parametrize("V,m,seed", [(1, 3, 0), (12, 30, 1), (40, 160, 2), (90, 500, 3), (200, 320, 4)])
def test_outlier_l2_matches_python(oracle, V, m, seed, labels):
    """The C oracle's mode L2 against its literal Counter restatement (outlier_l2_py): small
    random multigraphs (duplicates, self-loops, reciprocal pairs), LPA labels and arbitrary
    ones (a few communities, label values anywhere in [0, V))."""
    V, s, d = random_multigraph(V, m, seed)
    s, d = np.concatenate([s, d[: m // 4]]), np.concatenate([d, s[: m // 4]])   # reciprocal pairs
    rng = np.random.default_rng(seed)
    lab = oracle.lpa(V, s, d, 2) if labels == "lpa" else \
        rng.integers(0, V, size=max(V // 8, 1))[rng.integers(0, max(V // 8, 1), size=V)].astype(np.int32)
    edges = list(zip(s.tolist(), d.tolist()))
    for it in (1, 2, 3, 5, 8):
        sub, flags, summ = oracle.outlier_l2(V, s, d, lab, it)
        psub, pflags, psumm = oracle.outlier_l2_py(V, edges, lab.tolist(), it)
        assert sub.tolist() == psub, it
        assert flags.tolist() == pflags, it
        assert summ == psumm, it


def test_threshold_rule_lst_minus_zero(oracle):
    # n < 10 groups -> k = 0 -> lst[-0] == lst[0] = the LARGEST size (Graphframes.py:136)
    assert oracle.threshold_rule_py({1: 5, 2: 3, 3: 1}) == 5
    sizes = {i: i for i in range(1, 21)}   # n = 20 -> k = 2 -> 2nd smallest
    assert oracle.threshold_rule_py(sizes) == 2


# (sizes in ascending order, threshold, groups flagged): ties around position k = n // 10
THRESHOLD_CASES = [
    ([1, 2, 3, 4, 5, 6, 7, 8, 9], 9, 8),                 # n = 9: k = 0, the largest
    ([4] * 9, 4, 0),
    ([2] + [3] * 9, 2, 0),                               # n = 10: k = 1, the smallest; nothing is below it
    ([2, 2] + [3] * 8, 2, 0),
    ([5] * 10, 5, 0),
    ([1] + [3] * 10, 1, 0),                              # n = 11
    ([1, 1] + [3] * 17, 1, 0),                           # n = 19: still k = 1
    ([1, 3] + [4] * 18, 3, 1),                           # n = 20: k = 2, smallest < 2nd
    ([1, 1] + [4] * 18, 1, 0),                           # smallest = 2nd
    ([1, 3, 3] + [4] * 17, 3, 1),                        # 2nd = 3rd
    ([7] * 20, 7, 0),
    ([1, 3, 3] + [4] * 18, 3, 1),                        # n = 21: k = 2
    ([1] * 7 + [3] * 6 + [4] * 87, 3, 7),                # n = 100: k = 10, positions 8..13 tied
    ([1] * 5 + [3] * 5 + [4] * 90, 3, 5),                # the run ends at position k
    ([1] * 10 + [3] * 6 + [4] * 84, 1, 0),               # the run starts at position k + 1
    ([1] * 9 + [3] * 91, 3, 9),                          # position k opens the run
]


@pytest.mark.parametrize("sizes,thr,n_flagged_groups", THRESHOLD_CASES,
                         ids=[f"n{len(c[0])}_{i}" for i, c in enumerate(THRESHOLD_CASES)])
def test_threshold_rule_ties_around_k(oracle, sizes, thr, n_flagged_groups):
    """Hand-written thresholds at n = 9, 10, 11, 19, 20, 21, 100 with tied sizes around
    position k: the Python rule, the numpy restatement of the tests, and the C oracle (an
    edgeless graph whose labelling has exactly these group sizes, in shuffled order)."""
    n = len(sizes)
    rng = np.random.default_rng(n)
    shuffled = rng.permutation(sizes)
    assert oracle.threshold_rule_py({100 + i: int(c) for i, c in enumerate(shuffled)}) == thr
    assert threshold_of(shuffled) == thr
    V = int(sum(sizes))
    lab = np.repeat(np.cumsum(shuffled) - 1, shuffled).astype(np.int32)   # label = the group's last vertex
    none = np.zeros(0, np.int32)
    size, inc, flags, summ = oracle.outlier_l1(V, none, none, lab)
    assert (summ["n_groups"], summ["k"], summ["thr"]) == (n, n // 10, thr)
    assert np.array_equal(flags, size[lab] < thr)
    assert np.unique(lab[flags]).size == n_flagged_groups
    assert summ["n_flagged"] == sum(c for c in sizes if c < thr)


def test_outlier_groups_fixture_closed_form(oracle):
    """tests/graphs.py outlier_groups at CPU size (the cliques above 300 shrunk): the
    oracle's mode L2 reproduces the closed-form sub-labels, flags and summary at
    sub_iter 2, 3, 4, 5 and 8; its mode L1 equals the numpy restatement."""
    f = outlier_groups(big=False)
    assert f.V == 4096 and (f.labels == f.V - 1).any()
    assert {len(sz) for sz in f.sizes} >= {1, 2, 9, 10, 11, 19, 20, 21, 29, 30, 31, 100}
    flags, summ = f.closed_form()
    assert (summ["n_flagged"], summ["n_communities_flagged"]) == (86, 10)
    for it in (2, 3, 4, 5, 8):
        sub, fl, sm = oracle.outlier_l2(f.V, f.src, f.dst, f.labels, it)
        assert np.array_equal(sub, f.sub_labels(it)), it
        assert np.array_equal(fl, flags) and sm == summ, it
    size, inc, fl1, s1 = oracle.outlier_l1(f.V, f.src, f.dst, f.labels)
    nsize, ninc, nfl, ns1 = outlier_l1_np(f.V, f.src, f.dst, f.labels)
    assert np.array_equal(size, nsize) and np.array_equal(inc, ninc) and np.array_equal(fl1, nfl) and s1 == ns1
    # every member of a community shares its label, which is one of the members
    assert np.array_equal(f.comm[f.labels], f.comm)


def test_coarse_family_is_what_it_says(oracle):
    """coarse_family's hand-written (n_groups, k, thr, n_flagged) against the oracle and the
    numpy restatement on the labellings coarse_labels makes of them."""
    f = outlier_groups(big=False)
    seen = set()
    for name, sizes, want in coarse_family(f.V):
        lab = coarse_labels(f, sizes)
        _, _, _, summ = oracle.outlier_l1(f.V, f.src, f.dst, lab)
        assert summ == want, name
        assert outlier_l1_np(f.V, f.src, f.dst, lab)[3] == want, name
        seen.add(want["n_groups"])
    assert seen == {1, 9, 10, 11, 19, 20, 21, 99, 100, 101}


def test_bh_saturating_labels():
    """The BlockHist overflow fixture: >= 12 labels of one home slot in one 256-element
    stretch (more than the 8 probes reach), the heavy label of the same slot after them."""
    lab, coll, heavy = bh_saturating_labels()
    slots = bh_home_slot(np.append(coll, heavy))
    assert coll.size >= 12 and np.unique(coll).size == coll.size and (slots == slots[0]).all()
    stretch = lab[256 * 37:256 * 38]
    assert np.isin(coll, stretch).all() and heavy not in coll.tolist()
    assert (lab[256 * 38:256 * 44] == heavy).all()


def test_r9_fixture_facts(golden):
    # facts of the reference's own sample data
    assert int(golden["rows_total"]) == 18399          # Graphframes.py:18 print
    assert int(golden["rows_after_filter"]) == 18398   # :30 null filter drops 1 row
    V = golden["ids"].size
    assert V == 4613                                   # :54 print (distinct domains)
    s, d = golden["src"], golden["dst"]
    assert s.size == 18398
    assert np.unique(s.astype(np.int64) * V + d).size == 7742
    assert int((s == d).sum()) == 0
    deg = np.bincount(s, minlength=V) + np.bincount(d, minlength=V)
    assert deg.max() == 1223
    names = golden["names"]
    assert names[np.argmax(deg)] == "twitter.com"
    assert all(len(i) == 8 for i in golden["ids"][:50])


def test_r9_golden_reproduced_by_oracle(oracle, golden):
    V = golden["ids"].size
    final, hist, ties = oracle.lpa(V, golden["src"], golden["dst"], 10, per_iter=True)
    assert np.array_equal(hist, golden["labels_iter"])
    # survey-time scratch run: 619 communities, ties 622/310/201/184/194
    assert np.unique(hist[4]).size == 619
    assert ties[:5].tolist() == [622, 310, 201, 184, 194]
    assert ties.tolist() == golden["ties"].tolist()


def test_r9_outlier_facts(oracle, golden):
    V = golden["ids"].size
    lab = golden["labels_iter"][4]
    size, inc, flags, summ = oracle.outlier_l1(V, golden["src"], golden["dst"], lab)
    # App. B: n = 619, k = 61, 272 singletons -> thr = 1 -> nothing flagged
    assert (summ["n_groups"], summ["k"], summ["thr"], summ["n_flagged"]) == (619, 61, 1, 0)
    assert int((size == 1).sum()) == 272
    assert np.array_equal(size, golden["l1_size"]) and np.array_equal(inc, golden["l1_inc"])
    sub, flags2, s2 = oracle.outlier_l2(V, golden["src"], golden["dst"], lab, 5)
    # App. B L2 on C1: 40 vertices in 11 communities flagged
    assert (s2["n_flagged"], s2["n_communities_flagged"]) == (40, 11)
    assert np.array_equal(flags2, golden["l2_flags"].astype(bool))


def test_degree_mix_covers_bins():
    V, s, d = degree_mix(0)
    deg = np.bincount(s, minlength=V) + np.bincount(d, minlength=V)
    assert (deg > 4096).sum() >= 2 and ((deg > 512) & (deg <= 2048)).sum() >= 1
    for lo, hi in ((256, 512), (128, 256), (64, 128), (32, 64), (16, 32), (8, 16), (4, 8), (2, 4),
                   (1, 2), (0, 1)):
        assert ((deg > lo) & (deg <= hi)).sum() > 0, (lo, hi)
    assert (deg == 0).sum() > 0


def test_generators_deterministic(oracle):
    s1, d1 = oracle.gen_rmat(10, 16, seed=1)
    s2, d2 = oracle.gen_rmat(10, 16, seed=1)
    assert np.array_equal(s1, s2) and np.array_equal(d1, d2)
    assert s1.min() >= 0 and s1.max() < 1024
    s3, _ = oracle.gen_rmat(10, 16, seed=2)
    assert not np.array_equal(s1, s3)
    s, d = oracle.gen_sbm(1000, 10, 50000)
    same = (s // 100) == (d // 100)
    assert abs(same.mean() - 0.9) < 0.01


def test_chunglu_generator(oracle):
    """Config C5's generator (Chung-Lu, exponent 2.1, seed 7):
    deterministic, ids in range, the requested expected maximum degree, a heavy tail."""
    V, m = 200_000, 2_000_000
    s1, d1 = oracle.gen_chunglu(V, m, 2.1, 20_000.0, 7)
    s2, d2 = oracle.gen_chunglu(V, m, 2.1, 20_000.0, 7)
    assert np.array_equal(s1, s2) and np.array_equal(d1, d2)
    assert s1.min() >= 0 and max(s1.max(), d1.max()) < V
    s3, _ = oracle.gen_chunglu(V, m, 2.1, 20_000.0, 8)
    assert not np.array_equal(s1, s3)
    deg = np.bincount(s1, minlength=V) + np.bincount(d1, minlength=V)
    assert 0.9 * 20_000 < deg.max() < 1.1 * 20_000
    top = np.sort(deg)[::-1]
    # power-law tail: the top 1 % of vertices hold far more than 1 % of the arcs
    assert top[: V // 100].sum() > 0.2 * deg.sum()
