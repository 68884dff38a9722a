"""CPU checks of the label exchange's fixtures (tests/exchange_ref.py CASES): for every case of
tests/test_gpu_exchange_edges.py, the oracle's label history and the restated slot map put the
case where it was built to be -- the exact capd / capg of every superstep, on the intended side
of the intended threshold, and the forms that the restated rule derives from them.  A
precondition that does not hold fails here, without a GPU; the GPU tests repeat the same
assertions with the slot map read back from the library."""
import numpy as np
import pytest

import exchange_ref as X
import graphs


def _steps(name):
    _, P, pow2, req = X.CASES[name]
    V, s, d, groups, hist = X.case_history(name)
    smap = X.restated_map(V, s, d, P, pow2)
    return X.restate(V, s, d, hist, smap, req), smap, groups


def test_every_case_has_its_expectation():
    assert set(X.CASES) == set(X.EXPECT)


@pytest.mark.parametrize("name", list(X.CASES))
def test_case_precondition(oracle, name):
    steps, smap, _ = _steps(name)
    X.check_precondition(name, steps, smap)


def test_slot_map_round_trip():
    """map_from_l0 inverts l0_slices (what the GPU test reads back), and refuses a map that
    holds a vertex twice."""
    V, s, d, _ = graphs.blinker_field(70, paths=1)
    m = X.restated_map(V, s, d, 8)
    back = X.map_from_l0(V, 8, m.l0_slices(), m.slot_of[0])
    assert np.array_equal(back.slot_of, m.slot_of) and np.array_equal(back.order, m.order)
    bad = m.l0_slices().copy()
    bad[1, 0] = bad[0, 1]
    with pytest.raises(AssertionError):
        X.map_from_l0(V, 8, bad, m.slot_of[0])


def test_rule_at_its_thresholds():
    """choose / posted_cap against the sentences of DESIGN.md section 5, by hand."""
    S, dcap = 4096, 1024
    assert X.choose(dcap, dcap, S, dcap) == "delta"               # a delta of dcap entries fits
    assert X.choose(dcap + 1, dcap + 1, S, dcap) == "full"
    assert X.choose(dcap + 1, dcap, S, dcap) == "giant"           # capg == dcap fits
    assert X.choose(65, 1, S, dcap) == "delta"                    # capd == capg + slice / 64: the tie
    assert X.choose(66, 1, S, dcap) == "giant"
    assert X.choose(0, 0, S, dcap) == "delta"
    assert X.choose(16, 16, 64, 16) == "delta" and X.choose(17, 16, 64, 16) == "giant"
    assert X.choose(17, 17, 64, 16) == "full"
    assert X.posted_cap(4, 4096) == 1024 and X.posted_cap(512, 4096) == 1024
    assert X.posted_cap(513, 4096) == 2048 and X.posted_cap(513, 1024) == 0
    assert X.posted_cap(1 << 16, 1 << 20) == 1 << 17 and X.posted_cap((1 << 16) + 1, 1 << 20) == 0
    assert X.agreed_post_cap(4, 4096, [-1, 16]) == 16 and X.agreed_post_cap(4, 4096, [-1, 0]) == 0
    assert X.agreed_post_cap(4, 64, [1 << 20, -1]) == 0 and X.agreed_post_cap(4, 4096, [1 << 20] * 2) == 4096


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("S", [64, 4096])
def test_delta_capacity_sides(oracle, P, S):
    """The largest per-rank count of every superstep from 3 on is dcap - 1, dcap, dcap + 1."""
    for k in (-1, 0, 1):
        steps, smap, _ = _steps(f"dcap_s{S}_P{P}_{k:+d}")
        assert smap.slice == S
        assert all(st.capd == S // 4 + k and max(st.ng) == S // 4 + k for st in steps[2:])


def test_uneven_ranks_counts():
    """Counts of 0 beside counts of 1; ranks that own no real vertex, and no arc."""
    for name in ("uneven_P4_V70_pair", "uneven_P8_V70_path", "uneven_P8_V5_pair", "uneven_P4_V7_path"):
        steps, smap, _ = _steps(name)
        assert smap.slice == 64
        assert all(sorted(set(st.nd)) == [0, 1] for st in steps[2:]), name
    steps, smap, _ = _steps("uneven_P8_V5_pair")
    assert np.bincount(smap.rank_of, minlength=8).tolist() == [1, 1, 1, 1, 1, 0, 0, 0]


def test_giant_tie_sides():
    """capd == capg + slice / 64 in the superstep the leaves adopt G (tie: delta), one more
    (giant); capg == dcap and dcap + 1 with capd above dcap."""
    for name, t, diff in (("tie_D1_n127", 3, 64), ("tie_D1_n128", 3, 65), ("tie_D2_n128", 4, 64),
                          ("tie_D2_n129", 4, 65)):
        steps, smap, _ = _steps(name)
        st = steps[t - 1]
        assert smap.slice == 4096 and st.post == 0 and st.giant_offered
        assert st.capd - st.capg == diff and st.capd <= 1024, (name, st.capd, st.capg)
        assert st.form == ("delta" if diff == 64 else "giant")
    for name, capg in (("capg_dcap", 1024), ("capg_dcap+1", 1025)):
        st = _steps(name)[0][2]
        assert st.capg == capg and st.capd > 1024 and st.form == ("giant" if capg == 1024 else "full")


def test_rise_sides():
    """The broom's burst starts at superstep D + 2, a converged one: above dcap per rank with
    the lists walked (full from there on), below it (delta throughout)."""
    for D in (4, 6):
        steps, smap, groups = _steps(f"rise_lists_D{D}")
        assert smap.slice == 64 and D + 2 >= X.CONVERGED_FROM
        assert all(any(st.walked) for st in steps[4:])
        assert all(st.capd <= 16 and st.form == "delta" for st in steps[3:D + 1])
        assert all(st.capd > 16 and st.form == "full" for st in steps[D + 1:])
        steps, smap, _ = _steps(f"rise_lists_below_D{D}")
        assert all(any(st.walked) for st in steps[4:])
        assert all(14 <= st.capd <= 16 for st in steps[D + 1:]) and all(st.form == "delta" for st in steps[2:])
        steps, _, _ = _steps(f"rise_slice_D{D}")
        assert not any(any(st.walked) for st in steps)
        assert [st.form for st in steps[D + 1:D + 4]] == ["giant", "full", "giant"]


def test_pulse_sides():
    """delta -> full -> delta inside the converged supersteps, then deltas without an entry."""
    for name, D in (("pulse_lists_D4", 4), ("pulse_lists_D5", 5)):
        steps, smap, _ = _steps(name)
        assert smap.slice == 64 and all(any(st.walked) for st in steps[4:])
        forms = [st.form for st in steps]
        assert forms[D:D + 5] == ["delta", "full", "full", "full", "delta"] and D + 1 >= X.CONVERGED_FROM
        assert all(st.capd > 16 for st in steps[D + 1:D + 4]) and steps[D + 4].capd == 0
    steps, _, _ = _steps("pulse_slice_D4")
    assert [st.form for st in steps[4:]] == ["delta", "giant", "full", "giant", "delta", "delta"]
    assert not any(any(st.walked) for st in steps[:9]) and all(steps[9].walked)


def test_posted_sides():
    for c, S in ((16, 4096), (1024, 8192)):
        for k in (0, 1):
            steps, smap, _ = _steps(f"posted_{c}_{k:+d}")
            assert smap.slice == S and S // 4 >= 1024
            assert all(st.post == c and st.capd == c + k for st in steps[2:])
            assert all(st.counters == ((0, 1, 0, 1, 0) if k == 0 else (0, 1, 0, 0, 1)) for st in steps[2:])
    st = _steps("posted_miss_delta")[0][7]
    assert st.post == 16 < st.capd <= 1024 and st.counters == (0, 1, 0, 0, 1)
    st = _steps("posted_miss_full")[0][7]
    assert st.post == 8 < 16 < st.capd and st.counters == (1, 0, 0, 0, 1)
    steps = _steps("posted_adaptive_burst")[0]
    assert [st.post for st in steps[2:8]] == [4096, 4096, 1024, 1024, 1024, 1024]
    assert steps[7].capd > 1024 and steps[7].counters == (0, 0, 1, 0, 1)


def test_odd_slices_slots():
    """Tight slices, no multiple of 512 slots: slots 0, 63, 64 and slice - 1 of every rank
    change in every superstep from 3 on, and no vertex is isolated."""
    for name, P, S in (("odd_P3_s192", 3, 192), ("odd_P2_s576", 2, 576), ("odd_P2_s4160", 2, 4160)):
        steps, smap, _ = _steps(name)
        V, s, d, _, _ = X.case_history(name)
        assert smap.slice == S and S % 512 != 0 and V == P * S
        assert (np.bincount(s, minlength=V) + np.bincount(d, minlength=V)).min() >= 1
        for st in steps[2:]:
            for r in range(P):
                assert {0, 63, 64, S - 1} <= set(st.changed[r][0].tolist()), (name, st.t, r)


@pytest.mark.parametrize("name", list(X.COMPACT))
def test_compact_counts(oracle, name):
    """The caller-driven cases of k_delta_compact: 0, 1, 255, 256, 257 changes in one rank, and
    changes in the last 64 slots of a slice of 2^20 + 64 (the grid-stride loop's second trip)."""
    build, P, pow2, counts = X.COMPACT[name]
    V, s, d, _ = build()
    _, hist, _ = oracle.lpa(V, s, d, 8, per_iter=True)
    smap = X.restated_map(V, s, d, P, pow2)
    steps = X.restate(V, s, d, hist, smap)
    assert all(sorted(st.nd) == sorted(counts) for st in steps[2:]), [st.nd for st in steps]
    assert all(st.capd <= smap.slice // 4 for st in steps[2:])
    if name == "second_trip":
        assert smap.slice == (1 << 20) + 64 == 4096 * 256 + 64
        assert all(st.changed[r][0].max() == smap.slice - 1 for st in steps[2:] for r in range(P))
