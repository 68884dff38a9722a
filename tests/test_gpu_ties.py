"""Engineered ties and bin-edge degrees at the giant-label decision sites.

Every kernel that decides a row without tallying it (giant_decide, the row bins' and
k_lpa_block's giant tests, k_lpa_units_giant + k_hub_decide, the strict-majority settles
from the arc giant bits, the 2-bit giant codes) is exact through one strict comparison
and one packing width.  tests/graphs.py tie_rows builds rows whose neighbourhood
histogram is known analytically -- G exactly tied with a rival below / above it, G one
vote above / below, rivals sharing one hash bucket, whole 512-arc units of one bucket --
at degrees on both sides of every bin, tier and unit boundary, delivered to supersteps
2, 3 and 4 (rows of depth 1, 2, 3).  The oracle's history is first checked against the
analytic tables on the CPU (so no case passes vacuously), then every case is bit-exact
against it at supersteps 1..8.

Measured on the fixture (oracle; the preconditions below assert the bounds):
  V 163,522, 10,400,813 edges, 738 rows (60 of them without a blinker pair)
  changed-arc fraction after supersteps 1..5: 0.821, 0.480, 0.194, 0.035, 0.0003
  G on 0.617 / 0.684 / 0.750 of the slots after supersteps 1 / 2 / 3
  G on 0.626 / 0.686 / 0.745 of the 1024 highest-degree vertices
  loopback P = 2 and 4, every rank: 1 full exchange (superstep 1), 7 delta, 0 giant

Not reached: k_lpa_block's own giant test (gcnt > gmax).  In superstep 2 the block tiers
are decided by k_lpa_units_giant + k_hub_decide and the kernel gets no gsel; in the other
supersteps it either gets none (superstep 1) or is not launched.
"""
import numpy as np
import pytest

from graphs import tie_mode, tie_rows

pytestmark = pytest.mark.gpu

STEPS = 8
PAD = 1 << 22
K_REBUILD_FRAC = 0.25       # lpa_internal.h kRebuildFrac
K_FRONTIER_FRAC = 0.005     # kFrontierFrac
K_HOT_BITS = 32 * (40960 - 1)   # lpa_refresh.hip kHotBits: the hot slots of a P = 1 handle
BINS = ("seg", "w16", "w8", "w4", "w2", "g64", "g32", "g16", "g8", "g4", "g2", "g1")


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


class Ties:
    pass


@pytest.fixture(scope="module")
def ties(oracle):
    """The fixture, the oracle's history and the CPU preconditions, once per module."""
    t = Ties()
    t.V, t.s, t.d, t.rows, t.G = tie_rows()
    V, s, d, G = t.V, t.s, t.d, t.G
    _, t.hist, _ = oracle.lpa(V, s, d, STEPS, per_iter=True)
    t.hist.setflags(write=False)
    t.deg = np.bincount(s, minlength=V) + np.bincount(d, minlength=V)
    t.row_ids = np.array([r for r, _, _ in t.rows])
    t.row_depth = np.array([k for _, k, _ in t.rows])
    t.row_mode = np.array([tie_mode(tab) for _, _, tab in t.rows])
    t.row_deg = t.deg[t.row_ids]

    # histogram and mode: rows are only ever sources, so their arcs are the edges they start
    assert not np.isin(d, t.row_ids).any()
    order = np.argsort(s, kind="stable")
    start = np.searchsorted(s[order], np.arange(V + 1))
    for r, depth, tab in t.rows:
        nb = d[order[start[r]:start[r + 1]]]
        blinkers = nb.size - sum(tab.values())     # the pair, or none (the exact-half rows)
        assert nb.size == t.deg[r] and blinkers in (0, 2)
        for step in range(depth + 1, STEPS + 1):
            lab, cnt = np.unique(t.hist[step - 2][nb], return_counts=True)
            got = dict(zip(lab.tolist(), cnt.tolist()))
            single = [l for l in got if l not in tab]
            assert all(got.get(l) == v for l, v in tab.items()) and len(single) == blinkers and \
                all(got[l] == 1 for l in single), (r, depth, step, tab)
            assert t.hist[step - 1][r] == tie_mode(tab), (r, depth, step, tab)
    # G's share of the slots and of the 1024 highest-degree vertices
    top = np.argsort(-t.deg, kind="stable")[:1024]
    for step in (1, 2, 3):
        assert (t.hist[step - 1][top] == G).mean() >= 0.2, step
    for step in (1, 2):
        n_g = int((t.hist[step - 1] == G).sum())
        assert 2 * n_g >= V, (step, n_g)             # compact: the bits-mode rebuild
        assert 2 * n_g < K_HOT_BITS, (step, n_g)      # padded: G on under half the hot slots
    # changed arcs per superstep: rebuild, rebuild, scatter with every row, frontier from 5 on
    prev = np.arange(V)
    frac = []
    for step in range(1, STEPS + 1):
        frac.append(t.deg[t.hist[step - 1] != prev].sum() / (2 * s.size))
        prev = t.hist[step - 1]
    assert frac[0] > K_REBUILD_FRAC and frac[1] > K_REBUILD_FRAC, frac
    assert K_FRONTIER_FRAC < frac[2] < K_REBUILD_FRAC, frac
    assert all(0 < f < K_FRONTIER_FRAC for f in frac[4:]), frac
    return t


def _check(t, got, step, what):
    """Labels after superstep `step`: bit-exact against the oracle, and the rows' analytic modes."""
    ref = t.hist[step - 1]
    bad = np.flatnonzero(got[:t.V] != ref)
    rows = bad[np.isin(bad, t.row_ids)]
    detail = [(int(r), int(got[r]), int(ref[r]), t.rows[int(np.flatnonzero(t.row_ids == r)[0])][1:])
              for r in rows[:3]]
    assert bad.size == 0, f"{what} superstep {step}: {bad.size} labels differ ({rows.size} rows), first {detail}"
    assert np.array_equal(got[t.V:], np.arange(t.V, got.size)), f"{what} superstep {step}: padding changed"
    due = t.row_depth + 1 <= step
    assert np.array_equal(got[t.row_ids[due]], t.row_mode[due]), f"{what} superstep {step}: analytic row labels"


def _run_steps(gfa, t, V, what, after_first=None):
    with gfa.Graph(t.s, t.d, V) as g:
        for step in range(1, STEPS + 1):
            g.step(1)
            if step == 1 and after_first:
                after_first(g)
            _check(t, g.labels(), step, what)


def test_fixture_degrees_and_bins(gfa, ties):
    """lpa_degrees of every row is its intended degree, every degree bin holds vertices,
    and the rows above 1024 arcs are hub rows."""
    t = ties
    with gfa.Graph(t.s, t.d, t.V) as g:
        deg = g.degrees()
        info = g.info()
    assert np.array_equal(deg, t.deg)
    assert np.array_equal(deg[t.row_ids], t.row_deg)
    assert all(info["bin_vertices"][b] > 0 for b in BINS), info["bin_vertices"]
    assert info["hub_vertices"] >= int((t.row_deg > 1024).sum())
    assert info["max_degree"] == t.deg.max()


def test_compact_shipped_schedule(gfa, ties):
    """The compact fixture (G on more than half of the slots: the bits-mode rebuilds and the
    settles from the arc giant bits), the shipped schedule, then lpa_run(8) twice on the
    same handle (replayed graphs)."""
    t = ties
    with gfa.Graph(t.s, t.d, t.V) as g:
        for step in range(1, STEPS + 1):
            g.step(1)
            _check(t, g.labels(), step, "compact")
        assert g.info()["code_refresh"] == 0
        for k in range(2):
            _check(t, g.run(STEPS), STEPS, f"compact lpa_run({STEPS}) #{k + 1}")


@pytest.mark.parametrize("env", [{"LPA_FIRST_RUNS": "0"}, {"LPA_FRONTIER": "0"}, {"LPA_SERIAL": "1"},
                                 {"LPA_GRAPHS": "0"}, {"LPA_KEEP_BITS": "0"}, {"LPA_UNITS_PURE": "0"},
                                 {"LPA_FUSED_BINS": "0"}, {"LPA_REBUILD_HOT": "0"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_compact_switches(gfa, ties, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _run_steps(gfa, ties, ties.V, f"compact {env}")


@pytest.mark.parametrize("env", [{}, {"LPA_CODE_LBIN": "8"}, {"LPA_GIANT_CODES": "0"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "shipped")
def test_padded_giant_codes(gfa, ties, monkeypatch, env):
    """Padded to 2^22 slots (G on under half of the hot slots): the giant-code refresh after
    superstep 1, superstep 2's decisions from the 2-bit codes (k_lpa_units_code2 +
    k_hub_decide, k_code_settle) and superstep 3's (k_code_settle_hubs); with the cut that
    codes the rows of 9-64 arcs too, and with the codes off."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = 0 if "LPA_GIANT_CODES" in env else 1

    def taken(g):
        assert g.info()["code_refresh"] == want, "the giant-code refresh"

    _run_steps(gfa, ties, PAD, f"padded {env}", taken)


@pytest.mark.parametrize("P", [2, 4])
def test_padded_loopback_delta_after_code_refresh(gfa, ties, P):
    """The padded fixture on a loopback group: every rank bit-exact, and superstep 2's
    changes (far below slice / 4 per rank) arrive through a DELTA exchange after the
    giant-code refresh of superstep 1 -- the refresh that must rebuild al[] whatever the
    change count, since the rows settled from codes have no al[] entries."""
    t = ties
    lb = gfa.Loopback(P)
    ranks = [gfa.Graph(t.s, t.d, PAD, rank=r, loopback=lb) for r in range(P)]
    try:
        def work(r, g):
            labs, infos = [], []
            for step in range(1, STEPS + 1):
                g.step(1)
                labs.append(g.labels())
                infos.append(g.info())
            return labs, infos

        res = gfa.run_ranks(ranks, work)
        for r in range(P):
            labs, infos = res[r]
            print(f"P={P} rank {r} exchanges (full, delta, giant) per superstep:",
                  [(i["exchanges_full"], i["exchanges_delta"], i["exchanges_giant"]) for i in infos])
            for step in range(1, STEPS + 1):
                _check(t, labs[step - 1], step, f"P={P} rank {r}")
            assert infos[0]["code_refresh"] == 1, f"P={P} rank {r}: the giant-code refresh was not taken"
            assert infos[1]["exchanges_delta"] == infos[0]["exchanges_delta"] + 1, \
                f"P={P} rank {r}: superstep 2 was not a delta exchange"
    finally:
        for g in ranks:
            g.close()
        lb.close()
