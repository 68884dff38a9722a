"""The fill-scatter form in superstep 3's refresh (LPA_FILL_STEP3): when
superstep 2's refresh took the form and the new vector is still in bits mode, superstep 3's
refresh sets every arc giant bit again and visits only the columns off the new giant label G,
in place of k_al_scatter's walk over every position of every changed column.  The decision is
taken on the device (one captured graph, both outcomes); the arc bits come out exact.

Every case is bit-exact against the CPU oracle after each superstep, and asserts on the
oracle's history first what makes it exercise the form (or its refusal), so no case passes
vacuously.  The leaver gadget is test_gpu_sparse_al's: H, a column of 600 CSC positions, leaves
G in superstep 3 and so goes through the form's scatter (150 pieces); z's 1,300 positions rejoin
G in superstep 3 and are carried by the filled bits alone; H rejoins in superstep 4 through
k_al_scatter, which reads the new gbits.

Measured on the oracle (asserted below as bounds), after superstep 3:
  R-MAT-16 + gadget: dirty arcs 0.89 % of 2,099,752, arcs off G 0.042 % in 189 columns, the
            longest H with 600 positions, G on 0.713 of the slots
  R-MAT-22 + gadget: dirty arcs 1.5 %, arcs off G 0.02 %
  tie_rows(): arcs off G 39.8 %, dirty arcs 19.4 %, longest column off G 616,000 positions
  odd:      dirty arcs 0.57 % (no rebuild), G on 895 of 1,088 slots (bits mode)

Run once against the -DLPA_SPARSE_POISON build (csrc/Makefile `variant`, LPA_LIB_PATH) this file
also proves that no reader misses a bit of the form: there its fill poisons every al[] entry.
"""
import numpy as np
import pytest

from graphs import tie_rows
from test_gpu_fill_scatter import odd  # noqa: F401  (the fixture: an arc count that is no multiple of 64)
from test_gpu_sparse_al import K_HOT_BITS, K_HOT_MIN_SLOTS, K_REBUILD_FRAC, TIE_STEPS, Case, _check, _gadget_case

pytestmark = pytest.mark.gpu

K_FRONTIER_FRAC = 0.005     # lpa_internal.h kFrontierFrac
K_FILL3_RATIO = 0.16        # kFill3Ratio
K_FILL_CAP = 4096           # kFillCap
K_FILL_CAP_SHIFT = 15       # kFillCapShift
K_PICK = 1024               # lpa_refresh.hip kPickK

SWITCHES = [{}, {"LPA_KEEP_BITS": "0"}, {"LPA_UNITS_PURE": "0"}, {"LPA_FUSED_BINS": "0"}, {"LPA_FRONTIER": "0"},
            {"LPA_GRAPHS": "0"}, {"LPA_SERIAL": "1"}, {"LPA_SPARSE_AL": "0"}]


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _after3(c):
    """What superstep 3's refresh sees, from the oracle: the pick's G, the dirty arcs, the columns off G."""
    if not hasattr(c, "deg"):
        c.deg = np.bincount(c.s, minlength=c.V) + np.bincount(c.d, minlength=c.V)
    arcs = int(c.deg.sum())
    h2, h3 = c.hist[1], c.hist[2]
    order = np.argsort(-c.deg, kind="stable")
    lab, cnt = np.unique(h3[order[:K_PICK]], return_counts=True)
    c.G3 = int(lab[cnt == cnt.max()].min())
    c.try3 = 5 * int(cnt.max()) >= min(c.V, K_PICK)
    off = (h3 != c.G3) & (c.deg > 0)
    c.arcs = arcs
    c.dirty3 = float(c.deg[h3 != h2].sum() / arcs)
    c.off3 = float(c.deg[off].sum() / arcs)
    c.off3_cols = int(off.sum())
    c.longest3 = int(c.deg[off].max())
    c.hot3 = float((h3[order[:min(c.V, K_HOT_BITS)]] == c.G3).mean())
    c.cap = max(K_FILL_CAP, arcs >> K_FILL_CAP_SHIFT)
    print(f"after superstep 3: G {c.G3} dirty {c.dirty3:.5f} off G {c.off3:.6f} in {c.off3_cols} columns, "
          f"longest {c.longest3}, hot share {c.hot3:.3f}, cap {c.cap}")
    return c


def _device_takes(c):
    """The device decision's four conditions, and no rebuild."""
    return (c.try3 and c.hot3 >= 0.5 and c.longest3 <= c.cap and K_FRONTIER_FRAC < c.dirty3 <= K_REBUILD_FRAC
            and c.off3 <= K_FILL3_RATIO * c.dirty3)


def _gadget_step3(c):
    # H leaves G in superstep 3 (a long column off G: the form's scatter writes it), z joins it
    # (carried by the filled bits alone), H rejoins in superstep 4 (k_al_scatter on the new gbits)
    assert c.G3 == c.G
    assert c.hist[1][c.H] == c.G and c.hist[2][c.H] != c.G and c.hist[3][c.H] == c.G
    assert c.hist[1][c.z] != c.G and c.hist[2][c.z] == c.G
    assert c.deg[c.H] == 600 and c.deg[c.z] == 1300
    assert _device_takes(c), vars(c)


@pytest.fixture(scope="module")
def small(oracle):
    c = _after3(_gadget_case(oracle, 16, 10))
    assert c.V < K_HOT_MIN_SLOTS                       # the small-kernel side
    assert c.arcs == 2099752, c.arcs
    assert 0.008 < c.dirty3 < 0.010, c.dirty3          # 0.89 % measured
    assert 0.0003 < c.off3 < 0.0005 and c.off3_cols == 189, (c.off3, c.off3_cols)   # 0.042 %
    assert c.longest3 == 600 and 0.70 < c.hot3 < 0.73, (c.longest3, c.hot3)       # H; 0.713
    # superstep 2's device decision takes the form too (0.86 % of the arcs off G, z the longest)
    off2 = c.deg[c.hist[1] != c.G].sum() / c.arcs
    assert off2 <= 0.0154 and c.deg[c.hist[1] != c.G].max() == 1300, off2
    _gadget_step3(c)
    return c


@pytest.fixture(scope="module")
def hot(oracle):
    c = _after3(_gadget_case(oracle, 22, 6))
    assert c.V >= K_HOT_MIN_SLOTS                      # the hot-kernel side
    assert 0.012 < c.dirty3 < 0.018, c.dirty3          # 1.5 % measured
    assert 0.0001 < c.off3 < 0.0003, c.off3            # 0.02 %
    assert 1.0 - float(c.arc_share) <= 0.0154          # superstep 2's device decision takes the form
    _gadget_step3(c)
    return c


@pytest.fixture(scope="module")
def ties(oracle):
    c = Case()
    c.V, c.s, c.d, _, c.G = tie_rows()
    _, c.hist, _ = oracle.lpa(c.V, c.s, c.d, TIE_STEPS, per_iter=True)
    c.hist.setflags(write=False)
    c.steps = TIE_STEPS
    _after3(c)
    for step in (1, 2, 3):   # bits mode after supersteps 1-3
        assert 2 * int((c.hist[step - 1] == c.G).sum()) >= c.V, step
    assert c.G3 == c.G and c.hot3 >= 0.5
    assert 0.39 < c.off3 < 0.41 and 0.19 < c.dirty3 < 0.20, (c.off3, c.dirty3)   # 39.8 %, 19.4 %
    assert c.longest3 == 616000 and c.longest3 > c.cap, (c.longest3, c.cap)
    assert c.dirty3 <= K_REBUILD_FRAC                  # the refresh scatters, no rebuild
    assert not _device_takes(c)
    return c


def _run(gfa, c, what, runs=0):
    """-> (labels, fill_refreshes after each superstep)"""
    fills = []
    with gfa.Graph(c.s, c.d, c.V) as g:
        for step in range(1, c.steps + 1):
            g.step(1)
            _check(c, g.labels(), step, what)
            info = g.info()
            nf, ns = info["fill_refreshes"], info["sparse_refreshes"]
            print(f"{what} superstep {step}: fill_refreshes {nf} sparse_refreshes {ns}")
            assert nf <= ns, (nf, ns)
            fills.append(nf)
        for k in range(runs):   # a reset while the state is live, then the replayed graphs
            _check(c, g.run(c.steps), c.steps, f"{what} lpa_run({c.steps}) #{k + 1}")
        return g.labels().copy(), fills


def _both_forms(fills, what):
    # exactly one in superstep 2 and one more in superstep 3
    assert fills[:3] == [0, 1, 2], f"{what}: fill_refreshes per superstep {fills}"


@pytest.mark.parametrize("env", [{}, {"LPA_FILL_STEP3": "2"}], ids=["default", "forced"])
def test_small_kernel_gadget(gfa, small, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, fills = _run(gfa, small, f"small {env}", runs=2)
    _both_forms(fills, f"small {env}")


def test_hot_kernel_gadget(gfa, hot):
    _, fills = _run(gfa, hot, "hot default")
    _both_forms(fills, "hot default")


def test_off_switch(gfa, small, monkeypatch):
    on, fills_on = _run(gfa, small, "small default")
    monkeypatch.setenv("LPA_FILL_STEP3", "0")
    off, fills = _run(gfa, small, "small LPA_FILL_STEP3=0")
    assert fills[:3] == [0, 1, 1], fills
    assert fills_on[2] == 2, fills_on
    assert np.array_equal(on, off)


def test_device_refusal_after_the_count(gfa, ties, monkeypatch):
    # superstep 2's form forced, so the count of superstep 3 runs (its gate is open) and refuses:
    # the fallback k_al_scatter then runs with the old gbits and unfilled bits
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    monkeypatch.setenv("LPA_FILL_STEP3", "1")
    _, fills = _run(gfa, ties, "tie_rows refusal")
    assert fills[1] >= 1, fills
    assert fills[2] == fills[1], f"superstep 3 took the form: {fills}"


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "alone")
def test_tie_rows_switches(gfa, ties, monkeypatch, env):
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    monkeypatch.setenv("LPA_FILL_STEP3", "2")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, fills = _run(gfa, ties, f"tie_rows forced {env}")
    if "LPA_SPARSE_AL" in env:
        assert fills[-1] == 0, fills
    else:
        assert fills[1] >= 1 and fills[2] == fills[1] + 1, f"superstep 3 did not take the forced form: {fills}"


def test_odd_arc_count(gfa, odd, monkeypatch):  # noqa: F811
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    monkeypatch.setenv("LPA_FILL_STEP3", "2")
    c = odd
    # superstep 3's refresh scatters (no rebuild) and its vector is in bits mode: the forced form runs
    assert 2 in c.fill_steps, c.fill_steps
    h2, h3 = c.hist[1], c.hist[2]
    top = np.argsort(-c.deg, kind="stable")[:K_PICK]
    lab, cnt = np.unique(h3[top], return_counts=True)
    G3 = int(lab[cnt == cnt.max()].min())
    assert c.deg[h3 != h2].sum() / c.arcs <= K_REBUILD_FRAC
    assert 2 * int((h3 == G3).sum()) >= (c.V + 63) // 64 * 64
    assert (h3[1 << 10:] != G3).all()                  # the last arcs' columns are off G: the tail word
    _, fills = _run(gfa, c, "odd arcs")
    assert fills[2] == fills[1] + 1, fills
