"""The fill-scatter form of the sparse bits-mode rebuild (LPA_FILL_SCATTER, DESIGN.md sections 3
and 4): every arc giant bit is set, then only the columns off the giant label G are visited
through the CSC position index -- al[p] = L[u] and bit p cleared for each position p of such a
column u -- instead of a stream over every arc.

Every case is bit-exact against the CPU oracle after each superstep, and asserts on the
oracle's history first what makes it exercise the form, so no case passes vacuously.  The
leaver gadget is test_gpu_sparse_al's: z, a column of 1,300 CSC positions (325 of the scatter's
pieces, five rounds of one wave), holds G after superstep 1 and not after superstep 2,
so superstep 2's scatter writes it, 700 of its row's votes being bit-carried and 600
al-carried; H (600 positions) leaves G in superstep 3 through k_al_scatter on top of the
filled bits.

Measured on the oracle (asserted below as bounds): R-MAT-22 plus the gadget, after superstep 2
the columns off G hold 0.0153 of the arcs (0.0151 without the gadget).

The device decision takes the form up to kFillFrac = 0.0154 of the arcs (lpa_internal.h; half
the break-even share measured at R-MAT-24), so test_hot_kernel_default sees
it at this graph's 0.0153; test_hot_kernel_forced runs it there whatever the constant.

Run once against the -DLPA_SPARSE_POISON build (csrc/Makefile `variant`, LPA_LIB_PATH) this file
also proves that no reader misses a bit of the form: there every al[] entry is poisoned before
the scatter.
"""
import numpy as np
import pytest

from graphs import tie_rows
from test_gpu_sparse_al import K_HOT_BITS, K_HOT_MIN_SLOTS, K_REBUILD_FRAC, TIE_STEPS, Case, _check, _gadget_case

pytestmark = pytest.mark.gpu

SHIPS_ON = True         # LPA_FILL_SCATTER defaults to 1 (the device decision)


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _z_is_long_leaver(c):
    # z: G after superstep 1, not G after superstep 2 (written by superstep 2's scatter), long
    assert c.hist[0][c.z] == c.G and c.hist[1][c.z] != c.G
    assert c.deg[c.z] > 256, int(c.deg[c.z])
    assert c.deg[c.z] == 1300, int(c.deg[c.z])


@pytest.fixture(scope="module")
def small(oracle):
    c = _gadget_case(oracle, 16, 10)
    assert c.V < K_HOT_MIN_SLOTS                       # k_al_rebuild_small's side
    assert float((c.hist[1] == c.G).mean()) >= 0.5
    _z_is_long_leaver(c)
    return c


@pytest.fixture(scope="module")
def hot(oracle):
    c = _gadget_case(oracle, 22, 6)
    assert c.V >= K_HOT_MIN_SLOTS                      # k_al_rebuild_hot's side
    _z_is_long_leaver(c)
    c.off_share = 1.0 - float(c.arc_share)
    print(f"R-MAT-22 + gadget: arcs off G after superstep 2: {c.off_share:.4f}")
    assert c.off_share <= 0.03, c.off_share            # 0.0151 measured
    # supersteps 3-6: ordinary leavers and joiners on top of the filled bits (k_al_scatter)
    for step in range(3, c.steps + 1):
        was, now = c.hist[step - 2][:c.V - 2] == c.G, c.hist[step - 1][:c.V - 2] == c.G
        assert (was & ~now).sum() >= 100 and (~was & now).sum() >= 100, step
    return c


@pytest.fixture(scope="module")
def ties(oracle):
    c = Case()
    c.V, c.s, c.d, _, c.G = tie_rows()
    _, c.hist, _ = oracle.lpa(c.V, c.s, c.d, TIE_STEPS, per_iter=True)
    c.hist.setflags(write=False)
    c.steps = TIE_STEPS
    for step in (1, 2):   # the bits-mode rebuilds after supersteps 1 and 2
        assert 2 * int((c.hist[step - 1] == c.G).sum()) >= c.V, step
    return c


@pytest.fixture(scope="module")
def odd(oracle):
    """R-MAT-10 plus five pairs of fresh degree-1 vertices joined to each other: an arc count
    that is no multiple of 64, and the lowest-ranked rows (the last arcs) have columns that
    never hold G."""
    c = Case()
    s0, d0 = oracle.gen_rmat(10, 16, seed=1)
    V0, pairs = 1 << 10, 0
    s, d = s0, d0
    while pairs == 0 or (2 * s.size) % 64 == 0 or pairs < 5:
        a = V0 + 2 * pairs
        s = np.concatenate([s, np.array([a], np.int32)]).astype(np.int32)
        d = np.concatenate([d, np.array([a + 1], np.int32)]).astype(np.int32)
        pairs += 1
    c.V, c.s, c.d, c.steps = V0 + 2 * pairs, s, d, 6
    c.arcs = 2 * s.size
    assert c.arcs % 64 != 0, c.arcs
    _, c.hist, _ = oracle.lpa(c.V, c.s, c.d, c.steps, per_iter=True)
    c.hist.setflags(write=False)
    c.deg = np.bincount(c.s, minlength=c.V) + np.bincount(c.d, minlength=c.V)
    new = np.arange(V0, c.V)
    # the new vertices: degree 1 (no row ranks below them: degree descending, then id) ...
    assert (c.deg[new] == 1).all() and c.deg[c.deg > 0].min() == 1
    # ... and some refresh rebuilds in bits mode with them off its giant label: the most
    # frequent label among the 1,024 highest degrees, on at least half the slots (all hot here)
    c.fill_steps = []
    top = np.argsort(-c.deg, kind="stable")[:1024]
    for step in range(1, c.steps):
        h, prev = c.hist[step - 1], (c.hist[step - 2] if step > 1 else np.arange(c.V))
        lab, cnt = np.unique(h[top], return_counts=True)
        G = int(lab[cnt == cnt.max()].min())
        frac = c.deg[h != prev].sum() / c.arcs
        vpad = (c.V + 63) // 64 * 64
        if frac > K_REBUILD_FRAC and 2 * int((h == G).sum()) >= vpad and not (h[new] == G).any():
            c.fill_steps.append(step)
    assert c.fill_steps, "no bits-mode rebuild in the oracle's history"
    assert c.V < K_HOT_BITS
    return c


def _run(gfa, c, what, fill=None, sparse=True, runs=0, fill_from=2):
    """fill: True = fill_refreshes >= 1 from superstep fill_from on, False = stays 0, None = free."""
    with gfa.Graph(c.s, c.d, c.V) as g:
        if hasattr(c, "arcs"):
            assert g.info()["arcs"] == c.arcs, (g.info()["arcs"], c.arcs)
        for step in range(1, c.steps + 1):
            g.step(1)
            _check(c, g.labels(), step, what)
            info = g.info()
            nf, ns = info["fill_refreshes"], info["sparse_refreshes"]
            print(f"{what} superstep {step}: fill_refreshes {nf} sparse_refreshes {ns}")
            assert nf <= ns, (nf, ns)
            if sparse and step >= fill_from:
                assert ns >= 1, f"{what}: no refresh left al[] sparse by superstep {step}"
            if not sparse:
                assert ns == 0 and nf == 0, f"{what}: LPA_SPARSE_AL=0 and counters {ns}, {nf}"
            if fill is True and step >= fill_from:
                assert nf >= 1, f"{what}: no refresh took the fill-scatter form by superstep {step}"
            if fill is False:
                assert nf == 0, f"{what}: {nf} fill-scatter refreshes"
        for k in range(runs):   # a reset while the state is live, then the replayed graphs
            _check(c, g.run(c.steps), c.steps, f"{what} lpa_run({c.steps}) #{k + 1}")
        return g.labels().copy()


def test_small_kernel_forced(gfa, small, monkeypatch):
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    _run(gfa, small, "small LPA_FILL_SCATTER=2", fill=True, runs=2)


def test_small_kernel_off(gfa, small, monkeypatch):
    monkeypatch.setenv("LPA_FILL_SCATTER", "0")
    off = _run(gfa, small, "small LPA_FILL_SCATTER=0", fill=False)
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    on = _run(gfa, small, "small LPA_FILL_SCATTER=2", fill=True)
    assert np.array_equal(on, off)


def test_hot_kernel_default(gfa, hot):
    _run(gfa, hot, "hot default", fill=True if SHIPS_ON else None)


def test_hot_kernel_forced(gfa, hot, monkeypatch):
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    _run(gfa, hot, "hot LPA_FILL_SCATTER=2", fill=True)


@pytest.mark.parametrize("env", [{}, {"LPA_KEEP_BITS": "0"}, {"LPA_UNITS_PURE": "0"}, {"LPA_FUSED_BINS": "0"},
                                 {"LPA_FRONTIER": "0"}, {"LPA_GRAPHS": "0"}, {"LPA_SERIAL": "1"},
                                 {"LPA_SPARSE_AL": "0"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "alone")
def test_tie_rows_switches(gfa, ties, monkeypatch, env):
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sparse = "LPA_SPARSE_AL" not in env
    _run(gfa, ties, f"tie_rows LPA_FILL_SCATTER=2 {env}", fill=sparse, sparse=sparse)


def test_odd_arc_count(gfa, odd, monkeypatch):
    monkeypatch.setenv("LPA_FILL_SCATTER", "2")
    _run(gfa, odd, "odd arcs", fill=True, sparse=True, fill_from=odd.fill_steps[0])
