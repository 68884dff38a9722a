"""Sparse al[] after a one-GPU bits-mode rebuild: the arcs on the giant label are carried by
their arc giant bits, only the other arcs' labels are stored, and every reader of al[]
takes a set bit as the label Gb (gword[GW_AL_SPARSE]).

Every case is bit-exact against the CPU oracle after each superstep.  The preconditions
that make a case exercise the sparse path are asserted on the oracle's history first, so no
case passes vacuously.

The leaver gadget: two extra vertices z = V0 and H = V0 + 1, 700 parallel edges g* - z
(g* is the vertex whose id is the giant label) and 600 parallel edges z - H.  Oracle:
z holds G after superstep 1, leaves after 2 and rejoins after 3; H holds G after
superstep 2, takes z's id after 3 and rejoins after 4.
So H, a column of 600 CSC positions (more than one scatter chunk of 256), sits under a
set bit at the sparse rebuild of superstep 2, has its bits cleared through the
multi-chunk path in superstep 3 and is rewritten as a joiner in superstep 4, while z's
row (1,300 arcs, a hub row of three units) holds 700 bit-carried and 600 al-carried votes.

Measured on the oracle (asserted below as bounds):
  R-MAT-16: G on 0.591 of the slots after superstep 2 (k_al_rebuild_small's bits mode),
            changed-arc fraction of supersteps 1 -> 2 0.44 (> kRebuildFrac)
  R-MAT-22: G on 0.901 of the 1.31 M hottest vertices and on 0.985 of the arcs after
            superstep 2 (k_al_rebuild_hot's bits mode); from superstep 3 on 381-616
            ordinary vertices leave G in every superstep and about as many join it

Run once against the -DLPA_SPARSE_POISON build (csrc/Makefile `variant`, LPA_LIB_PATH) this
file also proves that no reader misses a bit: there the rebuild stores a wrong label on
the G arcs instead of skipping them.
"""
import numpy as np
import pytest

from graphs import tie_rows

pytestmark = pytest.mark.gpu

K_REBUILD_FRAC = 0.25           # lpa_internal.h kRebuildFrac
K_HOT_MIN_SLOTS = 1 << 22       # kHotMinSlots: k_al_rebuild_hot from here on
K_HOT_BITS = 32 * (40960 - 1)   # lpa_refresh.hip kHotBits
N_GZ, N_ZH = 700, 600
TIE_STEPS = 8


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


class Case:
    pass


def _gadget_case(oracle, scale, steps):
    """R-MAT-`scale` seed 1 plus the leaver gadget, the oracle's history and the preconditions."""
    c = Case()
    s0, d0 = oracle.gen_rmat(scale, 16, seed=1)
    V0 = 1 << scale
    _, h3, _ = oracle.lpa(V0, s0, d0, 3, per_iter=True)
    lab, cnt = np.unique(h3[2], return_counts=True)
    gstar = int(lab[np.argmax(cnt)])
    z, H = V0, V0 + 1
    c.V, c.z, c.H, c.G, c.steps = V0 + 2, z, H, gstar, steps
    c.s = np.concatenate([s0, np.full(N_GZ, gstar, np.int32), np.full(N_ZH, z, np.int32)]).astype(np.int32)
    c.d = np.concatenate([d0, np.full(N_GZ, z, np.int32), np.full(N_ZH, H, np.int32)]).astype(np.int32)
    _, c.hist, _ = oracle.lpa(c.V, c.s, c.d, steps, per_iter=True)
    c.hist.setflags(write=False)
    h = c.hist
    G = gstar
    # the H / z sequence
    assert h[0][z] == G and h[1][z] != G and h[2][z] == G, [int(h[k][z]) for k in range(4)]
    assert h[1][H] == G and h[2][H] == z and h[3][H] == G, [int(h[k][H]) for k in range(4)]
    c.deg = np.bincount(c.s, minlength=c.V) + np.bincount(c.d, minlength=c.V)
    # superstep 2's refresh rebuilds (changed arcs above kRebuildFrac) ...
    c.frac12 = c.deg[h[1] != h[0]].sum() / (2 * c.s.size)
    assert c.frac12 > K_REBUILD_FRAC, c.frac12
    # ... in bits mode: G on at least half of the hot slots (the kHotBits highest degrees)
    hot = np.argsort(-c.deg, kind="stable")[:min(c.V, K_HOT_BITS)]
    c.hot_share = float((h[1][hot] == G).mean())
    assert c.hot_share >= 0.5, c.hot_share
    c.arc_share = c.deg[h[1] == G].sum() / (2 * c.s.size)
    return c


@pytest.fixture(scope="module")
def small(oracle):
    c = _gadget_case(oracle, 16, 10)
    assert c.G == 12048, c.G
    assert c.V < K_HOT_MIN_SLOTS                       # k_al_rebuild_small
    assert float((c.hist[1] == c.G).mean()) >= 0.5     # 0.591 measured
    return c


@pytest.fixture(scope="module")
def hot(oracle):
    c = _gadget_case(oracle, 22, 6)
    assert c.V >= K_HOT_MIN_SLOTS                      # k_al_rebuild_hot
    assert c.hot_share >= 0.85 and c.arc_share >= 0.97, (c.hot_share, c.arc_share)
    # every superstep from 3 on has ordinary leavers and joiners (the clear-and-write path)
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
    # joiners in supersteps 2-4 and no leaver
    for step in range(2, c.steps + 1):
        was, now = c.hist[step - 2] == c.G, c.hist[step - 1] == c.G
        assert not (was & ~now).any(), step
        if step <= 4:
            assert (~was & now).any(), step
    return c


def _check(c, got, step, what):
    ref = c.hist[step - 1]
    bad = np.flatnonzero(got[:c.V] != ref)
    first = [(int(v), int(got[v]), int(ref[v])) for v in bad[:4]]
    assert bad.size == 0, f"{what} superstep {step}: {bad.size} labels differ, first (v, got, want) {first}"


def _run(gfa, c, what, sparse=True, runs=0):
    with gfa.Graph(c.s, c.d, c.V) as g:
        for step in range(1, c.steps + 1):
            g.step(1)
            _check(c, g.labels(), step, what)
            n = g.info()["sparse_refreshes"]
            print(f"{what} superstep {step}: sparse_refreshes {n}")
            if sparse and step >= 2:
                assert n >= 1, f"{what}: no refresh left al[] sparse by superstep {step}"
            if not sparse:
                assert n == 0, f"{what}: LPA_SPARSE_AL=0 and {n} sparse refreshes"
        for k in range(runs):   # a reset while al[] is sparse, then the replayed graphs
            _check(c, g.run(c.steps), c.steps, f"{what} lpa_run({c.steps}) #{k + 1}")


def test_small_kernel_leaver_gadget(gfa, small):
    _run(gfa, small, "small", runs=2)


def test_small_kernel_dense_switch(gfa, small, monkeypatch):
    monkeypatch.setenv("LPA_SPARSE_AL", "0")
    _run(gfa, small, "small LPA_SPARSE_AL=0", sparse=False, runs=1)


def test_hot_kernel_leaver_gadget(gfa, hot):
    _run(gfa, hot, "hot")


def test_hot_kernel_dense_switch(gfa, hot, monkeypatch):
    monkeypatch.setenv("LPA_SPARSE_AL", "0")
    _run(gfa, hot, "hot LPA_SPARSE_AL=0", sparse=False)


@pytest.mark.parametrize("env", [{}, {"LPA_SPARSE_AL": "0"}, {"LPA_KEEP_BITS": "0"}, {"LPA_UNITS_PURE": "0"},
                                 {"LPA_FUSED_BINS": "0"}, {"LPA_FRONTIER": "0"}, {"LPA_GRAPHS": "0"},
                                 {"LPA_SERIAL": "1"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "shipped")
def test_tie_rows_switches(gfa, ties, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _run(gfa, ties, f"tie_rows {env}", sparse="LPA_SPARSE_AL" not in env)
