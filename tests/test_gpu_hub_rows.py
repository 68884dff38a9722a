"""The hub-row kernels on the row-span loads (csrc/lpa_device.h span_load / span_pair_batch, DESIGN.md
section 4): k_settle_big (superstep 3's settle from the arc giant bits), k_hub_decide (superstep 2's
giant decision from the unit counts) and k_code_settle_hubs (superstep 3 after a giant-code refresh).
A wave reads its row 8 x 64 elements a step, clamped inside the row's last round and masked afterwards,
with its rows' bounds held 64 rows ahead in lanes; the settle issues the first 256 words of four of its
rows together.

Directly: tools/microbench/hub_rows_check.hip (built by the csrc Makefile, one fresh process per group)
calls the kernels' launch wrappers on synthetic rows and compares every output with a host reference --
row lengths around one lane trip, the settle's first 256 words, one span step, two and four steps; row
starts at bits 0, 1 and 63 of a word, ends on a word's last and first bit, the last row ending in the array's last word; set-bit counts
of exactly half (must not settle), half + 1, all, none, random, and the set bits packed into the row's
first or last word, every row's end bits and its neighbours' set; 0, 1, 3, 4, 5 rows, one more than the
grid's waves, one more than the 64-row bounds batch; the gates closed.  Each case is launched twice on
the same buffers; every output ends in a checked guard.

End to end: tie_rows with hub degrees at those edges, bit-exact against the CPU oracle after each of
supersteps 1-5 under the schedules that reach the three kernels.  The rows that turn an over-count into
a wrong label are tie_rows' z_half_pure rows (G on exactly half of all arcs, the smaller rival A on the
rest: one bit too many settles the row on G where A wins the tie); the long settled row is the G
anchor's own (every neighbour on G from superstep 1 on), and _majority_rows adds one row per degree
with G on half + 1 of all its arcs, which the settle must take."""
import os
import subprocess

import numpy as np
import pytest

from graphs import tie_anchor_ids, tie_rows
from test_gpu_sparse_al import Case, _check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "lpa_hip", "hub_rows_check")

# seconds: about ten times a group's wall time on one MI355X (settle 0.41, decide 0.37, code 0.28, mostly
# the process's start and the buffers' allocation), and room for a slow start on a shared machine; the
# limit only ends a hang
TIMEOUT = {"settle": 8, "decide": 8, "code": 8}

K_SPAN = 8                  # lpa_device.h kSpanK
K_PICK = 1024               # lpa_refresh.hip kPickK
STEP = K_SPAN * 4096        # arcs of one span step of bit words
HUB_DEGREES = (1025, 4095, 4096, 4097, STEP - 1, STEP, STEP + 1, 2 * STEP + 1)
STEPS = 5

SCHEDULES = [{}, {"LPA_SERIAL": "1"}, {"LPA_GRAPHS": "0"}, {"LPA_FILL_SCATTER": "0"}, {"LPA_GIANT_CODES": "0"}]


def _run_check(group):
    if not os.path.exists(CHECK):
        pytest.fail(f"{CHECK} missing: run __graft_entry__.build() (csrc Makefile target)")
    r = subprocess.run([CHECK, group], capture_output=True, text=True, timeout=TIMEOUT[group])
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"hub_rows_check {group}: ok (" in r.stdout, r.stdout + r.stderr


def test_settle_big_matches_bit_counts():
    _run_check("settle")


def test_hub_decide_matches_unit_sums():
    _run_check("decide")


def test_code_settle_hubs_matches_unit_sums():
    _run_check("code")


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _g_arcs(c, h):
    """Per vertex, the arcs of its row whose other end carries G under the label vector h."""
    isg = (h == c.G).astype(np.int64)
    return (np.bincount(c.s, weights=isg[c.d], minlength=c.V) + np.bincount(c.d, weights=isg[c.s], minlength=c.V)).astype(np.int64)


def _majority_rows(V, s, d, G, degrees):
    """One more row per degree, which superstep 3 must settle: G on d // 2 + 1 of ALL its arcs (tie_rows'
    own tables fall short of that by their two blinker arcs; its only settled hub row is the G anchor's).
    Those arcs go to tie_rows' G-mass vertices (two parallel edges to G each: on G from superstep 1 on
    with one row's arc on them), the others to leaves of a new anchor X (200 self-loops), eight
    parallel arcs per leaf (few leaves: G keeps half of the slots); each leaf is on 200 parallel edges to
    X, so the rows that share it never outvote X.  -> V, src, dst, row ids, X"""
    deg = np.bincount(s, minlength=V) + np.bincount(d, minlength=V)
    to_g = np.bincount(s[d == G], minlength=V)
    mass = np.flatnonzero((deg == 2) & (to_g == 2))
    n_g, n_x = sum(dg // 2 + 1 for dg in degrees), -(-max(degrees) // 16)
    assert mass.size >= n_g, mass.size   # a mass vertex takes one row: two rows with one label would outvote G
    X = V
    leaves = np.arange(V + 1, V + 1 + n_x)
    rows = np.arange(leaves[-1] + 1, leaves[-1] + 1 + len(degrees))
    es = [s, np.full(200, X), np.repeat(leaves, 200)]
    ed = [d, np.full(200, X), np.full(200 * n_x, X)]
    m0 = 0
    for r, dg in zip(rows, degrees):
        g = dg // 2 + 1
        es += [np.full(dg, r)]
        ed += [mass[m0:m0 + g], np.repeat(leaves, 8)[:dg - g]]
        m0 += g
    return int(rows[-1]) + 1, np.concatenate(es).astype(np.int32), np.concatenate(ed).astype(np.int32), rows, X


def _build_hubs(oracle):
    c = Case()
    V0, s0, d0, rows, c.G = tie_rows(degrees=HUB_DEGREES)
    c.V, c.s, c.d, c.major, c.X = _majority_rows(V0, s0, d0, c.G, HUB_DEGREES)
    c.steps = STEPS
    _, c.hist, _ = oracle.lpa(c.V, c.s, c.d, STEPS, per_iter=True)
    c.hist.setflags(write=False)
    c.deg = np.bincount(c.s, minlength=c.V) + np.bincount(c.d, minlength=c.V)
    L2, L3 = c.hist[1], c.hist[2]
    # G worth trying in superstep 3: it holds at least 1/5 of the K_PICK highest-degree slots of L2 ...
    top = np.argsort(-c.deg, kind="stable")[:K_PICK]
    lab, cnt = np.unique(L2[top], return_counts=True)
    assert int(lab[cnt == cnt.max()].min()) == c.G and 5 * int(cnt.max()) >= K_PICK, (lab, cnt)
    # ... and superstep 2's refresh is a bits-mode rebuild: G on at least half of the slots of L1 and L2
    for step in (1, 2):
        assert 2 * int((c.hist[step - 1] == c.G).sum()) >= c.V, step
    g2 = _g_arcs(c, L2)
    # The engineered rows of depth <= 2 see their table at L2.  z_half_pure at an even degree: G on exactly
    # half of ALL arcs -- the strict test's equality -- and the smaller rival A wins the tie, so a row
    # settled by one bit too many gets the wrong label; at an odd degree A is one ahead
    A = tie_anchor_ids()["A"]
    pure = [r for r, depth, tab in rows if depth <= 2 and set(tab) == {c.G, A} and c.deg[r] == tab[c.G] + tab[A]]
    # (tie_rows builds them up to 32,768 arcs)
    assert sorted({int(c.deg[r]) for r in pure}) == [d for d in HUB_DEGREES if d <= 32768], pure
    for r in pure:
        d = int(c.deg[r])
        assert int(g2[r]) == d // 2 and int(L3[r]) == A, (r, int(g2[r]), d, int(L3[r]))
    # half + 1 of the engineered votes: b_tie_hi at an odd vote count n = d - 2 has G one above C, the
    # row's two blinker arcs off G -- G is the mode on (n + 1) / 2 < d / 2 arcs: not settled, tallied
    C = tie_anchor_ids()["C"]
    plus = [r for r, depth, tab in rows if depth <= 2 and set(tab) == {c.G, C} and tab[c.G] == tab[C] + 1]
    assert sorted({int(c.deg[r]) for r in plus}) == [d for d in HUB_DEGREES if d % 2 == 1], plus
    for r in plus:
        assert 2 * int(g2[r]) < c.deg[r] and int(L3[r]) == c.G, (r, int(g2[r]), int(c.deg[r]), int(L3[r]))
    # half + 1 of ALL arcs (_majority_rows): settled on G at every degree, the other arcs on X
    assert [int(c.deg[r]) for r in c.major] == list(HUB_DEGREES)
    other = c.deg - g2 - _g_arcs(c, np.where(L2 == c.X, c.G, c.G + 1))   # arcs on neither G nor X
    for r in c.major:
        assert int(g2[r]) == c.deg[r] // 2 + 1 and other[r] == 0 and L3[r] == c.G, (r, int(g2[r]), int(other[r]))
    # hub rows on both sides of the settle; the G anchor's row settles, and is longer than two double steps
    hub = c.deg > 1024
    settled = hub & (2 * g2 > c.deg)
    assert settled[c.major].all() and int(settled.sum()) >= 1 + len(HUB_DEGREES)
    assert settled[c.G] and c.deg[c.G] > 4 * STEP, (bool(settled[c.G]), int(c.deg[c.G]))
    assert 0 < int(settled.sum()) < int(hub.sum())
    # a row of more than 512 units (k_hub_small's long word count) and one of more than 1024
    assert int(c.deg.max()) > 1024 * 512
    print(f"hub rows {int(hub.sum())}, settled at L2 {int(settled.sum())}, G row {int(c.deg[c.G])} arcs, "
          f"arcs {int(c.deg.sum())}")
    return c


@pytest.fixture(scope="module")
def hubs(oracle):
    return _build_hubs(oracle)


@pytest.mark.parametrize("env", SCHEDULES, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_hub_degrees_bit_exact(gfa, hubs, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = hubs
    with gfa.Graph(c.s, c.d, c.V) as g:
        for step in range(1, c.steps + 1):
            g.step(1)
            _check(c, g.labels(), step, f"hub degrees {env}")
