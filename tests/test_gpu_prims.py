"""The build primitives every graph build rests on (csrc/lpa_prims.hip: radix_sort_u64 / _kv and the
three exclusive scans) and the shared edge-list builds (csrc/lpa_adj.hip: arcs_count / arcs_lists,
simple_edges, key_bounds / key_col, form_lists, comp_sizes), called directly and compared with plain
host references at the sizes where their code changes path: around a wave, a block and a tile of 4096
elements, across scan levels, at the radix pass boundaries of V and past the block histograms' grid
cap.  The algorithm tests see them only through finished results at whatever sizes their graphs have;
here a wrong rank inside a wave or a lost carry between tiles is named by case and index
(tools/microbench/prims_check.hip, built by the csrc Makefile; one fresh process per group).  Not
covered yet: an edge list past the grid-stride kernels' 2^24-thread grid ("Open")."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "lpa_hip", "prims_check")

# seconds: about ten times a group's wall time on one MI355X (scan 1.6, sort 4.1, adj 1.0, mostly the
# host references); the margin is for a shared machine, the limit only ends a hang
TIMEOUT = {"scan": 15, "sort": 40, "adj": 10}


def _run(group):
    if not os.path.exists(CHECK):
        pytest.fail(f"{CHECK} missing: run __graft_entry__.build() (csrc Makefile target)")
    r = subprocess.run([CHECK, group], capture_output=True, text=True, timeout=TIMEOUT[group])
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"prims_check {group}: ok (" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_scans_match_running_sum():
    _run("scan")


@pytest.mark.gpu
def test_radix_sorts_match_stable_sort():
    _run("sort")


@pytest.mark.gpu
def test_edge_list_builds_match_host_lists():
    _run("adj")
