"""bench.py's plain run and --dump-outputs: a plain run prints the headline keys only
(the extra measurements sit behind --full), and the dump holds the labels that the
last timed labelPropagation(maxIter=10) call left, as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
# keys whose measurement takes runs of its own: --full only
FULL_ONLY = {"baseline_method", "run_maxiter10_ms", "roofline", "roofline_tally", "iteration_roofline",
             "moved_bytes_frac", "kernel_ms_per_step", "outlier_l1_ms", "cpu_baseline", "quality"}


def _load(d):
    return {n: np.load(os.path.join(d, f"labels{n}.npy")) for n in ("", "_index", "_summary")}


def test_dump_outputs_whole_vector(tmp_path):
    import bench

    lab = np.array([3, 3, 0, 7, 7, 7, 2], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "o"), lab)
    z = _load(tmp_path / "o")
    assert all(a.dtype == np.float64 for a in z.values())
    assert np.array_equal(z[""], lab) and np.array_equal(z["_index"], np.arange(7))
    assert z["_summary"].tolist() == [7, 4, 29]


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    import bench

    V = bench.DUMP_SAMPLE + 12345   # the smallest kind of size that takes the sampled path
    lab = (np.arange(V, dtype=np.int64) * 7919 % V).astype(np.int32)
    bench.dump_outputs(str(tmp_path / "a"), lab)
    bench.dump_outputs(str(tmp_path / "b"), lab)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)          # the same sample every run
    idx = a["_index"].astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and idx.min() >= 0 and idx.max() < V
    assert np.array_equal(a[""], lab[idx])
    assert a["_summary"].tolist() == [V, V, V * (V - 1) // 2]   # 7919 is coprime to V: a permutation
    total = sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000


@pytest.mark.gpu
def test_plain_run_headline_only_and_dumps_last_step_labels(tmp_path):
    """R-MAT scale 16 (65536 vertices: the whole vector is dumped), 2 timed steps."""
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "16", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert HEADLINE <= set(res) and not FULL_ONLY & set(res), sorted(res)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["unit"] == "GTEPS" and res["dtype"] == "int32"
    assert res["ms_per_step"] > 0 and res["value"] > 0
    # value and ms_per_step describe the same window: m * 9 supersteps per step
    assert res["value"] == pytest.approx(res["config"]["edges"] * 9 / (res["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)

    import bench
    import graphframes_amd as gfa

    cfg = dict(bench.CONFIGS["C3"], scale=16)
    s, d, V = bench.make_edges(gfa, cfg, 0)
    with gfa.Graph(s, d, V) as g:
        want = g.run(bench.MAX_ITER)
    z = _load(out)
    assert np.array_equal(z["_index"], np.arange(V)) and np.array_equal(z[""], want)
    assert z["_summary"].tolist() == [V, np.unique(want).size, int(want.sum(dtype=np.int64))]
