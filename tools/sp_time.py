"""Time Graph.shortest_paths() (lpa_shortest_paths) on an R-MAT graph generated in HBM.

    python tools/sp_time.py --scale 24 --edgefactor 16 [--landmarks 64] [--warmup 1] [--calls 5] [--ref]

Host wall clock around the blocking call, distances written into a device tensor.  The
landmarks are the vertices of highest in-degree.  A call is the build (keys, sort, the two
CSRs, the pull's lists) plus one pass per batch of 64 landmarks, so the split is taken from
two call lengths: the landmark list once and the same list twice (equal rows, twice the
passes): per pass set = t(twice) - t(once), build = t(once) - per pass set (medians over
--calls calls, alternating the two lengths).  "landmark_arcs_per_s" is landmarks x arcs / the
pass time: the arcs a search per landmark would have to look at, the usual aggregate rate of
a multi-source search.  The same is measured under each schedule: the default switch,
LPA_SP_ALPHA=0 (push only) and LPA_SP_PULL=1 (pull only), each on a handle of its own (the
overrides are read when a handle is created); distances are compared across the three.
--ref also times the numpy reference of the test suite (tests/sp_ref.py) on the same edges, on
this host's CPU, and compares exactly.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphframes_amd as gfa  # noqa: E402
import torch  # noqa: E402

SCHEDULES = (("default", {}), ("push_only", {"LPA_SP_ALPHA": "0"}), ("pull_only", {"LPA_SP_PULL": "1"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--landmarks", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--schedules", default="default,push_only,pull_only")
    ap.add_argument("--ref", action="store_true")
    a = ap.parse_args()
    V = 1 << a.scale
    n = a.landmarks
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    res = dict(tool="sp_time", scale=a.scale, edgefactor=a.edgefactor, V=V, landmarks=n, calls=a.calls, schedules={})
    out = torch.empty((2 * n, V), dtype=torch.int32, device="cuda:0")
    lms = first = None
    for name, env in SCHEDULES:
        if name not in a.schedules.split(","):
            continue
        for key, val in env.items():
            os.environ[key] = val
        g = gfa.Graph(src, dst, V)
        for key in env:
            del os.environ[key]
        if lms is None:
            rank = torch.empty(V, dtype=torch.float64, device="cuda:0")
            _, _, indeg, _ = g.pagerank(1, out=rank, stats=True)
            lms = torch.topk(indeg, n).indices.cpu().numpy().astype("int32")
            del rank, indeg
        lists = {1: lms, 2: list(lms) * 2}
        for _ in range(a.warmup):
            for k in (1, 2):
                g.shortest_paths(lists[k], out=out[:k * n])
        ms = {1: [], 2: []}
        for _ in range(a.calls):
            for k in (1, 2):
                t0 = time.perf_counter()
                g.shortest_paths(lists[k], out=out[:k * n])
                ms[k].append(1e3 * (time.perf_counter() - t0))
        _, summ = g.shortest_paths(lms, out=out[:n], stats=True)
        g.close()
        got = out[:n].clone()
        if first is None:
            first = got
        med = {k: statistics.median(v) for k, v in ms.items()}
        per_set = med[2] - med[1]
        batches = summ["batches"]
        res["schedules"][name] = dict(
            call_ms=round(med[1], 3), call_min_ms=round(min(ms[1]), 3), call_max_ms=round(max(ms[1]), 3),
            passes_ms=round(per_set, 3), per_batch_ms=round(per_set / batches, 3), build_ms=round(med[1] - per_set, 3),
            landmark_arcs_per_s=round(n * summ["arcs"] / (per_set * 1e-3), 1), same_as_first=bool(torch.equal(got, first)),
            **summ)
    if a.ref:
        print(json.dumps(dict(res, note="GPU done, numpy reference running")), flush=True)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import sp_ref

        s, d = src.cpu().numpy(), dst.cpu().numpy()
        t0 = time.perf_counter()
        ref = sp_ref.shortest_paths(V, s, d, lms)
        res["ref_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["ref_equal"] = bool((first.cpu().numpy() == ref).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
