"""Time Graph.pagerank() (lpa_pagerank) on an R-MAT graph generated in HBM.

    python tools/pagerank_time.py --scale 24 --edgefactor 16 [--iters 10] [--warmup 1] [--calls 5] [--ref]

Host wall clock around the blocking call, ranks written into a device tensor.  A call is
the build (keys, sort, rows, lists) plus max_iter supersteps plus the finish, so the split is
taken from two call lengths: per iteration = (t(1 + iters) - t(1)) / iters, build and finish
= t(1) - per iteration (medians over --calls calls, alternating the two lengths).  Beside
the per-iteration time it prints the algorithmic bytes of a superstep, 12 m + 32 V (a 4-byte
column and an 8-byte gather per kept edge; the r, c, w streams and the row offsets per
vertex), and the fraction of the 8 TB/s HBM peak that rate is.  --ref also times the numpy
reference of the test suite (tests/pr_ref.py) on the same edges, on this host's CPU, and
reports the largest relative difference against pr_ref.bound.  Prints one JSON line.
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

HBM_PEAK = 8e12   # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ref", action="store_true")
    a = ap.parse_args()
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    edges = (src.cpu().numpy(), dst.cpu().numpy()) if a.ref else None
    g = gfa.Graph(src, dst, V)
    del src, dst
    torch.cuda.empty_cache()
    out = torch.empty(V, dtype=torch.float64, device="cuda:0")
    lengths = (1, 1 + a.iters, a.iters)
    for _ in range(a.warmup):
        for k in lengths:
            g.pagerank(k, out=out)
    ms = {k: [] for k in lengths}
    for _ in range(a.calls):
        for k in lengths:
            t0 = time.perf_counter()
            g.pagerank(k, out=out)
            ms[k].append(1e3 * (time.perf_counter() - t0))
    _, _, _, summ = g.pagerank(a.iters, out=out, stats=True)
    g.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    per_iter = (med[1 + a.iters] - med[1]) / a.iters
    m = summ["edges"]
    it_bytes = 12 * m + 32 * V
    res = dict(tool="pagerank_time", scale=a.scale, edgefactor=a.edgefactor, V=V, iters=a.iters, calls=a.calls,
               call_ms=round(med[a.iters], 3), call_min_ms=round(min(ms[a.iters]), 3),
               call_max_ms=round(max(ms[a.iters]), 3), one_iter_call_ms=round(med[1], 3),
               per_iter_ms=round(per_iter, 4), build_finish_ms=round(med[1] - per_iter, 3), iter_bytes=it_bytes,
               iter_tb_per_s=round(it_bytes / (per_iter * 1e-3) / 1e12, 3),
               frac_of_hbm_peak=round(it_bytes / (per_iter * 1e-3) / HBM_PEAK, 4), **summ)
    if a.ref:
        print(json.dumps(dict(res, note="GPU done, numpy reference running")), flush=True)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import pr_ref

        t0 = time.perf_counter()
        rrank, _, rindeg, _ = pr_ref.pagerank(V, *edges, a.iters)
        res["ref_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        got = out.cpu().numpy()
        res["worst_rel_diff"] = float((abs(got - rrank) / rrank).max())
        res["bound"] = pr_ref.bound(a.iters, int(rindeg.max()), V)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
