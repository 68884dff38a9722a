"""Time Graph.triangle_count() (lpa_triangle_count) on an R-MAT graph generated in HBM.

    python tools/tc_time.py --scale 20 --edgefactor 16 [--warmup 1] [--calls 5] [--scipy]

Host wall clock around the blocking call, counts written into a device tensor.  Prints one
JSON line: median / min / max ms and the call's summary.  --scipy also times the CPU
reference of the test suite (tests/tc_ref.py, sparse matrix products) on the same edges and
checks that the two results are equal; it prints a progress line first, because the
reference can take minutes where the graph has hubs.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scipy", action="store_true")
    a = ap.parse_args()
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    m = int(src.numel())
    edges = (src.cpu().numpy(), dst.cpu().numpy()) if a.scipy else None
    g = gfa.Graph(src, dst, V)
    del src, dst
    torch.cuda.empty_cache()
    out = torch.empty(V, dtype=torch.int64, device="cuda:0")
    for _ in range(a.warmup):
        g.triangle_count(out=out)
    ms = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        g.triangle_count(out=out)
        ms.append(1e3 * (time.perf_counter() - t0))
    _, _, summ = g.triangle_count(out=out, stats=True)
    g.close()
    res = dict(tool="tc_time", scale=a.scale, edgefactor=a.edgefactor, V=V, m=m, calls=a.calls,
               median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), **summ)
    if a.scipy:
        print(json.dumps(dict(res, note="GPU done, scipy reference running")), flush=True)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import tc_ref

        t0 = time.perf_counter()
        last = [t0]

        def progress(rows, total):   # a line every half minute: the reference runs for minutes on hubs
            if time.perf_counter() - last[0] > 30:
                last[0] = time.perf_counter()
                print(f"scipy reference: {rows} of {total} rows, {last[0] - t0:.0f} s", flush=True)

        rcount, _ = tc_ref.triangles(V, *edges, progress=progress)
        res["scipy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["equal_to_scipy"] = bool((out.cpu().numpy() == rcount).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
