"""Time Graph.components() (lpa_components) on an R-MAT graph generated in HBM.

    python tools/cc_time.py --scale 24 --edgefactor 16 [--warmup 3] [--calls 10]

Host wall clock around the blocking call, components written into a device tensor.
Prints one JSON line: median / min / max ms, the algorithmic floor 8 m + 12 V bytes (edge
read + parent init + comp write) and the fraction of 8 TB/s the median reaches on that
floor, and for context the same handle's lpa_run(5) device time.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphframes_amd as gfa  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    m = int(src.numel())
    g = gfa.Graph(src, dst, V)
    del src, dst
    torch.cuda.empty_cache()
    out = torch.empty(V, dtype=torch.int32, device="cuda:0")
    for _ in range(a.warmup):
        g.components(out=out)
    ms = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        g.components(out=out)
        ms.append(1e3 * (time.perf_counter() - t0))
    _, _, summ = g.components(out=out, sizes=True)
    _, st = g.run(5, stats=True)
    g.close()
    floor = 8 * m + 12 * V
    med = statistics.median(ms)
    print(json.dumps(dict(
        tool="cc_time", scale=a.scale, edgefactor=a.edgefactor, V=V, m=m, calls=a.calls,
        median_ms=round(med, 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
        floor_bytes=floor, floor_fraction_of_8TBps=round(floor / (med * 1e-3) / PEAK_BYTES_PER_S, 4),
        lpa_run5_total_ms=round(st["total_ms"], 3), **summ)))


if __name__ == "__main__":
    main()
