"""Time Graph.betweenness() (lpa_betweenness) at every batch width on an R-MAT graph generated in HBM.

    python tools/bc_time.py --scale 20 --edgefactor 16 --pivots 256 [--warmup 1] [--calls 3] [--directed]

The pivots are the documented draw of GraphFrame.betweennessCentrality(k=pivots, seed=seed); the
graph is undirected unless --directed.  Host wall clock around the blocking call (it ends in a
stream synchronise), the result written into one device tensor that lives across the calls.  The
widths 1, 4, 8 and 16 take turns inside every round, so that a drift of the machine falls on all
of them alike: --warmup rounds are thrown away, then the median, smallest and largest of --calls
rounds.  "ms_per_source" is the median over the pivots, "pass_ms" the median over the passes;
"arcs_per_s" counts the distinct arcs once per source and direction of the sweep (2 arcs sources /
time: every source walks every arc it reaches forward and backward).  The results of all widths
are compared bit for bit with the first.  Prints one JSON line.
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

WIDTHS = (1, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--pivots", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--directed", action="store_true")
    ap.add_argument("--widths", default=",".join(str(w) for w in WIDTHS))
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(",")]
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    S = np.sort(np.random.default_rng(a.seed).choice(V, size=a.pivots, replace=False)).astype(np.int32)
    res = dict(tool="bc_time", scale=a.scale, edgefactor=a.edgefactor, V=V, m=int(src.numel()), pivots=a.pivots,
               directed=bool(a.directed), calls=a.calls, warmup=a.warmup)
    g = gfa.Graph(src, dst, V)
    out = torch.empty(V, dtype=torch.float64, device="cuda:0")
    ms = {w: [] for w in widths}
    first, same, summ = None, {}, {}
    for it in range(a.warmup + a.calls):
        for w in widths:
            t0 = time.perf_counter()
            _, summ[w] = g.betweenness(S, directed=a.directed, batch=w, out=out, stats=True)
            ms[w].append(1e3 * (time.perf_counter() - t0))
            if it == 0:
                raw = out.cpu().numpy()
                if first is None:
                    first = raw
                same[w] = bool(np.array_equal(raw, first))
    g.close()
    rows = {}
    for w in widths:
        t = ms[w][a.warmup:]
        med = statistics.median(t)
        rows[str(w)] = dict(call_ms=round(med, 2), call_min_ms=round(min(t), 2), call_max_ms=round(max(t), 2),
                            ms_per_source=round(med / a.pivots, 3), pass_ms=round(med / summ[w]["batches"], 2),
                            arcs_per_s=round(2.0 * summ[w]["arcs"] * a.pivots / (med * 1e-3), 1),
                            same_as_first=same[w], **summ[w])
    res["widths"] = rows
    res["nonzero"] = int((first > 0).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
