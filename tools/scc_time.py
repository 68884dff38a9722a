"""Time Graph.strongly_connected_components() (lpa_strongly_connected_components), converged.

    python tools/scc_time.py --graph rmat --scale 20 --edgefactor 16 [--warmup 2] [--calls 5]
    python tools/scc_time.py --graph r9
    python tools/scc_time.py --graph paths --width 256 --depth 2000 --blocks 0,4096

Host wall clock around the blocking call, components written into a device tensor.  One JSON
line per LPA_SCC_BLOCK value of --blocks (each on a handle of its own: the value is read when
the handle is created; the timed calls alternate between the handles): median / min / max ms,
the summary, and for context the same handle's lpa_components time.  The results of all the
handles are compared: they must be identical.

--graph paths: `width` disjoint directed paths of `depth` vertices, everything is trimmed in
depth / 2 levels of 2 * width vertices -- the graph on which the in-block trim's switch size
(kSccBlockTrim) was chosen: a level of n vertices in the block (--blocks 4096) against a
launch per row form and a host read of the tails (--blocks 0).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphframes_amd as gfa  # noqa: E402
import torch  # noqa: E402


def paths(width, depth):
    v = np.arange(width * depth, dtype=np.int64).reshape(width, depth)
    return width * depth, v[:, :-1].ravel().astype(np.int32), v[:, 1:].ravel().astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=("rmat", "r9", "paths"), default="rmat")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--depth", type=int, default=2000)
    ap.add_argument("--blocks", default="", help="comma-separated LPA_SCC_BLOCK values (default: the library's)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    if a.graph == "rmat":
        V = 1 << a.scale
        src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
        m = int(src.numel())
    elif a.graph == "r9":
        z = np.load(os.path.join(ROOT, "tests", "golden", "r9_golden.npz"), allow_pickle=False)
        V, src, dst = int(z["ids"].size), z["src"], z["dst"]
        m = int(src.size)
    else:
        V, src, dst = paths(a.width, a.depth)
        m = int(src.size)
    blocks = [b for b in a.blocks.split(",") if b != ""] or [None]
    handles = []
    for b in blocks:
        if b is None:
            os.environ.pop("LPA_SCC_BLOCK", None)
        else:
            os.environ["LPA_SCC_BLOCK"] = b
        handles.append(gfa.Graph(src, dst, V))
    os.environ.pop("LPA_SCC_BLOCK", None)
    del src, dst
    torch.cuda.empty_cache()
    out = torch.empty(V, dtype=torch.int32, device="cuda:0")
    ms = [[] for _ in handles]
    cc = [[] for _ in handles]
    for k in range(a.warmup + a.calls):
        for i, g in enumerate(handles):
            t0 = time.perf_counter()
            g.strongly_connected_components(out=out)
            t1 = time.perf_counter()
            g.components(out=out)
            t2 = time.perf_counter()
            if k >= a.warmup:
                ms[i].append(1e3 * (t1 - t0))
                cc[i].append(1e3 * (t2 - t1))
    first = None
    for i, g in enumerate(handles):
        comp, _, summ = g.strongly_connected_components(out=out, sizes=True)
        comp = comp.cpu().numpy()
        if first is None:
            first = (comp, summ)
        elif not np.array_equal(comp, first[0]) or summ != first[1]:
            raise AssertionError(f"LPA_SCC_BLOCK={blocks[i]} gives another result than {blocks[0]}")
        g.close()
        print(json.dumps(dict(
            tool="scc_time", graph=a.graph, V=V, m=m, scc_block=blocks[i], calls=a.calls,
            width=a.width if a.graph == "paths" else None, level=2 * a.width if a.graph == "paths" else None,
            median_ms=round(statistics.median(ms[i]), 3), min_ms=round(min(ms[i]), 3), max_ms=round(max(ms[i]), 3),
            components_median_ms=round(statistics.median(cc[i]), 3), **summ)), flush=True)


if __name__ == "__main__":
    main()
