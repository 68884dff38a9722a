"""Wall times of lpa_louvain beside lpa_run(10) on the same handle (DESIGN.md "Louvain").

    python tools/louvain_time.py --graph r9
    python tools/louvain_time.py --graph sbm            # bench.py's C2 shape
    python tools/louvain_time.py --graph rmat --scale 20 --edgefactor 16
    python tools/louvain_time.py --graph rmat --scale 16 --reference   # + the vectorised CPU reference, and equality

Host clock around the blocking calls after a warm-up.  `cumulative_ms_by_max_levels[L - 1]` is a
call stopped by max_levels = L (it skips the build of level L + 1).  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clock(fn, reps):
    import torch

    ts = []
    out = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        ts.append(round(1e3 * (time.perf_counter() - t), 3))
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["r9", "sbm", "rmat"], default="r9")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", action="store_true", help="also time tests/louvain_ref.py and compare")
    args = ap.parse_args()
    import graphframes_amd as gfa

    if args.graph == "r9":
        z = np.load(os.path.join(ROOT, "tests", "golden", "r9_golden.npz"))
        s, d, V = z["src"], z["dst"], int(z["ids"].size)
    elif args.graph == "sbm":
        V = 1_000_000
        s, d = gfa.gen_sbm(V, 100, 20_000_000, seed=20261015)
    else:
        V = 1 << args.scale
        s, d = gfa.gen_rmat(args.scale, args.edgefactor, seed=1)
    rep = dict(graph=args.graph, V=V, m=int(s.numel() if hasattr(s, "numel") else s.size))
    with gfa.Graph(s, d, V) as g:
        g.louvain()   # warm-up: code objects, the stream-ordered pool
        (comm, _, levels, summ), rep["louvain_ms"] = clock(lambda: g.louvain(stats=True), args.reps)
        rep["levels"], rep["summary"] = levels, summ
        rep["cumulative_ms_by_max_levels"] = [min(clock(lambda: g.louvain(max_levels=L), 2)[1])
                                              for L in range(1, len(levels) + 1)]
        g.run(10)
        lab, rep["lpa_run10_ms"] = clock(lambda: g.run(10), args.reps)
        q = g.quality(lab)
        rep["lpa_run10_quality"] = dict(n_communities=q["n_communities"], modularity=q["modularity"])
    if args.reference:
        import louvain_ref

        hs, hd = (s.cpu().numpy(), d.cpu().numpy()) if hasattr(s, "cpu") else (s, d)
        t = time.perf_counter()
        rcomm, rlevels, rsumm = louvain_ref.louvain(V, hs, hd)
        rep["reference_s"] = round(time.perf_counter() - t, 3)
        rep["equal"] = bool(np.array_equal(comm, rcomm) and levels == rlevels and
                            all(summ[k] == rsumm[k] for k in louvain_ref.SUMMARY_KEYS[:-1]))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
