"""Wall times of lpa_core_numbers beside its own build (max_k = 0) and lpa_triangle_count on the same
handle (DESIGN.md "k-core decomposition").

    python tools/kcore_time.py --graph r9
    python tools/kcore_time.py --graph sbm            # bench.py's C2 shape
    python tools/kcore_time.py --graph rmat --scale 20 --edgefactor 16
    python tools/kcore_time.py --graph rmat --scale 16 --reference   # + the vectorised CPU reference, and equality

Host clock around the blocking calls after a warm-up.  `build_ms` is the call with max_k = 0: the
sort-based build of the simple graph alone, which triangle_count shares; the peel is the
difference.  `summary.passes` is the peel's host round trips.  One JSON line.
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
    ap.add_argument("--reference", action="store_true", help="also time tests/kcore_ref.py and compare")
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
        g.core_numbers()   # warm-up: code objects, the stream-ordered pool
        (core, deg, summ), rep["core_numbers_ms"] = clock(lambda: g.core_numbers(stats=True), args.reps)
        _, rep["build_ms"] = clock(lambda: g.core_numbers(max_k=0), args.reps)
        rep["peel_ms"] = round(min(rep["core_numbers_ms"]) - min(rep["build_ms"]), 3)
        g.triangle_count()
        _, rep["triangle_count_ms"] = clock(lambda: g.triangle_count(), args.reps)
        rep["summary"] = summ
        rep["core1"] = int((core == 1).sum())
    if args.reference:
        import kcore_ref

        hs, hd = (s.cpu().numpy(), d.cpu().numpy()) if hasattr(s, "cpu") else (s, d)
        t = time.perf_counter()
        rcore, rdeg = kcore_ref.core_numbers(V, hs, hd)
        rep["reference_s"] = round(time.perf_counter() - t, 3)
        rsumm = kcore_ref.summary_of(rcore, rdeg)
        rep["equal"] = bool(np.array_equal(core, rcore) and np.array_equal(deg, rdeg) and
                            all(summ[k] == rsumm[k] for k in kcore_ref.PURE_KEYS))
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
