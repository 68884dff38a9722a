"""Wall times of lpa_scan beside lpa_triangle_count on the same handle (DESIGN.md "SCAN structural
clustering"): the triangle count walks the same oriented lists and finds the same matches without
the per-edge atomics.

    python tools/scan_time.py --graph r9
    python tools/scan_time.py --graph sbm            # bench.py's C2 shape
    python tools/scan_time.py --graph rmat --scale 20 --edgefactor 16
    python tools/scan_time.py --graph rmat --scale 11 --reference   # + the set-based CPU reference, and equality

Host clock around the blocking calls after a warm-up.  `scan_common_ms` is the call that also
reports the common neighbours per input row (the second sort then carries a payload).  One JSON
line.
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
    ap.add_argument("--eps", type=float, default=0.5)
    ap.add_argument("--mu", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", action="store_true", help="also time tests/scan_ref.py and compare")
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
    rep = dict(graph=args.graph, V=V, m=int(s.numel() if hasattr(s, "numel") else s.size), eps=args.eps, mu=args.mu)
    with gfa.Graph(s, d, V) as g:
        g.scan(args.eps, args.mu)   # warm-up: code objects, the stream-ordered pool
        (label, role, nsim, summ), rep["scan_ms"] = clock(lambda: g.scan(args.eps, args.mu, stats=True), args.reps)
        res, rep["scan_common_ms"] = clock(lambda: g.scan(args.eps, args.mu, common=True), args.reps)
        common = res[2]
        g.triangle_count()
        _, rep["triangle_count_ms"] = clock(lambda: g.triangle_count(), args.reps)
        rep["summary"] = summ
    if args.reference:
        import scan_ref

        hs, hd = (s.cpu().numpy(), d.cpu().numpy()) if hasattr(s, "cpu") else (s, d)
        t = time.perf_counter()
        prep = scan_ref.prepare(V, hs, hd)
        rlabel, rrole, rnsim, rsumm = scan_ref.scan(prep, args.eps, args.mu)
        rep["reference_s"] = round(time.perf_counter() - t, 3)
        rep["equal"] = bool(np.array_equal(label, rlabel) and np.array_equal(role, rrole) and
                            np.array_equal(nsim, rnsim) and np.array_equal(common, prep.common_rows) and
                            summ == rsumm)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
