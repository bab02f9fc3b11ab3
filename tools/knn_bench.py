"""Nearest neighbours on the GPU: ``embed.KnnIndex.query`` (exact float64, ordered ties) against what a user can do without it,
``torch.topk(Xn @ Qn.T, topn)`` in float64 (the same arithmetic width) and in float32 (for scale only: not reproducible, ties
unordered), on random float32 vectors of the RMAT-18 embedding's shape.  The three run in one process, alternating; the
first round is a warm-up; every timing is wall clock around a device synchronisation.

    python tools/knn_bench.py [--n 262144] [--dim 128] [--nq 4096] [--topn 10] [--repeats 3] [--all_rows]

One JSON line per query count: median / min / max seconds of each route, the score kernel's FMA rate (n * nq * dim over its
HIP-event time) and its share of the float64 vector spec rate (78.6 TFLOP/s = 39.3e12 FMA/s)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPEC_FMA_PER_S = 39.3e12
CHUNK = 4096   # queries per matmul of the torch routes: the score matrix of a chunk is n * 4096 values


def torch_route(Xn, Qn, topn, dtype):
    import torch

    Xd = Xn.to(dtype)
    out = []
    for lo in range(0, Qn.shape[0], CHUNK):
        s = Qn[lo:lo + CHUNK].to(dtype) @ Xd.T
        out.append(torch.topk(s, topn, dim=1))
        del s
    return out


def main():
    import torch

    from pecanpy_amd.embed import KnnIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--topn", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--all_rows", action="store_true", help="also query every row")
    args = ap.parse_args()

    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((args.n, args.dim), generator=g, device="cuda", dtype=torch.float32)
    Xn = X / X.norm(dim=1, keepdim=True)   # the torch routes score normalised rows; the index normalises by its own norms
    t0 = time.perf_counter()
    index = KnnIndex(X)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for nq in [args.nq] + ([args.n] if args.all_rows else []):
        rows = torch.arange(nq, device="cuda")
        Qn = Xn[:nq]
        routes = {
            "knn_index": lambda: index.query(rows=rows, topn=args.topn, exclude_self=False),
            "torch_f64": lambda: torch_route(Xn, Qn, args.topn, torch.float64),
            "torch_f32": lambda: torch_route(Xn, Qn, args.topn, torch.float32),
        }
        times = {k: [] for k in routes}
        kernel_ms = []
        for rep in range(args.repeats + 1):   # round 0 warms up
            for name, fn in routes.items():
                dt = timed(fn)
                if rep:
                    times[name].append(dt)
                    if name == "knn_index":
                        kernel_ms.append(index.last_stats["score_ms"])
        rec = {"n": args.n, "dim": args.dim, "nq": nq, "topn": args.topn, "repeats": args.repeats, "index_build_s": round(build_s, 4)}
        for name, ts in times.items():
            rec[name] = {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}
        rate = args.n * nq * args.dim / (statistics.median(kernel_ms) * 1e-3)
        rec["score_kernel_ms"] = round(statistics.median(kernel_ms), 3)
        rec["merge_ms"] = round(index.last_stats["merge_ms"], 3)
        rec["fma_per_s"] = float(f"{rate:.4g}")
        rec["share_of_spec"] = round(rate / SPEC_FMA_PER_S, 4)
        rec["stats"] = index.last_stats
        print(json.dumps(rec), flush=True)
    index.close()


if __name__ == "__main__":
    main()
