"""Link prediction on the GPU: the three calls of ``pecanpy_amd.linkpred`` (exact by written definitions) beside the plain
torch statement of each on the same device -- not reproducible bit for bit, for scale only.

    python tools/linkpred_bench.py [--n 262144] [--dim 128] [--pairs 10000000] [--scale 18] [--repeats 3]

  pair scores   ``KnnIndex.score_pairs(u, v, "dot")``   /  ``(X[u].double() * X[v].double()).sum(1)``
  AUC           ``linkpred.auc(pos, neg)``              /  ``torch.sort`` + two ``torch.searchsorted``
  sampler       ``g.sample_non_edges(pairs, seed)``     /  ``torch.randint`` + a ``searchsorted`` membership test on the edge keys
The routes of a call alternate in one process; the first round is a warm-up; every timing is wall clock around a device
synchronisation.  One JSON line per call: median / min / max seconds of each route; for the pair kernel the bytes it must read
(pairs * 2 * dim * 4) over its time and their share of the HBM peak (8.0 TB/s)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def main():
    import torch

    from pecanpy_amd import linkpred
    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.embed import KnnIndex
    from pecanpy_amd.synth import rmat_csr

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    m = args.pairs

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def compare(what, routes, extra=None):
        times = {k: [] for k in routes}
        for rep in range(args.repeats + 1):   # round 0 warms up
            for name, fn in routes.items():
                dt = timed(fn)
                if rep:
                    times[name].append(dt)
        rec = {"call": what, "pairs": m, "repeats": args.repeats}
        for name, ts in times.items():
            rec[name] = {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}
        if extra:
            rec.update(extra(rec))
        print(json.dumps(rec), flush=True)

    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((args.n, args.dim), generator=g, device="cuda", dtype=torch.float32)
    u = torch.randint(0, args.n, (m,), generator=g, device="cuda")
    v = torch.randint(0, args.n, (m,), generator=g, device="cuda")
    index = KnnIndex(X)

    def pair_extra(rec):
        nbytes = m * 2 * args.dim * 4
        rate = nbytes / rec["score_pairs"]["median_s"]
        return {"n": args.n, "dim": args.dim, "bytes_read": nbytes, "bytes_per_s": float(f"{rate:.4g}"), "share_of_hbm_peak": round(rate / HBM_PEAK, 4)}

    compare("pair_scores", {"score_pairs": lambda: index.score_pairs(u, v, metric="dot"),
                            "torch": lambda: (X[u].double() * X[v].double()).sum(1)}, pair_extra)

    pos = index.score_pairs(u, v, metric="cosine")
    neg = index.score_pairs(v, torch.roll(u, 1), metric="cosine")
    index.close()

    def torch_auc():
        s = torch.sort(neg).values
        lb, ub = torch.searchsorted(s, pos), torch.searchsorted(s, pos, right=True)
        return int(lb.sum()), int((ub - lb).sum())

    compare("auc", {"auc": lambda: linkpred.auc(pos, neg), "torch": torch_auc})
    del pos, neg, X, u, v

    indptr, indices, _ = rmat_csr(args.scale, seed=1)
    graph = node2vec.SparseOTF.from_csr(indptr, indices, None)
    graph.device = 0
    n_nodes = indptr.size - 1
    keys = (torch.from_numpy(np.repeat(np.arange(n_nodes, dtype=np.int64), np.diff(indptr.astype(np.int64)))) * n_nodes
            + torch.from_numpy(indices.astype(np.int64))).cuda()   # ascending: the CSR's order

    def torch_sampler():
        draw = int(m * 1.05) + 1024
        cu = torch.randint(0, n_nodes, (draw,), device="cuda")
        cv = torch.randint(0, n_nodes, (draw,), device="cuda")
        k = cu * n_nodes + cv
        at = torch.searchsorted(keys, k).clamp_(max=keys.numel() - 1)
        ok = (keys[at] != k) & (cu != cv)
        return cu[ok][:m], cv[ok][:m]

    graph.sample_non_edges(1, seed=1)   # (the handle: built before the clock starts)
    compare("sample_non_edges", {"sample_non_edges": lambda: graph.sample_non_edges(m, seed=7), "torch": torch_sampler},
            lambda rec: {"n_nodes": n_nodes, "nnz": int(indices.size)})


if __name__ == "__main__":
    main()
