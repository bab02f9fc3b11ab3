"""Edge hold-out on the GPU: ``Base.holdout_edges`` (exact by the written definition of csrc/holdout.hip.h) beside the plain
torch statement on the same device -- mask an ``edge_index`` tensor with ``torch.rand``, then ``from_edge_index`` -- which is
neither seeded in the project's sense nor protects a vertex's last edge: for scale only.

    python tools/holdout_bench.py [--scales 18 22] [--fraction 0.5] [--repeats 3]

The two routes alternate in one process; the first round is a warm-up; every timing is wall clock around a device
synchronisation.  One JSON line per graph: median / min / max seconds of each route, and the stages of the hold-out call as
the library times them (``last_holdout_stats``, medians, ms): word expansion, flag kernels, scans with the compactions, and
the build of the train graph's walk handle with the export of its arrays.  The torch route's own stages: the mask with the
row selection, and ``from_edge_index`` (CSR build on the device, export, handle)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.synth import rmat_csr

    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[18, 22])
    ap.add_argument("--fraction", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def summary(ts):
        return {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}

    for scale in args.scales:
        indptr, indices, _ = rmat_csr(scale, seed=1)
        n_nodes = indptr.size - 1
        graph = node2vec.SparseOTF.from_csr(indptr, indices, None)
        graph.device = 0
        graph._get_engine()   # (the source handle: built before the clock starts)
        rows = torch.from_numpy(np.repeat(np.arange(n_nodes, dtype=np.int64), np.diff(indptr.astype(np.int64)))).cuda()
        cols = torch.from_numpy(indices.astype(np.int64)).cuda()
        upper = rows < cols
        edge_index = torch.stack([rows[upper], cols[upper]])   # every undirected edge once, as a user holds it
        del rows, cols, upper
        torch_stage = {"mask_s": [], "from_edge_index_s": []}

        def torch_route(record):
            dt, kept = timed(lambda: edge_index[:, torch.rand(edge_index.shape[1], device="cuda") >= args.fraction])
            dt2, g2 = timed(lambda: node2vec.SparseOTF.from_edge_index(kept, num_nodes=n_nodes))
            if record:
                torch_stage["mask_s"].append(dt)
                torch_stage["from_edge_index_s"].append(dt2)
            g2._engine.close()

        def holdout_route(record):
            train, _, _ = graph.holdout_edges(args.fraction, seed=7)
            if record:
                stages.append(dict(graph.last_holdout_stats))
            train._engine.close()

        stages, times = [], {"holdout_edges": [], "torch": []}
        for rep in range(args.repeats + 1):   # round 0 warms up
            for name, fn in (("holdout_edges", holdout_route), ("torch", torch_route)):
                dt, _ = timed(lambda: fn(rep > 0))
                if rep:
                    times[name].append(dt)
        rec = {"call": "holdout_edges", "scale": scale, "n_nodes": n_nodes, "nnz": int(indices.size), "fraction": args.fraction,
               "repeats": args.repeats, "holdout_edges": summary(times["holdout_edges"]), "torch": summary(times["torch"]),
               "held": stages[0]["held"], "units": stages[0]["units"], "protected": stages[0]["protected"],
               "holdout_stages_ms": {k: round(statistics.median(s[k] for s in stages), 3)
                                     for k in ("expand_ms", "flag_ms", "scan_compact_ms", "split_call_ms", "handle_ms")},
               "torch_stages_s": {k: round(statistics.median(v), 5) for k, v in torch_stage.items()}}
        print(json.dumps(rec), flush=True)
        graph._engine.close()
        del edge_index, graph


if __name__ == "__main__":
    main()
