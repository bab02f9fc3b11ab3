#!/usr/bin/env python3
"""The embedding stage end to end: RMAT-18 (BASELINE config C2: pecanpy_amd.synth.rmat_csr(18, seed=1)), SparseOTF p=0.5 q=2,
10 x 80 walks, dim 128, window 10, 1 epoch, seed 0.  After one warm-up call of each route, `calls` timed calls of
  (a) Base.embed_array: walks -> skip-gram in device memory, vectors to the host once;
  (b) the host-matrix route: simulate_walks_array (matrix to the host) + train_sgns (matrix up again),
alternating.  One JSON line: total and per-stage ms of every call, trained pairs/s and the declared traffic of a pair,
(negative + 1) * 2 * 4 * dim + 2 * 4 * dim bytes (every target row read and written, the context row read and written), over
the 8 TB/s HBM peak.  On a tree without embed_array only route (b) runs (that is how the figure of the item-per-wavefront
kernel in MEASUREMENTS.md was taken).  The wall clock stops after the result is on the host (both routes end in a blocking copy).
usage: python tools/embed_bench.py [scale=18] [calls=3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIM, WINDOW, NEGATIVE, EPOCHS, NUM_WALKS, WALK_LENGTH, SEED = 128, 10, 5, 1, 10, 80, 0
HBM_PEAK = 8e12


def main():
    import torch

    from pecanpy_amd import embed, pecanpy
    from pecanpy_amd.synth import rmat_csr

    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 18
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    indptr, indices, data = rmat_csr(scale, seed=1)
    g = pecanpy.SparseOTF.from_csr(indptr, indices, data, p=0.5, q=2, random_state=SEED)
    g.device = 0
    have_a = hasattr(g, "embed_array")

    def route_a():
        t = time.perf_counter()
        vec = g.embed_array(DIM, NUM_WALKS, WALK_LENGTH, WINDOW, EPOCHS)
        total = (time.perf_counter() - t) * 1e3
        st = dict(g.last_embed_stats)
        st["total_ms"] = total
        return vec, st

    def route_b():
        t0 = time.perf_counter()
        mat = g.simulate_walks_array(NUM_WALKS, WALK_LENGTH)
        t1 = time.perf_counter()
        vec = embed.train_sgns(mat, g.num_nodes, dim=DIM, window=WINDOW, epochs=EPOCHS, negative=NEGATIVE, seed=SEED, device=0)
        t2 = time.perf_counter()
        # walks_call_ms holds the device-to-host copy of the matrix, train_call_ms its upload, the vocabulary pass, the
        # training and the download of the vectors
        return vec, {"total_ms": (t2 - t0) * 1e3, "walks_call_ms": (t1 - t0) * 1e3, "walk_kernel_ms": g.last_stats["walk_kernel_ms"],
                     "train_call_ms": (t2 - t1) * 1e3, "walk_matrix_host_bytes": 2 * mat.nbytes}

    routes = ([("a", route_a)] if have_a else []) + [("b", route_b)]
    for _, fn in routes:           # warm-up: first launches load the code objects, the walk engine builds its index
        fn()
    rows = {name: [] for name, _ in routes}
    for _ in range(calls):
        for name, fn in routes:
            torch.cuda.synchronize()
            _, st = fn()
            rows[name].append({k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()})
    out = {"workload": f"RMAT-{scale} SparseOTF p=0.5 q=2, {NUM_WALKS} x {WALK_LENGTH}, SGNS dim {DIM} window {WINDOW} negative {NEGATIVE} "
                       f"epochs {EPOCHS} seed {SEED}",
           "device": torch.cuda.get_device_name(0), "calls": calls, "kernel": "walk-resident" if have_a else "item-per-wavefront"}
    pair_bytes = (NEGATIVE + 1) * 2 * 4 * DIM + 2 * 4 * DIM
    out["declared_bytes_per_pair"] = pair_bytes
    for name, _ in routes:
        tot = sorted(r["total_ms"] for r in rows[name])
        out[f"route_{name}"] = {"total_ms_median": tot[len(tot) // 2], "total_ms_min": tot[0], "total_ms_max": tot[-1], "calls": rows[name]}
    if have_a:
        best = min(rows["a"], key=lambda r: r["train_ms"])
        out["trained_pairs"] = best["trained_pairs"]
        out["pairs_per_s"] = round(best["trained_pairs"] / best["train_ms"] * 1e3)
        out["hbm_frac_declared"] = round(best["trained_pairs"] * pair_bytes / (best["train_ms"] * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
