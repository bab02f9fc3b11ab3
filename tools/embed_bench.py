#!/usr/bin/env python3
"""The embedding stage end to end: RMAT-18 (BASELINE config C2: pecanpy_amd.synth.rmat_csr(18, seed=1)), SparseOTF p=0.5 q=2,
10 x 80 walks, dim 128, window 10, 1 epoch, seed 0.  After one warm-up call of each route, `calls` timed calls of
  (a) Base.embed_array: walks -> skip-gram in device memory, vectors to the host once;
  (b) the host-matrix route: simulate_walks_array (matrix to the host) + train_sgns (matrix up again),
alternating.  One JSON line: total and per-stage ms of every call, trained pairs/s and the declared traffic of a pair,
(negative + 1) * 2 * 4 * dim + 2 * 4 * dim bytes (every target row read and written, the context row read and written), over
the 8 TB/s HBM peak.  On a tree without embed_array only route (b) runs (that is how the figure of the item-per-wavefront
kernel in MEASUREMENTS.md was taken).  The wall clock stops after the result is on the host (both routes end in a blocking copy).
usage: python tools/embed_bench.py [scale=18] [calls=3]

--freeze-fraction F [F ...]: instead of the two routes, one skip-gram session per F on the same walks (Base.embed_session, racing
trainer): after the session is created a seeded random fraction F of the rows is frozen in BOTH matrices (SgnsSession.freeze), then
the schedule runs; `train_ms` (the training kernels, hipEvent) of `calls` sessions per F after one warm-up session, the values of F
taken in turn.  F = 0 freezes nothing and runs the kernel without locks.
--extend-fraction P: the use case -- a seeded random fraction P of the vertices is "new", the others keep the vectors of a full
embed_array; Base.extend_embedding(starts="new") end to end (walks from the new vertices, session, placement, training, vectors to
the host) beside a full embed_array, `calls` of each, alternating."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIM, WINDOW, NEGATIVE, EPOCHS, NUM_WALKS, WALK_LENGTH, SEED = 128, 10, 5, 1, 10, 80, 0
HBM_PEAK = 8e12


def _flag(argv, name):
    """The values after `name` up to the next flag (removed from argv), or None."""
    if name not in argv:
        return None
    i = argv.index(name)
    j = i + 1
    while j < len(argv) and not argv[j].startswith("--"):
        j += 1
    values = [float(x) for x in argv[i + 1:j]]
    del argv[i:j]
    return values


def freeze_table(g, fractions, calls, torch):
    import numpy as np

    def one(frac):
        with g.embed_session(DIM, NUM_WALKS, WALK_LENGTH, WINDOW, EPOCHS) as s:
            if frac > 0:
                rows = np.random.default_rng(SEED).permutation(g.num_nodes)[:int(round(frac * g.num_nodes))]
                s.freeze(torch.from_numpy(rows))
            s.run(EPOCHS)
            n0, n1, locked = s._lock_info()
            return {"train_ms": round(s.last_stats["train_ms"], 2), "frozen_rows": [n0, n1], "lock_instances": bool(locked),
                    "trained_pairs": s.last_stats["trained_pairs"]}

    one(fractions[0])
    rows = {f: [] for f in fractions}
    for _ in range(calls):
        for f in fractions:
            torch.cuda.synchronize()
            rows[f].append(one(f))
    return {str(f): {"train_ms": [r["train_ms"] for r in rows[f]], "frozen_rows": rows[f][0]["frozen_rows"],
                     "lock_instances": rows[f][0]["lock_instances"], "trained_pairs": rows[f][0]["trained_pairs"]} for f in fractions}


def extend_table(g, frac, calls, torch):
    import numpy as np

    full = g.embed_array(DIM, NUM_WALKS, WALK_LENGTH, WINDOW, EPOCHS)          # (warm-up, and the old vectors)
    new = np.zeros(g.num_nodes, dtype=bool)
    new[np.random.default_rng(SEED).permutation(g.num_nodes)[:max(1, int(round(frac * g.num_nodes)))]] = True
    known_ids = [g.nodes[i] for i in np.flatnonzero(~new).tolist()]
    known_vec = np.ascontiguousarray(full[~new])
    kw = dict(num_walks=NUM_WALKS, walk_length=WALK_LENGTH, window_size=WINDOW, epochs=EPOCHS)
    got = g.extend_embedding(known_ids, known_vec, **kw)                        # (warm-up)
    assert np.array_equal(got[~new].view(np.int32), known_vec.view(np.int32))
    out = {"new_vertices": int(new.sum()), "extend_total_ms": [], "embed_array_total_ms": []}
    for _ in range(calls):
        for key, fn in (("extend_total_ms", lambda: g.extend_embedding(known_ids, known_vec, **kw)),
                        ("embed_array_total_ms", lambda: g.embed_array(DIM, NUM_WALKS, WALK_LENGTH, WINDOW, EPOCHS))):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            out[key].append(round((time.perf_counter() - t) * 1e3, 2))
    return out


def main():
    import torch

    from pecanpy_amd import embed, pecanpy
    from pecanpy_amd.synth import rmat_csr

    argv = sys.argv[1:]
    fractions, extend = _flag(argv, "--freeze-fraction"), _flag(argv, "--extend-fraction")
    scale = int(argv[0]) if len(argv) > 0 else 18
    calls = int(argv[1]) if len(argv) > 1 else 3
    indptr, indices, data = rmat_csr(scale, seed=1)
    g = pecanpy.SparseOTF.from_csr(indptr, indices, data, p=0.5, q=2, random_state=SEED)
    g.device = 0
    have_a = hasattr(g, "embed_array")
    if fractions or extend:
        out = {"workload": f"RMAT-{scale} SparseOTF p=0.5 q=2, {NUM_WALKS} x {WALK_LENGTH}, SGNS dim {DIM} window {WINDOW} negative {NEGATIVE} "
                           f"epochs {EPOCHS} seed {SEED}", "device": torch.cuda.get_device_name(0), "calls": calls}
        if fractions:
            out["freeze_fraction"] = freeze_table(g, fractions, calls, torch)
        if extend:
            out["extend"] = extend_table(g, extend[0], calls, torch)
        print(json.dumps(out), flush=True)
        return

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
