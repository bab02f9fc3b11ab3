#!/usr/bin/env python3
"""Graph from an edge-list FILE, two routes to a ready walk handle on one GPU.  The file is synth.rmat_csr(scale, seed=1)
written as an unweighted edge list: every undirected edge once ("u<TAB>v", decimal ids), in a seeded random order, with a
random orientation.  Scale 20 when the file can be written in about a minute (estimated from the first sixteenth), else 18;
the result says which.
  (a) SparseOTF().read_edg (the native host reader, one thread) + the first handle creation (WalkEngine.from_csr: upload
      and index build): what a caller had before read_edg_device.
  (b) SparseOTF().read_edg_device: text uploaded, tokenised, numbered and built into the CSR on the device, exported, the
      handle made from the device CSR.
One warm-up of each route, then `calls` timed runs of each, alternating in one process.  Wall clock to the ready handle, the
device reader's stage times, and whether both routes gave the same names and CSR.  One JSON line.
usage: python tools/edgelist_bench.py [scale=20] [calls=3]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def edge_arrays(scale):
    import numpy as np

    from pecanpy_amd.synth import rmat_csr

    indptr, indices, _ = rmat_csr(scale, seed=1)
    n = indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    upper = rows < cols
    u, v = rows[upper], cols[upper]
    rng = np.random.default_rng(1)
    flip = rng.random(u.size) < 0.5
    u[flip], v[flip] = v[flip].copy(), u[flip].copy()
    order = rng.permutation(u.size)
    return u[order], v[order]


def write_edges(path, u, v, budget_s):
    """Writes the list; returns the seconds it took, or None when the first sixteenth says the whole would pass the budget."""
    t0 = time.perf_counter()
    step = max(1, u.size // 16)
    with open(path, "w") as f:
        for lo in range(0, u.size, step):
            f.write("".join(map("%d\t%d\n".__mod__, zip(u[lo:lo + step].tolist(), v[lo:lo + step].tolist()))))
            if lo == 0 and budget_s is not None and (time.perf_counter() - t0) * 16 > budget_s:
                return None
    return time.perf_counter() - t0


def main():
    import numpy as np

    from pecanpy_amd import pecanpy as node2vec

    asked = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    tmp = tempfile.mkdtemp(prefix="edgelist_bench_")
    path = os.path.join(tmp, "rmat.edg")
    scale, fell_back = asked, False
    try:
        u, v = edge_arrays(scale)
        write_s = write_edges(path, u, v, 60.0 if scale > 18 else None)
        if write_s is None:
            scale, fell_back = 18, True
            u, v = edge_arrays(scale)
            write_s = write_edges(path, u, v, None)
        lines = int(u.size)
        del u, v

        def route_a():
            t0 = time.perf_counter()
            g = node2vec.SparseOTF()
            g.read_edg(path, False, False)
            t1 = time.perf_counter()
            g._get_engine()
            t2 = time.perf_counter()
            return g, {"read_edg_ms": (t1 - t0) * 1e3, "handle_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}

        def route_b():
            t0 = time.perf_counter()
            g = node2vec.SparseOTF()
            g.read_edg_device(path, False, False)
            total = (time.perf_counter() - t0) * 1e3
            return g, {**g.last_build_stats, "total_ms": total}

        runs = {"a": [], "b": []}
        same = True
        for i in range(calls + 1):   # call 0: warm-up
            made = {}
            for name, route in (("a", route_a), ("b", route_b)):
                g, st = route()
                made[name] = g
                if i == 0:
                    print(json.dumps({"warmup": name, **st}), file=sys.stderr, flush=True)
                else:
                    runs[name].append(st)
                    print(json.dumps({"run": i, "route": name, "total_ms": st["total_ms"]}), file=sys.stderr, flush=True)
            a, b = made["a"], made["b"]
            same = same and b.last_build_stats["reader"] == "device" and a.nodes == b.nodes and all(
                x.dtype == y.dtype and np.array_equal(x, y) for x, y in ((a.indptr, b.indptr), (a.indices, b.indices), (a.data, b.data)))
            for g in made.values():
                g._engine.close()
            del made, a, b, g
        tot = {k: [r["total_ms"] for r in v] for k, v in runs.items()}
        stage = {k: [r[k] for r in runs["b"]] for k in ("upload_ms", "scan_ms", "ids_ms", "build_ms", "csr_kernels_ms", "export_ms", "handle_ms")}
        first = runs["b"][0]
        print(json.dumps({
            "bench": "edgelist", "scale": scale, "asked_scale": asked, "fell_back_to_18": fell_back, "write_s": write_s, "lines": lines,
            "file_bytes": os.path.getsize(path), "n_nodes": first["n_nodes"], "nnz": first["nnz"], "same_names_and_csr": bool(same),
            "a_total_ms": tot["a"], "b_total_ms": tot["b"], "a_total_ms_median": float(np.median(tot["a"])),
            "b_total_ms_median": float(np.median(tot["b"])), "a_read_edg_ms": [r["read_edg_ms"] for r in runs["a"]],
            "a_handle_ms": [r["handle_ms"] for r in runs["a"]], "b_stage_ms": stage,
            "a_lines_per_s": lines / (float(np.median([r["read_edg_ms"] for r in runs["a"]])) / 1e3),
            "speedup_to_ready_handle": float(np.median(tot["a"]) / np.median(tot["b"]))}))
    finally:
        if os.path.exists(path):
            os.unlink(path)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
