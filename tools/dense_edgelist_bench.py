#!/usr/bin/env python3
"""Dense graph from an edge-list FILE, two routes to a ready DenseOTF walk handle on one GPU.  The file is a weighted
Erdos-Renyi graph: every unordered pair with probability `density`, once ("u<TAB>v<TAB>w", decimal ids, a random orientation,
weights with four decimals in (0, 4]), in a seeded random order.
  (a) DenseOTF().read_edg (the native host reader, to_dense(), the float64 and bool N x N host arrays) + the first handle
      creation (WalkEngine.from_dense: pw_dense_create, one host thread over N^2 doubles): what a caller had before.
  (b) DenseOTF().read_edg_device: text uploaded, tokenised, numbered and sorted on the device, the CSR keeping the float64
      weights, the dense handle built from it; no N x N host array.
One warm-up of each route, then `calls` timed runs of each, alternating in one process.  Wall clock to the ready handle, the
device route's stage times, and (on the warm-up pair) whether both handles hold the same arrays.  One JSON line.
usage: python tools/dense_edgelist_bench.py [n_nodes=8192] [calls=3] [density=0.25]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_er(path, n, density, seed=1):
    import numpy as np

    rng = np.random.default_rng(seed)
    us, vs = [], []
    for i in range(n - 1):        # row by row: no N x N random matrix on the host
        js = np.nonzero(rng.random(n - 1 - i) < density)[0] + i + 1
        us.append(np.full(js.size, i, dtype=np.int64))
        vs.append(js.astype(np.int64))
    u, v = np.concatenate(us), np.concatenate(vs)
    flip = rng.random(u.size) < 0.5
    u[flip], v[flip] = v[flip].copy(), u[flip].copy()
    order = rng.permutation(u.size)
    u, v = u[order], v[order]
    w = rng.integers(1, 40_001, u.size)       # weight = w / 10^4
    step = 1 << 20
    with open(path, "w") as f:
        for lo in range(0, u.size, step):
            f.write("".join(map("%d\t%d\t%d.%04d\n".__mod__, zip(u[lo:lo + step].tolist(), v[lo:lo + step].tolist(),
                                                                 (w[lo:lo + step] // 10_000).tolist(), (w[lo:lo + step] % 10_000).tolist()))))
    return int(u.size)


def main():
    import numpy as np

    from pecanpy_amd import pecanpy as node2vec

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    density = float(sys.argv[3]) if len(sys.argv) > 3 else 0.25
    tmp = tempfile.mkdtemp(prefix="dense_edgelist_bench_")
    path = os.path.join(tmp, "er.edg")
    try:
        t0 = time.perf_counter()
        lines = write_er(path, n, density)
        write_s = time.perf_counter() - t0

        def route_a():
            t0 = time.perf_counter()
            g = node2vec.DenseOTF()
            g.read_edg(path, True, False)
            t1 = time.perf_counter()
            g._get_engine()
            t2 = time.perf_counter()
            return g, {"read_edg_ms": (t1 - t0) * 1e3, "handle_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}

        def route_b():
            t0 = time.perf_counter()
            g = node2vec.DenseOTF()
            g.read_edg_device(path, True, False)
            total = (time.perf_counter() - t0) * 1e3
            return g, {**g.last_build_stats, "total_ms": total}

        runs = {"a": [], "b": []}
        same = None
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
            if i == 0:
                xa, xb = a._engine.dense_arrays(), b._engine.dense_arrays()
                same = bool(b.last_build_stats["reader"] == "device" and a.nodes == b.nodes and b._data is None
                            and all(xa[k] == xb[k] for k in ("unit", "dense_nonneg", "nnz", "max_degree"))
                            and all(xa[k].tobytes() == xb[k].tobytes() for k in ("indptr", "indices", "data", "adjbits", "deg")))
                del xa, xb
            for g in made.values():
                g._engine.close()
            del made, a, b, g
        tot = {k: [r["total_ms"] for r in v] for k, v in runs.items()}
        stage = {k: [r.get(k) for r in runs["b"]] for k in ("upload_ms", "scan_ms", "ids_ms", "build_ms", "csr_kernels_ms", "dense_build_ms",
                                                        "read_call_ms", "handle_ms")}
        first = runs["b"][0]
        print(json.dumps({
            "bench": "dense_edgelist", "n_nodes": n, "density": density, "write_s": write_s, "lines": lines,
            "file_bytes": os.path.getsize(path), "nnz": first.get("nnz"), "host_matrix_bytes": 9 * n * n, "reader_b": first["reader"],
            "same_handle_arrays": same, "a_total_ms": tot["a"], "b_total_ms": tot["b"], "a_total_ms_median": float(np.median(tot["a"])),
            "b_total_ms_median": float(np.median(tot["b"])), "a_read_edg_ms": [r["read_edg_ms"] for r in runs["a"]],
            "a_handle_ms": [r["handle_ms"] for r in runs["a"]], "b_stage_ms": stage,
            "speedup_to_ready_handle": float(np.median(tot["a"]) / np.median(tot["b"]))}))
    finally:
        if os.path.exists(path):
            os.unlink(path)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
