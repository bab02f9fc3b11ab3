#!/usr/bin/env python3
"""Graph from an edge list, two routes to a ready walk handle on one GPU.  The graph is synth.rmat_csr(scale, seed=1)
(scale 22: BASELINE's RMAT-22) turned into a shuffled undirected COO: one orientation per edge (chosen at random), 2 % of
the edges repeated, the whole list permuted.
  (a) WalkEngine.from_edge_index on the COO as CUDA tensors: CSR built on the device (pw_coo_to_csr_device), exported,
      handle made from the device CSR (pw_csr_create_device).  Wall clock to the ready handle + the build's device ms.
  (b) what a caller had before from_edge_index: the same COO as host arrays, symmetrised, sorted with np.lexsort, the last
      of every run of equal pairs kept, indptr by counting -- then WalkEngine.from_csr.  (A caller whose COO is on the GPU
      pays a download in front of this; it is not counted.)
One warm-up of each route, then `calls` timed runs of each, alternating.  Both CSRs are compared with the generator's.
Also: the device time of copying the sort's key array once (8 bytes per insertion, read + write), the yardstick for
build_ms (the HIP-event time of the build's kernels alone, allocations excluded).  One JSON line.
usage: python tools/edge_index_bench.py [scale=22] [calls=3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_csr(e, n):
    """Sort / symmetrise / keep-last on the host (NumPy), the route (b) preparation."""
    import numpy as np

    src = np.empty(2 * e.shape[1], dtype=np.int64)
    dst = np.empty(2 * e.shape[1], dtype=np.int64)
    src[0::2], src[1::2] = e[0], e[1]      # insertion order: forward, then reverse, edge by edge
    dst[0::2], dst[1::2] = e[1], e[0]
    order = np.lexsort((dst, src))         # stable: equal pairs stay in insertion order
    src, dst = src[order], dst[order]
    last = np.empty(src.size, dtype=bool)
    last[-1:] = True
    last[:-1] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    src, dst = src[last], dst[last]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=indptr[1:])
    return indptr.astype(np.uint32), dst.astype(np.uint32)


def main():
    import numpy as np
    import torch

    from pecanpy_amd.engine import WalkEngine
    from pecanpy_amd.synth import rmat_csr

    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    indptr, indices, _ = rmat_csr(scale, seed=1)
    n = indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    upper = rows < cols
    e = np.stack([rows[upper], cols[upper]])
    del rows, cols
    rng = np.random.default_rng(1)
    e = np.concatenate([e, e[:, rng.integers(0, e.shape[1], e.shape[1] // 50)]], axis=1)
    flip = rng.random(e.shape[1]) < 0.5
    e[:, flip] = e[::-1, flip]
    e = np.ascontiguousarray(e[:, rng.permutation(e.shape[1])])
    t = time.perf_counter()
    d_e = torch.from_numpy(e).cuda()
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t) * 1e3

    def route_a():
        t0 = time.perf_counter()
        eng = WalkEngine.from_edge_index(d_e, None, num_nodes=n, directed=False, device=0)
        total = (time.perf_counter() - t0) * 1e3
        st = dict(eng.build_stats)
        st["total_ms"] = total
        return eng, st

    def route_b():
        t0 = time.perf_counter()
        ip, ix = host_csr(e, n)
        t1 = time.perf_counter()
        eng = WalkEngine.from_csr(ip, ix, None, device=0)
        t2 = time.perf_counter()
        eng.csr = (ip, ix)
        return eng, {"host_csr_ms": (t1 - t0) * 1e3, "from_csr_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}

    runs = {"a": [], "b": []}
    ok = True
    for i in range(calls + 1):   # call 0: warm-up
        for name, route in (("a", route_a), ("b", route_b)):
            eng, st = route()
            if i == 0:
                ok = ok and np.array_equal(eng.csr[0], indptr) and np.array_equal(eng.csr[1], indices)
                st["lane_list_entries"] = eng.index_info()["lane_list_entries"]
                print(json.dumps({"warmup": name, **st}), file=sys.stderr, flush=True)
            else:
                runs[name].append(st)
                print(json.dumps({"run": i, "route": name, "total_ms": st["total_ms"]}), file=sys.stderr, flush=True)
            eng.close()
            del eng
    n_ins = runs["a"][0]["insertions"]
    keys = torch.empty(n_ins, dtype=torch.int64, device="cuda")
    out = torch.empty_like(keys)
    copy_ms = []
    for _ in range(4):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out.copy_(keys)
        ev[1].record()
        torch.cuda.synchronize()
        copy_ms.append(ev[0].elapsed_time(ev[1]))
    tot = {k: [r["total_ms"] for r in v] for k, v in runs.items()}
    build = [r["build_ms"] for r in runs["a"]]
    print(json.dumps({
        "bench": "edge_index", "scale": scale, "n_nodes": n, "coo_edges": int(e.shape[1]), "insertions": n_ins,
        "nnz": int(indices.size), "csr_matches_generator": bool(ok), "coo_upload_ms": upload_ms,
        "a_total_ms": tot["a"], "b_total_ms": tot["b"], "a_total_ms_median": float(np.median(tot["a"])),
        "b_total_ms_median": float(np.median(tot["b"])), "a_build_ms": build, "a_runs": runs["a"], "b_runs": runs["b"],
        "key_copy_ms": copy_ms[1:], "build_over_key_copy": float(np.median(build) / np.median(copy_ms[1:])),
        "sort_passes": -(-2 * max(1, int(n - 1).bit_length()) // 8)}))


if __name__ == "__main__":
    main()
