#!/usr/bin/env python3
"""Writing the walk corpus file: SparseOTF, p = 0.5, q = 2, 10 walks of length 80 per vertex, names str(i), seeded, to a file
on local disk.  After one warm-up call of each route, `calls` timed calls, alternating, in one process, of
  (a) RMAT-16 only: the ID-list route of PECANPY_AMD_DUMP_WALKS=1 -- simulate_walks (List[List[str]]) + cli._dump_walks;
      pure Python behind the walk matrix (at RMAT-18 it would make 2 * 10^8 Python strings);
  (b) RMAT-16 and RMAT-18: Base.walks_to_file -- the walk matrix stays in device memory, csrc/walk_text.hip.h makes the text
      (count pass, scan, fill pass per chunk), the chunks are copied to pinned buffers and written by the library.
One JSON line: ms of every call and the medians, for (b) also walk_ms / write_call_ms and the writer's format_ms / copy_ms /
write_ms of every call, and the kernels' declared traffic -- the matrix read by the count pass and again by the fill pass, the
name bytes gathered, the text written once -- over format_ms against the 8 TB/s HBM peak.  The two RMAT-16 files of the last
round are compared byte for byte.  The wall clock of a call stops when its file is closed.
usage: python tools/walks_text_bench.py [calls=3] [directory=<tempfile default>] [scales=16,18]"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12
NUM_WALKS, WALK_LENGTH = 10, 80


def main():
    import torch

    from pecanpy_amd import cli
    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.synth import rmat_csr

    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    scales = [int(s) for s in sys.argv[3].split(",")] if len(sys.argv) > 3 else [16, 18]
    out = {"bench": "walks_text", "mode": "SparseOTF", "p": 0.5, "q": 2, "num_walks": NUM_WALKS, "walk_length": WALK_LENGTH,
           "calls": calls, "device": torch.cuda.get_device_name(0)}
    identical = None
    with tempfile.TemporaryDirectory(dir=sys.argv[2] if len(sys.argv) > 2 else None) as tmp:
        path_a, path_b = os.path.join(tmp, "a.txt"), os.path.join(tmp, "b.txt")
        for scale in scales:
            indptr, indices, data = rmat_csr(scale, seed=1)

            def graph():
                g = node2vec.SparseOTF.from_csr(indptr, indices, data, p=0.5, q=2, random_state=1)
                g.device = 0           # one device: a call of this size would otherwise spread over every visible GPU
                return g

            g_a, g_b = graph(), graph()

            def route_a():
                t0 = time.perf_counter()
                cli._dump_walks(path_a, g_a.simulate_walks(NUM_WALKS, WALK_LENGTH))
                return {"total_ms": (time.perf_counter() - t0) * 1e3}

            def route_b():
                t0 = time.perf_counter()
                g_b.walks_to_file(path_b, NUM_WALKS, WALK_LENGTH)
                return {"total_ms": (time.perf_counter() - t0) * 1e3, **g_b.last_corpus_stats}

            routes = (("a", route_a), ("b", route_b)) if scale == scales[0] else (("b", route_b),)
            for _, fn in routes:       # warm-up: the graph goes up, the first launch loads the code object, the file gets its blocks
                fn()
            res = {name: [] for name, _ in routes}
            for _ in range(calls):
                for name, fn in routes:
                    res[name].append(fn())
            if "a" in res:
                with open(path_a, "rb") as fa, open(path_b, "rb") as fb:
                    identical = fa.read() == fb.read()
            b = res["b"]
            if b[-1]["walk_matrix_host_bytes"] != 0:
                raise SystemExit("walks_to_file did not take the device route")
            size, tokens, rows = b[-1]["bytes"], b[-1]["tokens"], b[-1]["rows"]
            fmt = statistics.median(c["format_ms"] for c in b)
            declared = 2 * 4 * rows * (WALK_LENGTH + 2) + (size - tokens) + size
            rec = {"vertices": 1 << scale, "rows": rows, "tokens": tokens, "file_bytes": size, "chunks": b[-1]["chunks"],
                   "b_walks_to_file_ms": [round(c["total_ms"], 2) for c in b],
                   "b_median_ms": round(statistics.median(c["total_ms"] for c in b), 2)}
            for key in ("walk_ms", "write_call_ms", "format_ms", "copy_ms", "write_ms"):
                rec["b_" + key] = [round(c[key], 3) for c in b]
            rec.update({"kernels_declared_bytes": declared, "kernels_declared_bytes_per_s": round(declared / (fmt * 1e-3)),
                        "kernels_share_of_hbm_peak": round(declared / (fmt * 1e-3) / HBM_PEAK, 5)})
            if "a" in res:
                med_a = statistics.median(c["total_ms"] for c in res["a"])
                rec.update({"a_id_lists_ms": [round(c["total_ms"], 2) for c in res["a"]], "a_median_ms": round(med_a, 2),
                            "a_over_b": round(med_a / rec["b_median_ms"], 2)})
            out[f"rmat{scale}"] = rec
            os.remove(path_b)
    out["files_identical"] = identical
    print(json.dumps(out))
    if identical is False:
        raise SystemExit("the two routes wrote different files")


if __name__ == "__main__":
    main()
