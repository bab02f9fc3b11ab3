#!/usr/bin/env python3
"""Writing the embedding file: a float32[262144, 128] device tensor of N(0, 0.3) values (the RMAT-18 shape of
tools/embed_bench.py), names str(i), to a file on local disk.  After one warm-up call of each route, `calls` timed calls of
  (a) the host route: t.cpu().numpy() + embed.save_word2vec_format (Python's % operator over blocks of rows);
  (b) the device route: embed.save_word2vec_format_device (csrc/emb_text.hip.h: count pass, scan, fill pass per chunk, the
      chunks copied to pinned buffers and written by the library),
alternating, in one process.  One JSON line: ms of every call and the medians, for (b) also format_ms / copy_ms / write_ms
of every call, and the kernels' declared traffic -- the matrix read by the count pass and again by the fill pass, the text
written once -- over format_ms against the 8 TB/s HBM peak.  The two files of the last round are compared byte for byte.
The wall clock of a call stops when its file is closed.
usage: python tools/emb_write_bench.py [rows=262144] [dim=128] [calls=3] [directory=<tempfile default>]"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12


def main():
    import torch

    from pecanpy_amd import embed

    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    dim = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    gen = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn((rows, dim), generator=gen, device="cuda", dtype=torch.float32) * 0.3
    names = [str(i) for i in range(rows)]
    with tempfile.TemporaryDirectory(dir=sys.argv[4] if len(sys.argv) > 4 else None) as tmp:
        path_a, path_b = os.path.join(tmp, "a.emb"), os.path.join(tmp, "b.emb")

        def route_a():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            embed.save_word2vec_format(path_a, names, t.cpu().numpy())
            return {"total_ms": (time.perf_counter() - t0) * 1e3}

        def route_b():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            embed.save_word2vec_format_device(path_b, names, t)
            return {"total_ms": (time.perf_counter() - t0) * 1e3, **embed.save_word2vec_format_device.last_stats}

        routes = (("a", route_a), ("b", route_b))
        for _, fn in routes:           # warm-up: the first launch loads the code object, the first file creates its blocks
            fn()
        res = {name: [] for name, _ in routes}
        for _ in range(calls):
            for name, fn in routes:
                res[name].append(fn())
        with open(path_a, "rb") as fa, open(path_b, "rb") as fb:
            identical = fa.read() == fb.read()
        size = os.path.getsize(path_b)
    med = {name: statistics.median(c["total_ms"] for c in res[name]) for name in res}
    fmt = statistics.median(c["format_ms"] for c in res["b"])
    declared = 2 * 4 * rows * dim + size
    print(json.dumps({
        "bench": "emb_write", "rows": rows, "dim": dim, "calls": calls, "file_bytes": size, "files_identical": identical,
        "device": torch.cuda.get_device_name(0),
        "a_host_writer_ms": [round(c["total_ms"], 2) for c in res["a"]], "a_median_ms": round(med["a"], 2),
        "b_device_writer_ms": [round(c["total_ms"], 2) for c in res["b"]], "b_median_ms": round(med["b"], 2),
        "b_format_ms": [round(c["format_ms"], 3) for c in res["b"]], "b_copy_ms": [round(c["copy_ms"], 3) for c in res["b"]],
        "b_write_ms": [round(c["write_ms"], 3) for c in res["b"]], "b_chunks": res["b"][-1]["chunks"],
        "a_over_b": round(med["a"] / med["b"], 2),
        "kernels_declared_bytes": declared, "kernels_declared_bytes_per_s": round(declared / (fmt * 1e-3)),
        "kernels_share_of_hbm_peak": round(declared / (fmt * 1e-3) / HBM_PEAK, 5),
    }))
    if not identical:
        raise SystemExit("the two routes wrote different files")


if __name__ == "__main__":
    main()
