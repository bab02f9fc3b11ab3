#!/usr/bin/env python3
"""Reading the walk corpus file: the files tools/walks_text_bench.py writes (SparseOTF, p = 0.5, q = 2, 10 walks of length 80
per vertex, names str(i), seeded; Base.walks_to_file) at RMAT-16 and RMAT-18, on local disk.  Per file, in one process:
  (a) corpus.read_walks_device: one warm-up call, then `calls` timed calls -- the wall clock of the call and the library's
      stage times (upload_ms, scan_ms, tokens_ms, fill_ms), the names' download (names_ms);
  (b) embed.train_sgns_file with its defaults (dim 128, window 10, one epoch, hogwild), seeded: `calls` timed calls, the wall
      clock of the call and the trainer's share of it;
  (c) corpus.read_walks, the host definition, on the same file: ONE call (pure Python behind the split: minutes at RMAT-18),
      for the scales named in host_scales; its matrix and names are compared with (a)'s.
One JSON line with every call's ms and the medians.  Progress goes to stderr.
usage: python tools/corpus_read_bench.py [calls=3] [directory=<tempfile default>] [scales=16,18] [host_scales=16,18]"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NUM_WALKS, WALK_LENGTH = 10, 80
STAGES = ("upload_ms", "scan_ms", "tokens_ms", "fill_ms", "names_ms", "call_ms")


def note(text):
    print(text, file=sys.stderr, flush=True)


def main():
    import numpy as np
    import torch

    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.corpus import read_walks, read_walks_device
    from pecanpy_amd.embed import train_sgns_file
    from pecanpy_amd.synth import rmat_csr

    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    scales = [int(s) for s in sys.argv[3].split(",")] if len(sys.argv) > 3 else [16, 18]
    host_scales = [int(s) for s in sys.argv[4].split(",") if s] if len(sys.argv) > 4 else scales
    out = {"bench": "corpus_read", "num_walks": NUM_WALKS, "walk_length": WALK_LENGTH, "calls": calls,
           "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(dir=sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else None) as tmp:
        path = os.path.join(tmp, "walks.txt")
        for scale in scales:
            indptr, indices, data = rmat_csr(scale, seed=1)
            g = node2vec.SparseOTF.from_csr(indptr, indices, data, p=0.5, q=2, random_state=1)
            g.device = 0
            g.walks_to_file(path, NUM_WALKS, WALK_LENGTH)
            del g
            note(f"rmat{scale}: {os.path.getsize(path)} bytes written")

            read_walks_device(path)   # warm-up: the first launch loads the code object, the file is in the page cache
            reads = []
            for _ in range(calls):
                d_walks, names = read_walks_device(path)
                torch.cuda.synchronize()
                reads.append(dict(read_walks_device.last_stats))
            st = reads[-1]
            if st["reader"] != "device":
                raise SystemExit("read_walks_device did not take the device reader")
            rec = {"vertices": 1 << scale, "file_bytes": st["file_bytes"], "lines": st["lines"], "tokens": st["tokens"],
                   "names": st["names"], "width": int(d_walks.shape[1])}
            for key in STAGES:
                rec["read_" + key] = [round(c[key], 3) for c in reads]
                rec["read_" + key + "_median"] = round(statistics.median(c[key] for c in reads), 3)
            note(f"rmat{scale}: read_walks_device {rec['read_call_ms_median']} ms")

            trains = []
            for _ in range(calls):
                t0 = time.perf_counter()
                _, d_vec = train_sgns_file(path, seed=1)
                torch.cuda.synchronize()
                ts = train_sgns_file.last_stats
                trains.append({"total_ms": (time.perf_counter() - t0) * 1e3, "read_ms": ts["read"]["call_ms"],
                               "trainer_ms": ts["train"]["vocab_ms"] + ts["train"]["init_ms"] + ts["train"]["train_ms"]})
            for key in ("total_ms", "read_ms", "trainer_ms"):
                rec["train_file_" + key] = [round(c[key], 2) for c in trains]
            rec["train_file_median_ms"] = round(statistics.median(c["total_ms"] for c in trains), 2)
            note(f"rmat{scale}: train_sgns_file {rec['train_file_median_ms']} ms")

            if scale in host_scales:
                t0 = time.perf_counter()
                mat, host_names = read_walks(path)
                rec["host_read_walks_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["host_over_device"] = round(rec["host_read_walks_ms"] / rec["read_call_ms_median"], 1)
                same = host_names == names and np.array_equal(d_walks.cpu().numpy().view(np.uint32), mat)
                rec["host_equals_device"] = bool(same)
                note(f"rmat{scale}: read_walks {rec['host_read_walks_ms']} ms, equal: {same}")
                del mat, host_names
                if not same:
                    out[f"rmat{scale}"] = rec
                    print(json.dumps(out))
                    raise SystemExit("the host and the device reader disagree")
            del d_walks, d_vec, names
            out[f"rmat{scale}"] = rec
            os.remove(path)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
