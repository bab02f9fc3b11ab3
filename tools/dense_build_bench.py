#!/usr/bin/env python3
"""Building a dense weighted graph handle: the host route (pw_dense_create, one thread over N^2 doubles) against the device
route (pw_dense_create_device, csrc/dense_build.hip.h), and the node2vec+ thresholds on the host against the device.

The matrix is that of tools/dense_weighted_bench.py: Erdos-Renyi N nodes, density 0.25, hashed U(0, 1] float64 weights.
usage: python tools/dense_build_bench.py [N=20000] [repetitions=3] [density=0.25]

One process, one JSON line per repetition (no best-of):
  from_dense              WalkEngine.from_dense(data): wall clock of the call
  from_dense_tensor_numpy from_dense_tensor on the NumPy array: wall clock (upload included), build_ms
  from_dense_tensor_cuda  from_dense_tensor on a CUDA tensor: wall clock, build_ms.  Every repetition uploads the matrix into a
                          new tensor first (outside the clock), so the build does not find it in the caches it left itself;
                          torch's allocator may hand out the same block again
  d2d_copy                one torch device-to-device copy of the matrix between two events: the in-run yardstick for "one
                          stream of the matrix" (N^2 * 8 bytes read and as many written)
  thresholds_host / thresholds_device   pw_noise_thresholds_dense(data) / pw_dense_noise_thresholds(handle): wall clock
build_ms is the HIP-event time of the build's kernels alone; wall clocks end after a device synchronise."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from pecanpy_amd import _lib
    from pecanpy_amd.engine import WalkEngine

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dens = float(sys.argv[3]) if len(sys.argv) > 3 else 0.25
    lib = _lib.load()
    if lib.pw_device_count() <= 0:
        raise SystemExit("dense_build_bench needs a GPU")
    rng = np.random.default_rng(1)
    t = time.time()
    up = np.triu(rng.random((n, n), dtype=np.float32) < dens, 1)
    w = rng.random((n, n), dtype=np.float32).astype(np.float64) * 0.999 + 0.001
    data = np.where(up, w, 0.0)
    del up, w
    data = data + data.T
    nbytes = data.nbytes
    print(f"# ER-{n} weighted dense matrix in {time.time() - t:.1f}s, nnz {int((data != 0).sum())}, {nbytes / 1e9:.2f} GB", flush=True)

    def line(what, rep, **kw):
        print(json.dumps({"what": what, "n": n, "density": dens, "rep": rep, **{k: round(v, 3) if isinstance(v, float) else v for k, v in kw.items()}}),
              flush=True)

    torch.cuda.synchronize()
    WalkEngine.from_dense_tensor(torch.zeros((64, 64), dtype=torch.float64, device="cuda")).close()   # code objects, streams: warm
    ref = None
    for rep in range(reps):
        t = time.perf_counter()
        eng = WalkEngine.from_dense(data)
        line("from_dense", rep, wall_ms=(time.perf_counter() - t) * 1e3)
        if ref is None:
            ref = eng.dense_arrays()
        eng.close()
    for rep in range(reps):
        t = time.perf_counter()
        eng = WalkEngine.from_dense_tensor(data, device=0)
        torch.cuda.synchronize()
        line("from_dense_tensor_numpy", rep, wall_ms=(time.perf_counter() - t) * 1e3, build_ms=eng.build_stats["build_ms"],
             upload_ms=eng.build_stats["upload_ms"])
        eng.close()
    same = None
    for rep in range(reps):
        d = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng = WalkEngine.from_dense_tensor(d)
        torch.cuda.synchronize()
        line("from_dense_tensor_cuda", rep, wall_ms=(time.perf_counter() - t) * 1e3, build_ms=eng.build_stats["build_ms"],
             matrix_gb_per_build_s=nbytes / eng.build_stats["build_ms"] / 1e6)
        if same is None and ref is not None:
            got = eng.dense_arrays()
            same = all(got[k].tobytes() == ref[k].tobytes() for k in ("indptr", "indices", "data", "adjbits", "deg"))
            print(f"# device-built handle equals the host-built one: {same}", flush=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dst = torch.empty_like(d)
        torch.cuda.synchronize()
        e0.record()
        dst.copy_(d)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        line("d2d_copy", rep, copy_ms=ms, gb_per_s_read_plus_write=2 * nbytes / ms / 1e6)
        del dst, d
        thr = np.zeros(n, dtype=np.float32)
        t = time.perf_counter()
        _lib.check(lib.pw_noise_thresholds_dense(C.c_void_p(data.ctypes.data), n, C.c_double(0.5), C.c_void_p(thr.ctypes.data)))
        line("thresholds_host", rep, wall_ms=(time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        got = eng.compute_thresholds(0.5)
        line("thresholds_device", rep, wall_ms=(time.perf_counter() - t) * 1e3,
             equal=bool(np.array_equal(got.view(np.uint32)[~np.isnan(thr)], thr.view(np.uint32)[~np.isnan(thr)])))
        eng.close()
    if same is False:
        raise SystemExit("the device-built handle differs from the host-built one")


if __name__ == "__main__":
    main()
