#!/usr/bin/env python3
"""node2vec++ (Node2vecPlusPlus, walk_dense_weighted_kernel<DW_N2VPP>) against node2vec+ (DenseOTF extend) on the weighted dense
graph of tools/dense_weighted_bench.py: Erdos-Renyi N nodes, density 0.25, U(0,1] float64 weights, p=0.5 q=2.  The two modes run
alternately in one process, `passes` passes each; one JSON line per pass.  Both read the same bytes per step:
12 d(cur) + N / 8 + 8 d(prev) + 12 (node2vec+'s declared format).
usage: python tools/n2vpp_bench.py [N=20000] [num_walks=10] [walk_length=80] [passes=3]"""
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
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 80
    passes = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    dens = 0.25
    rng = np.random.default_rng(1)
    up = np.triu(rng.random((n, n), dtype=np.float32) < dens, 1)
    w = rng.random((n, n), dtype=np.float32).astype(np.float64) * 0.999 + 0.001
    data = np.where(up, w, 0.0)
    del up, w
    data = data + data.T
    eng = WalkEngine.from_dense(data)
    thr = np.zeros(n, dtype=np.float32)
    _lib.check(_lib.load().pw_noise_thresholds_dense(C.c_void_p(data.ctypes.data), n, C.c_double(0.0), C.c_void_p(thr.ctypes.data)))
    eng.set_thresholds(thr)
    dmean = float((data != 0).sum(1).mean())
    del data
    starts = np.concatenate([np.arange(n, dtype=np.uint32)] * W)
    np.random.RandomState(0).shuffle(starts)
    d_starts = torch.from_numpy(starts.view(np.int32)).cuda()
    eng.simulate_device("Node2vecPlusPlus", 0.5, 2.0, False, d_starts[:4096], L, seed=99)   # (first launch of each kernel)
    eng.simulate_device("DenseOTF", 0.5, 2.0, True, d_starts[:4096], L, seed=99)
    for k in range(passes):
        for mode, extend, label in (("DenseOTF", True, "node2vec+"), ("Node2vecPlusPlus", False, "node2vec++")):
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.simulate_device(mode, 0.5, 2.0, extend, d_starts, L, seed=k)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t) * 1e3
            st = eng.last_stats
            steps = st["total_steps"]
            declared = steps * (12 * dmean + n / 8 + 8 * dmean + 12)
            print(json.dumps({"workload": f"ER-{n} density {dens} weighted {label} p=0.5 q=2, {W} x {L}", "pass": k,
                              "ms_per_pass": round(ms, 2), "value": round(steps / ms / 1e3, 2), "unit": "million walk-steps/s",
                              "walk_kernel_ms": round(st["walk_kernel_ms"], 2), "declared_bytes": declared,
                              "hbm_frac": round(declared / st["walk_kernel_ms"] / 1e6 / 8000, 3),
                              "ambiguous_steps": st["ambiguous_steps"], "redo_walks": st["redo_walks"]}), flush=True)


if __name__ == "__main__":
    main()
