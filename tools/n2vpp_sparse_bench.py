#!/usr/bin/env python3
"""node2vec++ on a CSR handle (SparseNode2vecPlusPlus, walk_sparse_pp_kernel) against SparseOTF node2vec+ on weighted RMAT-20
(synth.rmat_csr(20, weighted=True), the C5 graph), p = 0.5, q = 2, 10 x 80 walks.  Three forms alternate in one process,
`passes` passes each; one JSON line per pass:
  node2vec++            SparseNode2vecPlusPlus (mode 6)
  node2vec+ lanes       SparseOTF extend as shipped (weighted lane form)
  node2vec+ wave        SparseOTF extend on the wave kernel (PECANPY_AMD_NO_LANES=1: a second handle made with it set)
Declared bytes per step of node2vec++ (walk_sparse_pp.hip.h header): 24 d(cur) (key, weight, threshold, prev's filter word)
+ 44, with d(cur) the degree-weighted mean degree sum(d^2) / sum(d) (the row a step stands on); the 12 bytes per filter
survivor (index probe + prev's weight) are left out.  It reads every element of cur's row at every step.  The node2vec+ forms
stop at the sampled element with per-edge row totals: the same formula does not describe them, so their
lines carry no declared bytes.
usage: python tools/n2vpp_sparse_bench.py [scale=20] [num_walks=10] [walk_length=80] [passes=3] [forms=all | comma list of
       pp,lanes,wave]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from pecanpy_amd import synth
    from pecanpy_amd.engine import WalkEngine
    from pecanpy_amd.experimental import SparseNode2vecPlusPlus
    from pecanpy_amd.pecanpy import SparseOTF

    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 80
    passes = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    indptr, indices, data = synth.rmat_csr(scale, weighted=True)
    n = indptr.size - 1
    deg = np.diff(indptr.astype(np.int64))
    d_step = float((deg * deg).sum() / deg.sum())   # mean degree of the vertex a step stands on (degree-biased)
    g = SparseOTF.from_csr(indptr, indices, data)
    thr_plus = g.get_noise_thresholds()
    thr_pp = SparseNode2vecPlusPlus.from_csr(indptr, indices, data).get_noise_thresholds()
    eng = WalkEngine.from_csr(indptr, indices, data)          # node2vec++
    eng_lanes = WalkEngine.from_csr(indptr, indices, data)    # (a handle per form: the lane form's per-(p, q) tables depend on
    eng_lanes.set_thresholds(thr_plus)                        #  the thresholds and would be built again at every switch)
    eng.set_thresholds(thr_pp)
    os.environ["PECANPY_AMD_NO_LANES"] = "1"
    eng_wave = WalkEngine.from_csr(indptr, indices, data)
    eng_wave.set_thresholds(thr_plus)
    os.environ.pop("PECANPY_AMD_NO_LANES")
    starts = np.concatenate([np.arange(n, dtype=np.uint32)] * W)
    np.random.RandomState(0).shuffle(starts)
    d_starts = torch.from_numpy(starts.view(np.int32)).cuda()
    want = sys.argv[5].split(",") if len(sys.argv) > 5 else ["pp", "lanes", "wave"]
    forms = (("node2vec++", eng, "SparseNode2vecPlusPlus", False, {}),
             ("node2vec+ lanes", eng_lanes, "SparseOTF", True, {}),
             ("node2vec+ wave", eng_wave, "SparseOTF", True, {"PECANPY_AMD_NO_LANES": "1"}))
    forms = tuple(f for f, key in zip(forms, ("pp", "lanes", "wave")) if key in want)
    for label, e, mode, extend, env in forms:   # (first launch of each kernel and its per-(p, q) tables)
        os.environ.update(env)
        e.simulate_device(mode, 0.5, 2.0, extend, d_starts[:4096], L, seed=99)
        for k in env:
            os.environ.pop(k)
    for k in range(passes):
        for label, e, mode, extend, env in forms:
            os.environ.update(env)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e.simulate_device(mode, 0.5, 2.0, extend, d_starts, L, seed=k)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t) * 1e3
            for key in env:
                os.environ.pop(key)
            st = e.last_stats
            steps = st["total_steps"]
            declared = steps * (24 * d_step + 44) if mode == "SparseNode2vecPlusPlus" else None
            print(json.dumps({"workload": f"weighted RMAT-{scale} {label} p=0.5 q=2, {W} x {L}", "pass": k, "mean_row": round(d_step, 1),
                              "ms_per_pass": round(ms, 2), "value": round(steps / ms / 1e3, 2), "unit": "million walk-steps/s",
                              "walk_kernel_ms": round(st["walk_kernel_ms"], 2), "declared_bytes": declared,
                              "hbm_frac": round(declared / st["walk_kernel_ms"] / 1e6 / 8000, 3) if declared else None,
                              "ambiguous_steps": st["ambiguous_steps"], "lane_kernel": st.get("lane_kernel")}), flush=True)
    for e in (eng, eng_lanes, eng_wave):
        e.close()


if __name__ == "__main__":
    main()
