"""Neighbourhood link-prediction baselines on the GPU: ``Base.neighbour_scores`` (exact by the written definition of
csrc/nbr_scores.hip.h) beside the torch statement of the same quantity that a user would otherwise write on the same device.

    python tools/nbr_bench.py [--scale 18] [--pairs 10000000] [--repeats 3] [--out profiles/nbr_bench.jsonl] [--limit 600]

Workload: RMAT-``scale`` from ``synth``, half of its edges held out (``holdout_edges``), the scores taken on the TRAIN graph for
``pairs`` pairs: one half held-out edges (the list repeated until it is long enough: the graph has fewer edges than that), one
half non-edges of the original (``sample_non_edges``), shuffled together.  Two steps, each a child process of its own under its
own time limit; the first failure ends the run:

  kinds   each of the five kinds, the library call and the torch statement alternating; round 0 warms up; median / min / max of
          the wall clock around a device synchronisation, and for the library the device time of the score kernel alone (events).
  sweep   ``short_max`` -- the cut between the kernel's lane form and its wavefront form -- over 0, 8, 16, 32, 64, 128, 256 and
          all-lane for common neighbours and Adamic-Adar: the kernel's event time.  The header's NBR_SHORT_MAX is the best.

The TORCH STATEMENT is a yardstick, not the code under test: the shorter row of every pair is expanded with
``repeat_interleave``, the keys ``row * N + z`` are looked up by ``torch.searchsorted`` in the sorted edge keys, ``scatter_add``
into the pair gives the count or, in float64, the weighted sum (a million pairs at a time: the expansion is bounded).  Its sum
order is its own -- ``scatter_add`` adds in whatever order the device likes -- so its weighted values are compared with the
library's within a tolerance, here and nowhere else; the integer kinds are compared exactly.  One JSON line per record."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KINDS = ("common_neighbours", "jaccard", "adamic_adar", "resource_allocation", "preferential_attachment")
SWEEP = (0, 8, 16, 32, 64, 128, 256, 0xFFFFFFFF)
CHUNK = 1 << 20


def workload(args):
    """``(train graph, u, v)``: the pairs as int64 tensors on the device, positives and negatives shuffled together."""
    import torch

    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.synth import rmat_csr

    indptr, indices, _ = rmat_csr(args.scale, seed=1)
    g = node2vec.SparseOTF.from_csr(indptr, indices, None)
    g.device = 0
    train, (eu, ev, _), _ = g.holdout_edges(0.5, seed=1)
    half = args.pairs // 2
    reps = -(-half // int(eu.numel()))
    pu, pv = eu.repeat(reps)[:half], ev.repeat(reps)[:half]
    nu, nv, _ = g.sample_non_edges(args.pairs - half, seed=1)
    perm = torch.randperm(args.pairs, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    u, v = torch.cat([pu, nu])[perm].contiguous(), torch.cat([pv, nv])[perm].contiguous()
    info = {"scale": args.scale, "n_nodes": int(indptr.size - 1), "train_nnz": int(train.indices.size), "held_out": int(eu.numel()), "pairs": args.pairs}
    return train, u, v, info


class TorchStatement:
    """The yardstick: the scores of the train CSR by torch calls on the device."""

    def __init__(self, train):
        import torch

        self.torch = torch
        self.n = int(train.indptr.size - 1)
        self.indptr = torch.from_numpy(train.indptr.astype(np.int64)).cuda()
        self.indices = torch.from_numpy(train.indices.astype(np.int64)).cuda()
        rows = torch.repeat_interleave(torch.arange(self.n, device="cuda"), self.indptr[1:] - self.indptr[:-1])
        self.keys = rows * self.n + self.indices   # ascending: the CSR's order
        loops = torch.zeros(self.n, dtype=torch.int64, device="cuda")
        loops[rows[rows == self.indices]] = 1
        self.deg = self.indptr[1:] - self.indptr[:-1] - loops

    def common(self, u, v, table=None):
        torch = self.torch
        out = torch.zeros(u.numel(), dtype=torch.float64 if table is not None else torch.int64, device="cuda")
        for c0 in range(0, u.numel(), CHUNK):
            cu, cv = u[c0:c0 + CHUNK], v[c0:c0 + CHUNK]
            len_u, len_v = self.indptr[cu + 1] - self.indptr[cu], self.indptr[cv + 1] - self.indptr[cv]
            swap = len_v < len_u
            a, b = torch.where(swap, cv, cu), torch.where(swap, cu, cv)   # a: the shorter row, expanded; b: searched
            len_a = torch.minimum(len_u, len_v)
            pair = torch.repeat_interleave(torch.arange(cu.numel(), device="cuda"), len_a)
            first = torch.cumsum(len_a, 0) - len_a
            z = self.indices[self.indptr[a][pair] + torch.arange(pair.numel(), device="cuda") - first[pair]]
            key = b[pair] * self.n + z
            at = torch.searchsorted(self.keys, key).clamp_(max=self.keys.numel() - 1)
            hit = (self.keys[at] == key) & (z != cu[pair]) & (z != cv[pair])
            if table is None:
                out[c0:c0 + CHUNK].scatter_add_(0, pair, hit.to(torch.int64))
            else:
                out[c0:c0 + CHUNK].scatter_add_(0, pair, torch.where(hit, table[z], torch.zeros((), dtype=torch.float64, device="cuda")))
        return out

    def score(self, u, v, kind):
        torch = self.torch
        if kind == "preferential_attachment":
            return (self.deg[u] * self.deg[v]).to(torch.float64)
        if kind == "common_neighbours":
            return self.common(u, v).to(torch.float64)
        if kind == "jaccard":
            cn = self.common(u, v)
            den = self.deg[u] + self.deg[v] - cn
            return torch.where(den == 0, torch.zeros((), dtype=torch.float64, device="cuda"), cn.to(torch.float64) / den.clamp(min=1).to(torch.float64))
        d = self.deg.to(torch.float64)
        f = 1.0 / torch.log(d) if kind == "adamic_adar" else 1.0 / d   # (the device's log: a yardstick's table)
        return self.common(u, v, torch.where(self.deg >= 2, f, torch.zeros((), dtype=torch.float64, device="cuda")))


def library_call(train, u, v, kind, short_max=-1):
    """``(score, kernel ms)`` through pw_nbr_scores_device_cut: the call of ``linkpred.neighbour_scores`` with the cut forced."""
    import torch

    from pecanpy_amd import _lib, linkpred

    eng = train._get_engine()
    table = linkpred.degree_table(train, kind) if kind in ("adamic_adar", "resource_allocation") else None
    d_u, d_v = u.to(torch.int32), v.to(torch.int32)
    score = torch.empty(u.numel(), dtype=torch.float64, device=u.device)
    ms = C.c_float(0.0)
    torch.cuda.synchronize()
    _lib.check(_lib.load().pw_nbr_scores_device_cut(eng._h, C.c_void_p(d_u.data_ptr()), C.c_void_p(d_v.data_ptr()), u.numel(),
                                                    _lib.NBR_KINDS["weighted" if table is not None else kind],
                                                    C.c_void_p(table.data_ptr()) if table is not None else None, C.c_void_p(score.data_ptr()),
                                                    short_max, C.byref(ms)))
    return score, float(ms.value)


def _stats(ts, digits=5):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def step_kinds(args, emit):
    import torch

    train, u, v, info = workload(args)
    yard = TorchStatement(train)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    for kind in KINDS:
        wall = {"neighbour_scores": [], "torch": []}
        kernel_ms, got, want = [], None, None
        for rep in range(args.repeats + 1):   # round 0 warms up
            dt, got = timed(lambda: train.neighbour_scores(u, v, kind))
            dt_t, want = timed(lambda: yard.score(u, v, kind))
            ms = library_call(train, u, v, kind)[1]
            if rep:
                wall["neighbour_scores"].append(dt)
                wall["torch"].append(dt_t)
                kernel_ms.append(ms)
        if kind in ("common_neighbours", "preferential_attachment"):
            agree = {"equal": bool(torch.equal(got, want))}
        else:   # the yardstick's own sum order (and its own log): a tolerance, in the bench only
            agree = {"max_rel_diff": float(((got - want).abs() / want.abs().clamp(min=1e-300)).max())}
        emit({"step": "kinds", "kind": kind, **info, "repeats": args.repeats, "neighbour_scores_s": _stats(wall["neighbour_scores"]),
              "torch_s": _stats(wall["torch"]), "score_kernel_ms": _stats(kernel_ms, 3),
              "torch_over_library": round(statistics.median(wall["torch"]) / statistics.median(wall["neighbour_scores"]), 2), **agree})


def step_sweep(args, emit):
    import torch

    train, u, v, info = workload(args)
    for kind in ("common_neighbours", "adamic_adar"):
        base = None
        for rep_cut in SWEEP:
            times = []
            for rep in range(args.repeats + 1):   # round 0 warms up
                score, ms = library_call(train, u, v, kind, short_max=rep_cut)
                if rep:
                    times.append(ms)
            base = score if base is None else base
            emit({"step": "sweep", "kind": kind, **info, "short_max": "all-lane" if rep_cut == 0xFFFFFFFF else rep_cut, "repeats": args.repeats,
                  "score_kernel_ms": _stats(times, 3), "same_bits_as_cut_0": bool(torch.equal(score.view(torch.int64), base.view(torch.int64)))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nbr_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=600, help="seconds a step may take")
    ap.add_argument("--step", choices=("kinds", "sweep"), default=None, help="run this step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.step:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")

        {"kinds": step_kinds, "sweep": step_sweep}[args.step](args, emit)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w", encoding="utf-8").close()
    for step in ("kinds", "sweep"):   # each step a fresh process under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--scale", str(args.scale), "--pairs", str(args.pairs), "--repeats",
               str(args.repeats), "--out", args.out]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"step {step} passed its limit of {args.limit} s: stopping", flush=True)
            return 124
        if rc != 0:
            print(f"step {step} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
