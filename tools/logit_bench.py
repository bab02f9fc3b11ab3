"""Exact logistic regression on the GPU (``pecanpy_amd.classify``) beside the plain torch statement in float64 on the same
device -- not reproducible bit for bit, for scale only.

    python tools/logit_bench.py [--n 262144] [--dim 128] [--pairs 10000000] [--op hadamard] [--repeats 30] [--fit_repeats 5] [--out profiles/logit_bench.jsonl]

  evaluation   one ``logit_eval`` (loss and gradient: the forward, gradient and reduce kernels) -- wall clock around a device
               synchronisation and ``kernel_ms`` between two events -- / gather, operator, ``@ w``, ``torch.sigmoid``, ``F.T @ r``
  fit          a whole ``classify.fit`` on labels planted from a linear rule of the features, with its ``n_iter`` / ``n_eval``,
               repeated ``--fit_repeats`` times after a warm-up
The two routes of the evaluation alternate in one process; the first round is a warm-up; the median, minimum and maximum of the
repeats are reported.  Declared bytes of one evaluation: ``2 * (2 m dim 4)``, the two rows of every sample in each of the two
kernels, over the median ``kernel_ms`` and as a share of the HBM peak (8.0 TB/s): DECLARED bytes, not measured
HBM traffic -- a matrix that fits the 256 MB Infinity Cache is served from there.  One JSON line per call, appended to ``--out``."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def main():
    import torch

    from pecanpy_amd import classify
    from pecanpy_amd.embed import KnnIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--op", default="hadamard", choices=classify.OPERATORS)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--fit_repeats", type=int, default=5)
    ap.add_argument("--fit_iter", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, dim = args.pairs, args.dim

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def summary(ts):
        return {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}

    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((args.n, dim), generator=gen, device="cuda", dtype=torch.float32)
    u = torch.randint(0, args.n, (m,), generator=gen, device="cuda")
    v = torch.randint(0, args.n, (m,), generator=gen, device="cuda")
    w_true = torch.randn(dim, generator=gen, device="cuda", dtype=torch.float64)

    def features(lo, hi):
        a, b = X[u[lo:hi]].double(), X[v[lo:hi]].double()
        return {"row": a, "average": (a + b) * 0.5, "hadamard": a * b, "l1": (a - b).abs(), "l2": (a - b) ** 2}[args.op]

    step = 1 << 20   # (the float64 feature matrix of all pairs at once would not be the statement anyone writes: 10 GB)
    y = torch.cat([((features(i, i + step) @ w_true + 0.5 * torch.randn(min(step, m - i), generator=gen, device="cuda", dtype=torch.float64)) > 0)
                   for i in range(0, m, step)]).to(torch.uint8)
    theta = np.random.default_rng(2).standard_normal(dim + 1) * 0.05
    w, bias = torch.from_numpy(theta[:dim]).cuda(), float(theta[dim])
    sign = 2.0 * y.double() - 1.0
    l2 = 1e-3

    def torch_eval():
        grad, loss = torch.zeros(dim, dtype=torch.float64, device="cuda"), 0.0
        for i in range(0, m, step):
            F = features(i, i + step)
            s = sign[i:i + step]
            z = F @ w + bias
            r = -s * torch.sigmoid(-s * z)
            grad += F.T @ r
            loss = loss + torch.nn.functional.softplus(-s * z).sum()
        return float(loss) / m + 0.5 * l2 * float(w @ w), grad / m + l2 * w

    index = KnnIndex(X)
    problem = classify._DeviceProblem(index, u, v, y, args.op)
    times = {"logit_eval": [], "torch": []}
    kernel_ms = []
    for rep in range(args.repeats + 1):   # round 0 warms up
        for name, fn in (("logit_eval", lambda: problem.evaluate(theta, l2)), ("torch", torch_eval)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t)
                if name == "logit_eval":
                    kernel_ms.append(problem.last_kernel_ms)
            if name == "logit_eval":
                ours = out
            else:
                theirs = out
    nbytes = 2 * (2 * m * dim * 4)
    k_med = statistics.median(kernel_ms) * 1e-3
    emit({"call": "evaluation", "op": args.op, "n": args.n, "dim": dim, "pairs": m, "repeats": args.repeats, "logit_eval": summary(times["logit_eval"]),
          "kernel_ms": {"median": round(statistics.median(kernel_ms), 4), "min": round(min(kernel_ms), 4), "max": round(max(kernel_ms), 4)},
          "torch": summary(times["torch"]), "declared_bytes": nbytes, "bytes_per_s": float(f"{nbytes / k_med:.4g}"),
          "share_of_hbm_peak": round(nbytes / k_med / HBM_PEAK, 4), "loss": ours[0], "torch_loss": theirs[0],
          "grad_max_abs_diff_from_torch": float(np.abs(ours[1][:dim] - theirs[1].cpu().numpy()).max())})

    fit_times = []
    for rep in range(args.fit_repeats + 1):   # round 0 warms up; every fit is the same computation, bit for bit
        torch.cuda.synchronize()
        t = time.perf_counter()
        model = classify.fit(index, u, v, y, args.op, l2=l2, max_iter=args.fit_iter)
        torch.cuda.synchronize()
        if rep:
            fit_times.append(time.perf_counter() - t)
    emit({"call": "fit", "op": args.op, "n": args.n, "dim": dim, "pairs": m, "max_iter": args.fit_iter, "repeats": args.fit_repeats,
          "wall": summary(fit_times), "n_iter": model.n_iter, "n_eval": model.n_eval, "converged": model.converged, "loss": model.loss,
          "s_per_eval": round(statistics.median(fit_times) / model.n_eval, 5)})
    index.close()


if __name__ == "__main__":
    main()
