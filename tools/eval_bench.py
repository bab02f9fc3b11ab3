#!/usr/bin/env python3
"""One read-only scoring pass beside one training epoch of the same session: RMAT-18 (BASELINE config C2:
pecanpy_amd.synth.rmat_csr(18, seed=1)), SparseOTF p=0.5 q=2, 10 x 80 walks, dim 128, window 10, negative 5, seed 0, the
trainer's default wavefront count.  One session of `rounds` + 1 epochs; after a warm-up of each (one epoch, one evaluate),
`rounds` times: SgnsSession.evaluate() on the session's own corpus, then SgnsSession.run(1), each between device synchronises on
the host clock (evaluate is one kernel and two small reductions; run(1) also reports its kernels' hipEvent time, train_ms).
evaluate_foreign_ms scores the same matrix passed as a foreign one: the pass plus the device check of its contents.
One JSON line.
usage: python tools/eval_bench.py [scale=18] [rounds=3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIM, WINDOW, NEGATIVE, NUM_WALKS, WALK_LENGTH, SEED = 128, 10, 5, 10, 80, 0


def main():
    import torch

    from pecanpy_amd import pecanpy
    from pecanpy_amd.synth import rmat_csr

    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 18
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    indptr, indices, data = rmat_csr(scale, seed=1)
    g = pecanpy.SparseOTF.from_csr(indptr, indices, data, p=0.5, q=2, random_state=SEED)
    g.device = 0

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t) * 1e3

    rows = []
    with g.embed_session(DIM, NUM_WALKS, WALK_LENGTH, WINDOW, epochs=rounds + 1) as s:   # (a plain trainer: no loss in its epochs)
        s.run(1)
        s.evaluate()
        for _ in range(rounds):
            scored, evaluate_ms = timed(s.evaluate)
            foreign, foreign_ms = timed(lambda: s.evaluate(s.d_walks.clone()))
            assert foreign == scored, (foreign, scored)
            trained, run_ms = timed(lambda: s.run(1)[0])
            rows.append({"evaluate_ms": round(evaluate_ms, 2), "evaluate_foreign_ms": round(foreign_ms, 2), "run_ms": round(run_ms, 2),
                         "train_ms": round(s.last_stats["train_ms"], 2), "evaluations": scored["evaluations"],
                         "trained_pairs": trained["trained_pairs"], "mean_loss_scored": scored["loss"] / scored["evaluations"]})
        waves = s.last_stats["wavefronts"]
    med = lambda key: sorted(r[key] for r in rows)[len(rows) // 2]   # noqa: E731
    out = {"workload": f"RMAT-{scale} SparseOTF p=0.5 q=2, {NUM_WALKS} x {WALK_LENGTH}, SGNS dim {DIM} window {WINDOW} negative {NEGATIVE} "
                       f"seed {SEED}", "device": torch.cuda.get_device_name(0), "rounds": rounds, "training_wavefronts": waves,
           "evaluate_ms_median": med("evaluate_ms"), "evaluate_foreign_ms_median": med("evaluate_foreign_ms"),
           "run_ms_median": med("run_ms"), "train_ms_median": med("train_ms"),
           "evaluate_over_epoch": round(med("evaluate_ms") / med("run_ms"), 4), "calls": rows}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
