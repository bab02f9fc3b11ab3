#!/usr/bin/env python3
"""Generate tests/golden/n2vpp_sparse/n2vpp_sparse_*.npz by running the reference's node2vec++ (experimental.Node2vecPlusPlus)
itself, on dense float64 matrices whose weights are float32-exact: the reference has no sparse node2vec++, so
experimental.SparseNode2vecPlusPlus is pinned to its dense class run on A.toarray().astype(np.float64).

Same recipe, shims and file layout as make_golden_n2vpp.py (whose ``case`` writes the fixture).  The walks on CSR handles
also reuse the float32-exact fixtures of tests/golden/n2vpp/ (karate, sink, wdy, wre) as they are.

usage:  python tests/golden/make_golden_n2vpp_sparse.py        (rewrites tests/golden/n2vpp_sparse/n2vpp_sparse_*.npz)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_n2vpp as mgp  # noqa: E402  (the reference, its shims and the fixture writer)
import numpy as np  # noqa: E402


def case(name, mat, p, q, gamma, seed, num_walks, walk_length, n_prob_samples=40):
    mat = np.asarray(mat, dtype=np.float64)
    assert np.array_equal(mat.astype(np.float32).astype(np.float64), mat), "weights must be float32-exact"
    out = mgp.case(name, mat, p, q, gamma, seed, num_walks, walk_length, n_prob_samples)
    src = os.path.join(HERE, "n2vpp", name + ".npz")
    dst = os.path.join(HERE, "n2vpp_sparse", name + ".npz")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    os.replace(src, dst)
    print(f"moved to {dst}")
    return out


def main():
    # weights near 2^-60 (float32-exact) beside weights of order 1: b < 2^-54 makes 1 + (b - 1) zero -- NaN probabilities
    # for q > 1, inf / NaN for q < 1
    rng = np.random.default_rng(17)
    n = 14
    up = np.triu(rng.random((n, n)) < 0.4, 1)
    up[np.arange(n - 1), np.arange(1, n)] = True
    vals = rng.choice(np.array([2.0 ** -60, 3 * 2.0 ** -61, 0.5, 2.0, 5.0, 0.75]), size=(n, n))
    tm = np.where(up, vals, 0.0)
    tm = tm + tm.T
    for q, seed in ((2.0, 18), (0.5, 19)):
        o = case(f"n2vpp_sparse_tiny_p0.5_q{q:g}", tm, 0.5, q, 0.0, seed, 6, 20, n_prob_samples=60)
        assert np.isnan(o["prob_vals"]).any(), "the tiny-weight graph must reach NaN probabilities"

    # directed weighted graph with self loops, sinks (vertices without out-edges) and an isolated vertex
    rng = np.random.default_rng(23)
    n = 20
    m = (rng.random((n, n)) < 0.18) * rng.choice(np.array([0.25, 0.5, 1.0, 1.5, 3.0, 0.125]), size=(n, n))
    m[np.arange(0, n, 3), np.arange(0, n, 3)] = 2.0     # self loops
    m[[4, 11], :] = 0.0                                  # sinks
    m[17, :] = 0.0
    m[:, 17] = 0.0                                       # isolated vertex
    for p, q, gamma, seed in ((0.5, 2.0, 0.0, 24), (0.7, 0.4, 0.5, 25)):
        case(f"n2vpp_sparse_dirloop_g{gamma}_p{p:g}_q{q:g}", m, p, q, gamma, seed, 5, 16)


if __name__ == "__main__":
    main()
