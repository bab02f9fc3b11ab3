#!/usr/bin/env python3
"""Generate tests/golden/n2vpp/n2vpp_*.npz by running the reference's node2vec++ (experimental.Node2vecPlusPlus) itself.

Same recipe and shims as make_golden.py (whose module it imports: stub packages for numba & co., ``SeqArray`` rows whose
``.sum()`` is Numba's sequential loop).  Every fixture holds the dense matrix, the parameters, the shuffled starts, the walk
matrix, the float32 noise thresholds and float64 probability vectors of sampled (cur, prev) pairs (prev = -1: a first step).

usage:  python tests/golden/make_golden_n2vpp.py        (rewrites tests/golden/n2vpp/n2vpp_*.npz; a directory of their own,
        because the suites of the other modes read every tests/golden/*.npz)
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the stubs and the reference on sys.path)
import numpy as np  # noqa: E402
from pecanpy.experimental import Node2vecPlusPlus  # noqa: E402  (the reference)


def case(name, mat, p, q, gamma, seed, num_walks, walk_length, n_prob_samples=40):
    mat = np.asarray(mat, dtype=np.float64)
    g = Node2vecPlusPlus.from_mat(mat, [str(i) for i in range(mat.shape[0])], p=p, q=q, gamma=gamma, random_state=seed)
    mg._shim(g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (empty rows: NaN thresholds; tiny weights: NaN probabilities)
        starts, walks = mg.ref_walk_matrix(g, num_walks, walk_length)
        thr = g.get_noise_thresholds()
        rng = np.random.default_rng(321)
        pairs = []
        for row in walks[rng.permutation(walks.shape[0])]:
            ln = int(row[-1])
            if ln >= 3:
                j = int(rng.integers(2, ln))
                pairs.append((int(row[j - 1]), int(row[j - 2])))
            elif ln == 2:
                pairs.append((int(row[0]), -1))
            if len(pairs) >= n_prob_samples:
                break
        pairs += [(int(walks[i, 0]), -1) for i in range(3) if walks[i, -1] >= 2]
        pc, pp, pv, po = [], [], [], [0]
        for cur, prev in pairs:
            pr = g.get_normalized_probs(g.data, g.nonzero, g.p, g.q, cur, None if prev < 0 else prev, thr)
            pc.append(cur)
            pp.append(prev)
            pv.append(np.asarray(pr, dtype=np.float64))
            po.append(po[-1] + pr.size)
    out = dict(data=mat, p=float(p), q=float(q), gamma=float(gamma), seed=int(seed), num_walks=int(num_walks),
               walk_length=int(walk_length), starts=starts, walks=walks, thr=thr,
               prob_cur=np.array(pc, np.int64), prob_prev=np.array(pp, np.int64), prob_vals=np.concatenate(pv),
               prob_off=np.array(po, np.int64))
    path = os.path.join(HERE, "n2vpp", name + ".npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"wrote {path}")
    return out


def dense_of(fixture):
    z = np.load(os.path.join(HERE, fixture + ".npz"))
    return mg.dense_from_csr(z["indptr"], z["indices"], z["data"].astype(np.float64))


def main():
    # karate club, unit weights: node2vec's walks while every threshold is finite; q = 1: scale 0
    k = np.load(os.path.join(HERE, "karate_csr.npz"))
    km = mg.dense_from_csr(k["indptr"], k["indices"], k["data"].astype(np.float64))
    case("n2vpp_karate_p0.5_q2", km, 0.5, 2.0, 0.0, 0, 10, 40)
    case("n2vpp_karate_p1_q0.5", km, 1.0, 0.5, 0.0, 1, 10, 40)
    case("n2vpp_karate_p0.3_q1", km, 0.3, 1.0, 0.0, 2, 10, 40)

    # the 48-vertex weighted graphs of make_golden.py (real and dyadic weights), gamma 0 and 0.5
    for tag in ("wre", "wdy"):
        wm = dense_of(f"{tag}_DenseOTF_n2v_g0.0_p0.5_q2")
        for gamma in (0.0, 0.5):
            case(f"n2vpp_{tag}_g{gamma}_p0.7_q0.4", wm, 0.7, 0.4, gamma, 13, 4, 30)

    # directed unit graph with a sink and an isolated vertex: NaN thresholds, dead ends
    sm = dense_of("sink_DenseOTF_p0.5_q2")
    case("n2vpp_sink_p0.5_q2", sm, 0.5, 2.0, 0.0, 5, 6, 12)
    case("n2vpp_sink_p0.7_q0.4", sm, 0.7, 0.4, 0.0, 6, 6, 12)

    # weights of about 1e-20 beside weights of order 1: b < 2^-54 makes 1 + (b - 1) zero -- NaN probabilities for q > 1,
    # inf / NaN for q < 1
    rng = np.random.default_rng(7)
    n = 12
    up = np.triu(rng.random((n, n)) < 0.45, 1)
    up[np.arange(n - 1), np.arange(1, n)] = True
    vals = rng.choice(np.array([1e-20, 3e-20, 0.5, 2.0, 5.0]), size=(n, n))
    tm = np.where(up, vals, 0.0)
    tm = tm + tm.T
    for q, seed in ((2.0, 8), (0.5, 9)):
        o = case(f"n2vpp_tiny_p0.5_q{q:g}", tm, 0.5, q, 0.0, seed, 6, 20, n_prob_samples=60)
        assert np.isnan(o["prob_vals"]).any(), "the tiny-weight graph must reach NaN probabilities"


if __name__ == "__main__":
    main()
