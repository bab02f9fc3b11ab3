"""An independent naive reference of the nearest-neighbour definition (csrc/knn.hip.h): float64 loops with k
ascending and ``lexsort``.  It imports nothing from ``pecanpy_amd``."""
import numpy as np

NONE = -1


def dot_rows(q, X64):
    """dot(q, x) for every row x: (((0.0 + q[0] x[0]) + q[1] x[1]) + ...), one rounding per addition."""
    acc = np.zeros(X64.shape[0])
    for k in range(X64.shape[1]):
        acc = acc + float(q[k]) * X64[:, k]
    return acc


def norms(X):
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    acc = np.zeros(X64.shape[0])
    for k in range(X64.shape[1]):
        acc = acc + X64[:, k] * X64[:, k]
    return np.sqrt(acc)


def knn_ref(X, queries=None, rows=None, topn=10, metric="cosine", exclude_self=None):
    """``(idx int64[nq, topn], score float64[nq, topn])``, padded with -1 / -inf."""
    assert (queries is None) != (rows is None)
    X = np.asarray(X, dtype=np.float32)
    X64 = X.astype(np.float64)
    n = X.shape[0]
    if exclude_self is None:
        exclude_self = rows is not None
    Q = X[np.asarray(rows, dtype=np.int64)] if rows is not None else np.asarray(queries, dtype=np.float32)
    Q64 = Q.astype(np.float64)
    xn = norms(X)
    idx = np.full((Q.shape[0], topn), NONE, dtype=np.int64)
    score = np.full((Q.shape[0], topn), -np.inf)
    for i in range(Q.shape[0]):
        s = dot_rows(Q64[i], X64)
        if metric == "cosine":
            qn = float(np.sqrt(dot_rows(Q64[i], Q64[i:i + 1])[0]))
            den = qn * xn
            with np.errstate(all="ignore"):
                s = np.where(den == 0.0, 0.0, s / den)
        else:
            assert metric == "dot"
        cand = np.arange(n)
        if exclude_self and rows is not None:
            cand = cand[cand != int(rows[i])]
        order = cand[np.lexsort((cand, -s[cand]))][:topn]
        idx[i, :order.size] = order
        score[i, :order.size] = s[order]
    return idx, score
