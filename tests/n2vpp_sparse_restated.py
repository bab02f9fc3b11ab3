"""CSR NumPy restatement of node2vec++ on sparse graphs (experimental.SparseNode2vecPlusPlus).  Test infrastructure.

The contract: walks, probabilities and steps on a CSR graph with float32 weights ``A`` equal the reference's
experimental.Node2vecPlusPlus on ``A.toarray().astype(np.float64)``.  Every step here calls the dense restatement's
arithmetic (tests/n2vpp_restated.py) on a local dense problem: the columns of cur's row plus cur and prev, with prev's
weights looked up by ``np.searchsorted`` in prev's row.  Nothing of size N x N is formed, so graphs whose dense form would
not fit can be walked (one job at a time: slow, for the first few hundred jobs of a large graph).
"""
import warnings

import numpy as np

import n2vpp_restated as rs


def noise_thresholds(indptr, data, gamma):
    """``DenseRWGraph.get_noise_thresholds`` of the dense float64 form: each row's non-zeros widened to float64."""
    n = indptr.size - 1
    thr = np.zeros(n, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for i in range(n):
            w = np.asarray(data[indptr[i]:indptr[i + 1]], dtype=np.float64)
            w = w[w != 0]
            thr[i] = w.mean() + gamma * w.std()
    return np.maximum(thr, 0)


def _local(indptr, indices, data, cur, prev):
    """Local dense rows of cur and prev over the columns C = row(cur) + {cur, prev}: ({local row: float64 row}, C, local
    cur, local prev).  Only rows cur and prev are ever read by the dense restatement, so they are kept in a dict."""
    cs, ce = int(indptr[cur]), int(indptr[cur + 1])
    cols = np.asarray(indices[cs:ce], dtype=np.int64)
    extra = [cur] + ([] if prev is None else [prev])
    C = np.union1d(cols, np.array(extra, dtype=np.int64))
    ci = int(np.searchsorted(C, cur))
    wc = np.zeros(C.size, dtype=np.float64)
    wc[np.searchsorted(C, cols)] = np.asarray(data[cs:ce], dtype=np.float64)
    rows = {ci: wc}
    pi = None
    if prev is not None:
        pi = int(np.searchsorted(C, prev))
        ps, pe = int(indptr[prev]), int(indptr[prev + 1])
        prow = np.asarray(indices[ps:pe], dtype=np.int64)
        wp = np.zeros(C.size, dtype=np.float64)
        if prow.size:
            pos = np.searchsorted(prow, C)
            hit = (pos < prow.size) & (prow[np.minimum(pos, prow.size - 1)] == C)
            wp[hit] = np.asarray(data[ps + pos[hit]], dtype=np.float64)
        rows.setdefault(pi, wp)   # (prev == cur: the same row)
    return rows, C, ci, pi


def _nz(rows):
    return {k: v != 0 for k, v in rows.items()}


def normalized_probs(indptr, indices, data, p, q, cur, prev, thr):
    """The float64 probability vector over cur's row (CSR order) that the dense reference computes."""
    rows, C, ci, pi = _local(indptr, indices, data, cur, prev)
    return rs.normalized_probs(rows, _nz(rows), p, q, ci, pi, thr[C])


def step(indptr, indices, data, p, q, cur, prev, thr, r):
    """``move_forward`` with the draw ``r``; the read past the row is clamped to the last neighbour."""
    rows, C, ci, pi = _local(indptr, indices, data, cur, prev)
    return int(C[rs.step(rows, _nz(rows), p, q, ci, pi, thr[C], r)])


def random_walks(indptr, indices, data, p, q, gamma, seed, starts, walk_length, n_jobs=None, thr=None):
    """The reference's single-thread ``_random_walks`` (pecanpy.py:164-210) over the first ``n_jobs`` jobs of ``starts``."""
    indptr = np.asarray(indptr, dtype=np.int64)
    data = np.ones(len(indices), np.float32) if data is None else np.asarray(data, dtype=np.float32)
    if thr is None:
        thr = noise_thresholds(indptr, data, gamma)
    has = indptr[1:] > indptr[:-1]
    n_jobs = starts.size if n_jobs is None else int(n_jobs)
    mat = np.zeros((n_jobs, walk_length + 2), dtype=np.uint32)
    mat[:, 0] = starts[:n_jobs]
    mat[:, -1] = walk_length + 1
    np.random.seed(seed)
    for i in range(n_jobs):
        s = int(mat[i, 0])
        if not has[s]:
            mat[i, -1] = 1
            continue
        mat[i, 1] = step(indptr, indices, data, p, q, s, None, thr, np.random.random())
        for j in range(2, walk_length + 1):
            cur = int(mat[i, j - 1])
            if not has[cur]:
                mat[i, -1] = j
                break
            mat[i, j] = step(indptr, indices, data, p, q, cur, int(mat[i, j - 2]), thr, np.random.random())
    return mat


def csr_of(mat):
    """(indptr, indices, float32 data) of a dense matrix."""
    mat = np.asarray(mat)
    idx = np.nonzero(mat)
    indptr = np.concatenate([[0], np.cumsum((mat != 0).sum(1))]).astype(np.uint32)
    return indptr, idx[1].astype(np.uint32), mat[idx].astype(np.float32)
