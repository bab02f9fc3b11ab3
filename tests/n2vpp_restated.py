"""NumPy restatement of node2vec++ (the reference's experimental.Node2vecPlusPlus, experimental.py:31-102) and of the
single-stream walk loop around it (pecanpy.py:133-206).  Test infrastructure: the fixtures tests/golden/n2vpp/n2vpp_*.npz come from
the reference itself (tests/golden/make_golden_n2vpp.py); tests/test_n2vpp_host.py checks that this restatement reproduces
them, and the GPU tests compare the walk kernel with it on graphs too large for a fixture.

What pins it to the reference under Numba: the row sum is a sequential float64 loop (``np.cumsum(...)[-1]``), the bias is
evaluated literally in the reference's order, and the step is ``np.searchsorted`` (NaN-last order) on ``np.cumsum`` of the
normalised row; a draw no partial sum reaches takes the last neighbour (the walk engine's clamp of the read past the row).
"""
import numpy as np


def noise_thresholds(data, gamma):
    """``DenseRWGraph.get_noise_thresholds`` (rw/dense_rw.py:11-19): float32, NaN for a row without non-zeros."""
    n = data.shape[0]
    nonzero = data != 0
    thr = np.zeros(n, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for i in range(n):
                w = data[i, nonzero[i]]
                thr[i] = w.mean() + gamma * w.std()
    return np.maximum(thr, 0)


def normalized_probs(data, nonzero, p, q, cur, prev, thr):
    """experimental.py:62-102 with ``w.sum()`` as a sequential loop."""
    w = data[cur].copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if prev is not None:
            wp = data[prev]
            out = nonzero[cur] & (wp < thr)
            out[prev] = False
            t = wp[out] / thr[out]
            t = 1 - t.clip(0, 1) if q < 1 else t.clip(0, 1)
            b = w[out] / thr[out]
            scale = np.abs(1 - 1 / q)
            offset = np.minimum(1, 1 / q)
            alpha = t * b / (1 + (b - 1)) * scale + offset
            w[out] *= alpha
            w[prev] /= p
        u = w[nonzero[cur]]
        tot = np.cumsum(u)[-1]
        return u / tot


def step(data, nonzero, p, q, cur, prev, thr, r):
    """``move_forward`` with the draw ``r`` (experimental.py:42-58); the read past the row is clamped to the last neighbour."""
    probs = normalized_probs(data, nonzero, p, q, cur, prev, thr)
    with np.errstate(invalid="ignore"):
        k = int(np.searchsorted(np.cumsum(probs), r))
    nbrs = np.nonzero(nonzero[cur])[0]
    return int(nbrs[min(k, nbrs.size - 1)])


def start_array(n, num_walks, seed):
    """pecanpy.py:135-141."""
    starts = np.concatenate([np.arange(n, dtype=np.uint32)] * num_walks)
    np.random.seed(seed)
    np.random.shuffle(starts)
    return starts


def random_walks(data, p, q, gamma, seed, starts, walk_length, n_jobs=None, thr=None):
    """The reference's single-thread ``_random_walks`` (pecanpy.py:164-210) over the first ``n_jobs`` jobs of ``starts``:
    one MT19937 stream seeded with ``seed``, one ``random()`` per step."""
    data = np.asarray(data, dtype=np.float64)
    nonzero = data != 0
    has = nonzero.any(axis=1)
    if thr is None:
        thr = noise_thresholds(data, gamma)
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
        mat[i, 1] = step(data, nonzero, p, q, s, None, thr, np.random.random())
        for j in range(2, walk_length + 1):
            cur = int(mat[i, j - 1])
            if not has[cur]:
                mat[i, -1] = j
                break
            mat[i, j] = step(data, nonzero, p, q, cur, int(mat[i, j - 2]), thr, np.random.random())
    return mat
