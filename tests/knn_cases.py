"""The shared cases of the nearest-neighbour tests (tests/test_knn_host.py, tests/test_gpu_knn.py): the smallest shapes at
which a tile, a list or a tie rule can go wrong, each with its reference (tests/knn_ref.py) computed once.

QT = 8 queries share a wavefront's registers and 64 rows a row group, so n runs over {1, 2, 63, 64, 65, 257, 700, 5000}, nq
over {1, QT, QT + 1, 33} and topn over {1, 10, 128} (128 > n at the small n).  dim is 128 and 37 everywhere, the other
dims (1, 3, 130, 515: below a 16-byte group, not a multiple of 4, past one chunk of 32 columns by 2, many chunks) at n = 257."""
import ctypes as C
import functools

import numpy as np

import knn_ref

QT = 8
METRICS = ("cosine", "dot")
METRIC_ID = {"dot": 0, "cosine": 1}


class Case:
    def __init__(self, name, X, queries=None, rows=None, topn=10, exclude_self=None):
        self.name, self.X, self.topn = name, np.ascontiguousarray(X, dtype=np.float32), topn
        self.queries = None if queries is None else np.ascontiguousarray(queries, dtype=np.float32)
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
        self.exclude_self = (rows is not None) if exclude_self is None else bool(exclude_self)

    @property
    def nq(self):
        return len(self.rows) if self.rows is not None else self.queries.shape[0]

    def __repr__(self):
        return self.name


def _normal(rng, n, dim):
    return rng.standard_normal((n, dim)).astype(np.float32)


def _rows(rng, n, nq):
    return rng.integers(0, n, size=nq).astype(np.uint32)


def _plant(X, n):
    """Exact ties: rows 0, 64, 256 and n - 1 (those that exist) become row 1 scaled by 1, 2, 0.25 and 2^-3 -- equal cosine
    scores, in different blocks and workgroups -- and the row behind each a plain duplicate of row 1."""
    if n < 3:
        return X
    for at, scale in ((0, 1.0), (64, 2.0), (256, 0.25), (n - 1, 0.125)):
        if at < n and at != 1:
            X[at] = X[1] * np.float32(scale)
            if at + 1 < n and at + 1 != 1:
                X[at + 1] = X[1]
    return X


def _build():
    cases = []
    rng = np.random.default_rng(20240917)
    nqs, topns = (1, QT, QT + 1, 33), (1, 10, 128)
    k = 0
    for n in (1, 2, 63, 64, 65, 257, 700, 5000):
        for dim in (128, 37):
            nq, topn = nqs[k % 4], topns[k % 3]
            X = _normal(rng, n, dim)
            if k % 2:
                cases.append(Case(f"normal-n{n}-d{dim}-rows{nq}-top{topn}", X, rows=_rows(rng, n, nq), topn=topn))
            else:
                cases.append(Case(f"normal-n{n}-d{dim}-vec{nq}-top{topn}", X, queries=_normal(rng, nq, dim), topn=topn))
            k += 1
    for dim, nq, topn in ((1, 33, 10), (3, QT + 1, 128), (130, QT, 10), (515, 1, 1)):
        cases.append(Case(f"normal-n257-d{dim}-rows{nq}-top{topn}", _normal(rng, 257, dim), rows=_rows(rng, 257, nq), topn=topn))

    for n, dim, topn in ((257, 37, 10), (700, 128, 128), (65, 128, 10)):
        X = _plant(_normal(rng, n, dim), n)
        rows = np.array([r for r in (1, 0, 64, 65, 256, n - 1, 5) if r < n], dtype=np.uint32)
        cases.append(Case(f"ties-n{n}-d{dim}-top{topn}", X, rows=rows, topn=topn))
        cases.append(Case(f"ties-n{n}-d{dim}-top{topn}-vector-equal-to-a-row", X, queries=X[[1, 5]], topn=topn))
    X = np.tile(_normal(rng, 1, 37), (257, 1))
    cases.append(Case("all-rows-equal-n257", X, rows=np.array([0, 3, 64, 256], dtype=np.uint32), topn=10))
    cases.append(Case("all-rows-equal-n257-keep-self", X, rows=np.array([0, 200], dtype=np.uint32), topn=128, exclude_self=False))
    A = np.abs(_normal(rng, 130, 37)) + np.float32(0.5)
    cases.append(Case("x-and-minus-x", np.concatenate([A, -A]), rows=np.array([0, 129, 130, 259, 64], dtype=np.uint32), topn=10))
    cases.append(Case("every-score-negative", A, queries=-np.abs(_normal(rng, QT + 1, 37)) - np.float32(0.5), topn=128))
    X = _normal(rng, 257, 37)
    X[[0, 7, 64, 256]] = 0.0
    Q = _normal(rng, 3, 37)
    Q[1] = 0.0
    cases.append(Case("zero-rows-zero-query-vec", X, queries=Q, topn=10))
    cases.append(Case("zero-rows-by-row", X, rows=np.array([0, 7, 1, 256], dtype=np.uint32), topn=128))
    X = np.zeros((257, 37), dtype=np.float32)
    X[np.arange(257), np.arange(257) % 37] = rng.choice(np.array([1.0, -1.0, 2.0], dtype=np.float32), size=257)
    cases.append(Case("one-hot", X, rows=np.array([0, 36, 37, 64, 256], dtype=np.uint32), topn=10))
    sign = rng.choice(np.array([1.0, -1.0], dtype=np.float32), size=(257, 37))
    X = sign * np.exp2(rng.integers(-60, 61, size=(257, 37))).astype(np.float32)
    cases.append(Case("powers-of-two", X, rows=_rows(rng, 257, QT + 1), topn=10))
    cases.append(Case("powers-of-two-vec", X, queries=X[:2] * np.float32(0.5), topn=1))
    return cases


CASES = _build()
IDS = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def _reference(index, metric):
    c = CASES[index]
    idx, score = knn_ref.knn_ref(c.X, queries=c.queries, rows=c.rows, topn=c.topn, metric=metric, exclude_self=c.exclude_self)
    idx.setflags(write=False)
    score.setflags(write=False)
    return idx, score


def reference(case, metric):
    """``knn_ref`` of a case, computed once and read-only."""
    return _reference(CASES.index(case), metric)


def selftest(case, metric, on_device, tiles=None, device=0):
    """``pw_selftest_knn`` -> ``(rc, idx int64 with -1 padding, score)``; the outputs are born as a pattern no answer holds."""
    from pecanpy_amd import _lib

    lib = _lib.load()
    nq = case.nq
    idx = np.full((nq, case.topn), 0xDEADBEEF, dtype=np.uint32)
    score = np.full((nq, case.topn), np.nan)
    t = _lib.PwKnnTiles(*tiles) if tiles is not None else None
    rc = lib.pw_selftest_knn(int(on_device), device, C.c_void_p(case.X.ctypes.data), case.X.shape[0], case.X.shape[1],
                             C.c_void_p(case.queries.ctypes.data) if case.queries is not None else None,
                             C.c_void_p(case.rows.ctypes.data) if case.rows is not None else None, nq, case.topn, METRIC_ID[metric],
                             int(case.exclude_self), C.byref(t) if t is not None else None, C.c_void_p(idx.ctypes.data),
                             C.c_void_p(score.ctypes.data))
    out = idx.astype(np.int64)
    out[idx == 0xFFFFFFFF] = -1
    return rc, out, score


def assert_same(got_idx, got_score, want_idx, want_score):
    """idx equal, score bit for bit."""
    assert got_idx.shape == want_idx.shape and got_score.shape == want_score.shape
    assert np.array_equal(got_idx, want_idx), np.argwhere(got_idx != want_idx)[:5]
    assert np.array_equal(got_score.view(np.uint64), np.asarray(want_score).view(np.uint64)), np.argwhere(got_score != want_score)[:5]
