"""The shared cases of the edge hold-out tests (tests/test_holdout_host.py, tests/test_gpu_holdout.py): graphs, parameters, the
selftest hook as a function, and the plain-loop statement (``linkpred.holdout_edges_host``) computed once per case.

The graphs are the smallest at which the kernels can go wrong: no entry at all, one edge, a path, a star whose hub row (300
entries) is longer than a wavefront and than a 256-lane workgroup and is searched from 300 one-entry rows, the karate club,
self loops in every place the rule names (a row that starts with its loop, a row that holds only its loop, a loop in the
middle of a row), a symmetric random graph with ``w(u, v) != w(v, u)`` so that the carried weight shows whose entry it was, a
directed random graph.  Word batches of 64 and 100 cut every graph but the smallest in many places."""
import ctypes as C
import functools
import os
from fractions import Fraction

import numpy as np

from pecanpy_amd import _lib, linkpred

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20
FRACTIONS = (Fraction(0), Fraction(1, 2), Fraction(2 ** 32 - 1, 2 ** 32))   # thresholds 0, 2^31, 2^32 - 1
PROTECTS = (True, False)
FIRST_WORDS = (0, 2 ** 33 + 5)
BATCHES = (64, 100, 0)   # 0: the default
U32_SENTINEL, COUNT_SENTINEL = 0xDEADBEEF, 0xDEAD


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _csr(n, entries, weight=None):
    """Ascending duplicate-free CSR of the ordered pairs ``entries``; ``weight(r, c)`` gives an entry's float32 or is None."""
    entries = sorted(set((int(a), int(b)) for a, b in entries))
    indptr = np.zeros(n + 1, dtype=np.uint32)
    for a, _ in entries:
        indptr[a + 1] += 1
    indptr = np.cumsum(indptr, dtype=np.uint32)
    indices = np.array([b for _, b in entries], dtype=np.uint32)
    data = None if weight is None else np.array([weight(a, b) for a, b in entries], dtype=np.float32)
    return indptr, indices, data


def _both(pairs):
    return [(a, b) for a, b in pairs] + [(b, a) for a, b in pairs]


def _asymmetric(a, b):
    """A float32 weight with ``w(a, b) != w(b, a)`` and no two entries alike (a, b < 1000)."""
    return np.float32(0.25 + a + b / 1024.0)


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> (indptr, indices, data or None, directed)"""
    z = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    g = {"single-vertex": _csr(1, []) + (False,),
         "one-edge": _csr(2, _both([(0, 1)])) + (False,),
         "path-5": _csr(5, _both([(i, i + 1) for i in range(4)])) + (False,),
         "star-300": _csr(301, _both([(0, i) for i in range(1, 301)])) + (False,),
         "karate": (z["indptr"].astype(np.uint32), z["indices"].astype(np.uint32), None, False),
         # row 0 = [0, 1, 2] starts with its loop, row 2 = [0, 1, 2, 3] has its loop mid-row, row 5 = [5] holds only its loop
         "self-loops": _csr(6, _both([(0, 1), (0, 2), (1, 2), (2, 3), (3, 4)]) + [(0, 0), (2, 2), (5, 5)], _asymmetric) + (False,)}
    rng = np.random.default_rng(41)
    a, b = rng.integers(0, 700, size=(2, 5200))
    g["er-700"] = _csr(700, _both([(x, y) for x, y in zip(a, b) if x != y]), _asymmetric) + (False,)   # about 10^4 entries
    a, b = rng.integers(0, 700, size=(2, 10000))   # loops stay in: about one entry in 700
    g["directed-700"] = _csr(700, list(zip(a, b)), _asymmetric) + (True,)
    for arrays in g.values():
        for x in arrays[:3]:
            if x is not None:
                x.setflags(write=False)
    return g


# the path 0 - 1 - 2 - 3 - 4 without the entry 3 -> 2: the entry 2 -> 3, at position 4, is the first without a mate
MISSING_MATE = _csr(5, [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 4), (4, 3)]) + (False,)
MISSING_AT = 4


def parameter_sets():
    """Every ``(fraction, protect, first_word)``."""
    return [(f, p, w) for f in FRACTIONS for p in PROTECTS for w in FIRST_WORDS]


class Result:
    """What one call of pw_selftest_holdout_edges left: ``rc``, the buffers as they are, and the cut views."""

    def __init__(self, rc, buffers, counts):
        self.rc, self.buffers = rc, buffers
        self.counts = tuple(int(x) for x in counts)   # train entries, held units, units, protected units
        kept, held = (self.counts[0], self.counts[1]) if rc == 0 else (0, 0)
        self.train = (buffers["indptr"], buffers["indices"][:kept], buffers["data"][:kept])
        self.held = (buffers["u"][:held], buffers["v"][:held], buffers["weight"][:held])

    def untouched(self):
        b = self.buffers
        return (all((b[k] == U32_SENTINEL).all() for k in ("indptr", "indices", "u", "v")) and np.isnan(b["data"]).all() and
                np.isnan(b["weight"]).all() and self.counts == (COUNT_SENTINEL,) * 4)


def selftest(graph, fraction, protect, first_word, on_device, batch=0, seed=SEED, directed=None):
    """pw_selftest_holdout_edges on ``graph``; every output is born as a sentinel (0xDEADBEEF, NaN, 0xDEAD)."""
    indptr, indices, data, graph_directed = graph
    n, nnz = indptr.size - 1, indices.size
    buffers = {"indptr": np.full(n + 1, U32_SENTINEL, dtype=np.uint32), "indices": np.full(nnz, U32_SENTINEL, dtype=np.uint32),
               "data": np.full(nnz, np.nan, dtype=np.float32), "u": np.full(nnz, U32_SENTINEL, dtype=np.uint32),
               "v": np.full(nnz, U32_SENTINEL, dtype=np.uint32), "weight": np.full(nnz, np.nan, dtype=np.float32)}
    counts = (C.c_uint64 * 4)(*(COUNT_SENTINEL,) * 4)
    rc = _lib.load().pw_selftest_holdout_edges(int(on_device), 0, _ptr(indptr), _ptr(indices), _ptr(data), n,
                                               int(graph_directed if directed is None else directed), seed, first_word,
                                               linkpred.holdout_threshold(fraction), int(protect), batch,
                                               *[_ptr(buffers[k]) for k in ("indptr", "indices", "data", "u", "v", "weight")], counts)
    return Result(rc, buffers, counts)


@functools.lru_cache(maxsize=None)
def statement(name, fraction, protect, first_word, seed=SEED):
    """``(train, held, (units, protected))`` of the plain-loop statement."""
    indptr, indices, data, directed = graphs()[name]
    train, held, used = linkpred.holdout_edges_host(indptr, indices, data, fraction, seed, directed=directed, protect=protect, first_word=first_word)
    assert used == indices.size
    stats = linkpred.holdout_edges_host.last_stats
    for x in train + held:
        x.setflags(write=False)
    return train, held, (stats["units"], stats["protected"])


def same_arrays(got, want):
    """Array for array: shape, dtype and every bit (float32 compared as its bits)."""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            return False
    return True


def equals_statement(result, name, fraction, protect, first_word):
    train, held, (units, protected) = statement(name, fraction, protect, first_word)
    return (result.rc == 0 and same_arrays(result.train, train) and same_arrays(result.held, held) and
            result.counts == (train[1].size, held[0].size, units, protected))


def last_error():
    return _lib.load().pw_last_error()
