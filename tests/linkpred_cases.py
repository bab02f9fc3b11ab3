"""The shared cases of the link-prediction tests (tests/test_linkpred_host.py, tests/test_gpu_linkpred.py): pair lists,
score arrays and graphs, the selftest hooks as functions, and the NumPy statements (pecanpy_amd/linkpred.py) computed once
per case.

Pair scores: a wavefront takes 64 pairs and stages 32 columns at a time, so m runs over {0, 1, 63, 64, 65, 1000} and (n, dim)
over (1, 1), (65, 37), (700, 128), (257, 515): below a 16-byte group, not a multiple of 4, whole chunks, many chunks and a
ragged last one.  AUC: a wavefront sorts 2048 keys and 256 lanes count, so (m, n) runs up to (5000, 3000).  Sampler: forced
batches of 64 and 100 candidates cut every answer in many places."""
import ctypes as C
import functools
import os

import numpy as np

from pecanpy_amd import _lib, linkpred

METRICS = ("cosine", "dot")
PAIR_SHAPES = ((1, 1), (65, 37), (700, 128), (257, 515))
PAIR_MS = (0, 1, 63, 64, 65, 1000)
AUC_SIZES = ((1, 1), (63, 65), (65, 63), (5000, 3000))
SAMPLE_MS = (0, 1, 64, 1000)
SAMPLE_BATCHES = (64, 100, 0)   # 0: the default
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


# ---- pair scores -------------------------------------------------------------------------------------------------------
def _matrix(rng, n, dim):
    """Mixed sign and magnitude (10^-3 .. 10^3 per value: the order of the additions shows); rows 0 and n // 2 all zero."""
    X = (rng.standard_normal((n, dim)) * 10.0 ** rng.integers(-3, 4, size=(n, dim))).astype(np.float32)
    if n > 2:
        X[0] = 0.0
        X[n // 2] = 0.0
    return X


@functools.lru_cache(maxsize=None)
def pair_case(n, dim, m, second):
    """``(A, B or None, u, v)``: random pairs; pairs 0 / 1 are ``u == v``, pairs 2 .. 4 one repeated pair, pairs 5 .. 7 meet
    the zero rows from either side and from both (as far as m reaches)."""
    rng = np.random.default_rng(1000 * n + dim + 7 * m + (1 if second else 0))
    A = _matrix(rng, n, dim)
    B = _matrix(rng, n + 3, dim) if second else None
    nb = n + 3 if second else n
    u, v = rng.integers(0, n, size=m).astype(np.uint32), rng.integers(0, nb, size=m).astype(np.uint32)
    planted = ((0, n - 1, n - 1), (1, 0, 0), (2, n // 3, n // 4), (3, n // 3, n // 4), (4, n // 3, n // 4), (5, 0, n - 1), (6, n - 1, n // 2), (7, 0, n // 2))
    for i, pu, pv in planted:
        if i < m:
            u[i], v[i] = pu, pv
    return A, B, u, v


def score_selftest(A, B, u, v, metric, on_device, dim_b=None):
    """``(rc, score)`` of pw_selftest_score_pairs; ``score`` is born NaN, so a refused call shows that nothing was written."""
    m = len(u)
    score = np.full(m, np.nan)
    u, v = np.ascontiguousarray(u, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
    rc = _lib.load().pw_selftest_score_pairs(int(on_device), 0, _ptr(A), A.shape[0], _ptr(B), 0 if B is None else B.shape[0], A.shape[1],
                                             (B if B is not None else A).shape[1] if dim_b is None else dim_b, _ptr(u), _ptr(v), m,
                                             _lib.KNN_METRICS[metric], _ptr(score))
    return rc, score


@functools.lru_cache(maxsize=None)
def score_statement(n, dim, m, second, metric):
    A, B, u, v = pair_case(n, dim, m, second)
    s = linkpred.score_pairs_host(A, u, v, metric=metric, other=B)
    s.setflags(write=False)
    return s


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- AUC ---------------------------------------------------------------------------------------------------------------
HAND = (np.array([0.1, 0.4, 0.35, 0.8]), np.array([0.1, 0.35]))   # wins: 0 + 2 + 1 + 2 = 5; ties: 0.1 and 0.35 = 2; auc 12 / 16
HAND_ANSWER = (0.75, 5, 2)


@functools.lru_cache(maxsize=None)
def auc_cases():
    """name -> (pos, neg)"""
    rng = np.random.default_rng(77)
    cases = {}
    for m, n in AUC_SIZES:
        cases[f"normal-{m}x{n}"] = (rng.standard_normal(m), rng.standard_normal(n))
    cases["all-equal-63x65"] = (np.full(63, 0.25), np.full(65, 0.25))
    seven = np.array([-2.5, -1.0, -0.0, 0.0, 0.5, 0.5000000000000001, 3.0])
    cases["seven-values-5000x3000"] = (rng.choice(seven, size=5000), rng.choice(seven, size=3000))
    zeros = np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0])
    cases["signed-zeros-65x63"] = (rng.choice(zeros, size=65), rng.choice(zeros, size=63))
    infs = np.array([np.inf, -np.inf, 0.0, 1e308, -1e308, 1.0])
    cases["infinities-63x65"] = (rng.choice(infs, size=63), rng.choice(infs, size=65))
    sub = rng.integers(-6, 7, size=(2, 200)).astype(np.float64) * 5e-324
    cases["subnormals-200x200"] = (sub[0], sub[1])
    cases["hand-4x2"] = HAND
    for p, q in cases.values():
        p.setflags(write=False)
        q.setflags(write=False)
    return cases


def auc_selftest(pos, neg, on_device):
    """``(rc, wins, ties)`` of pw_selftest_auc; the counts are born as 0xDEAD."""
    pos, neg = np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(neg, dtype=np.float64)
    out = (C.c_uint64 * 2)(0xDEAD, 0xDEAD)
    rc = _lib.load().pw_selftest_auc(int(on_device), 0, _ptr(pos), pos.size, _ptr(neg), neg.size, out)
    return rc, int(out[0]), int(out[1])


@functools.lru_cache(maxsize=None)
def auc_statement(name):
    return linkpred.auc_host(*auc_cases()[name])


# ---- sampler -----------------------------------------------------------------------------------------------------------
def _csr(n, edges):
    """Ascending duplicate-free CSR of the ordered pairs ``edges``."""
    rows = [[] for _ in range(n)]
    for a, b in edges:
        rows[a].append(b)
    rows = [sorted(set(r)) for r in rows]
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.array([x for r in rows for x in r], dtype=np.uint32)


def _both(pairs):
    return [(a, b) for a, b in pairs] + [(b, a) for a, b in pairs]


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> (indptr, indices)"""
    z = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    g = {"karate": (z["indptr"].astype(np.uint32), z["indices"].astype(np.uint32))}
    g["ring-97"] = _csr(97, _both([(i, (i + 1) % 97) for i in range(97)]))
    g["star-65"] = _csr(65, _both([(0, i) for i in range(1, 65)]))
    rng = np.random.default_rng(5)   # directed: vertices 30 .. 39 have no out-edge (sinks), vertex 3 has a loop
    g["directed-sinks-40"] = _csr(40, [(int(a), int(b)) for a, b in zip(rng.integers(0, 30, 200), rng.integers(0, 40, 200))] + [(3, 3)])
    g["k5-minus-an-edge"] = _csr(5, [(a, b) for a in range(5) for b in range(5) if a != b and {a, b} != {1, 3}])
    return g


COMPLETE_5 = _csr(5, [(a, b) for a in range(5) for b in range(5) if a != b])
# The cap: the complete directed graph on 16 vertices less the arc CAP_ARC has ONE acceptable pair among 256, so a call for
# one non-edge may examine 16 * 256 + 64 = 4160 candidates.  Seed CAP_SEED's stream does not draw that pair among the 4160
# candidates from CAP_FIRST on (found by scanning the stream once), so the call passes the cap; one candidate earlier it ends
# at once.
CAP_SEED, CAP_ARC, CAP_FIRST = 1, (1, 0), 4717624   # candidate 4717623 is (1, 0); the next (1, 0) comes 4201 candidates later


def cap_graph(arc):
    return _csr(16, [(a, b) for a in range(16) for b in range(16) if a != b and (a, b) != tuple(arc)])


def sample_selftest(graph, seed, first, m, on_device, batch=0):
    """``(rc, u, v, used)`` of pw_selftest_sample_non_edges; the outputs are born as 0xDEADBEEF / 0xDEAD."""
    indptr, indices = graph
    u, v = np.full(m, 0xDEADBEEF, dtype=np.uint32), np.full(m, 0xDEADBEEF, dtype=np.uint32)
    used = C.c_uint64(0xDEAD)
    rc = _lib.load().pw_selftest_sample_non_edges(int(on_device), 0, _ptr(indptr), _ptr(indices), indptr.size - 1, seed, first, m, batch,
                                                  _ptr(u), _ptr(v), C.byref(used))
    return rc, u, v, int(used.value)


@functools.lru_cache(maxsize=None)
def sample_statement(name, seed, first, m):
    u, v, used = linkpred.sample_non_edges_host(*graphs()[name], m, seed, first)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v, used


def last_error():
    return _lib.load().pw_last_error()
