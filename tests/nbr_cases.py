"""The shared cases of the neighbourhood-baseline tests (tests/test_nbr_host.py, tests/test_gpu_nbr.py): three small graphs
from a fixed seed, pair lists, tables, the selftest hooks as functions, and the plain statement
(``linkpred.neighbour_scores_host``) computed once per case.

The kernel (csrc/nbr_scores.hip.h) takes 64 pairs per wavefront, settles a pair in one lane when its shorter row has at most
``short_max`` entries (by a merge when the longer row is under 4 times as long, by searches otherwise) and by the whole
wavefront, 64 entries of the shorter row at a time, otherwise.  So m runs over {0, 1, 63, 64, 65, 200}, the rows of ``hubs`` have
0, 1, 63, 64, 65, 129, 130, 600, 2000 and 4097 entries, and ``short_max`` is forced to 0, 1, 64, all-lane and the default."""
import ctypes as C
import functools

import numpy as np

from pecanpy_amd import _lib, linkpred

MS = (0, 1, 63, 64, 65, 200)
KINDS = ("common_neighbours", "jaccard", "preferential_attachment", "adamic_adar", "resource_allocation", "wide")
SHORT_MAXES = {"all-wavefront": 0, "one": 1, "sixty-four": 64, "all-lane": _lib.NBR_ALL_LANE, "default": -1}
GRAPHS = ("hubs", "er-loops", "directed")
HUBS_N = 4300


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _csr(n, rows):
    """Ascending duplicate-free CSR of ``rows``: vertex -> an iterable of entries."""
    rows = [sorted(set(int(x) for x in rows.get(r, ()))) for r in range(n)]
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.array([x for r in rows for x in r], dtype=np.uint32)


def _hubs():
    """Rows chosen freely (a directed CSR: N(x) is the out-row).  Row 0: the 4097 entries 4 .. 4100.  Row 1: 130 entries, all of
    them in row 0, the first (4) and the last (4100) among them: (0, 1) is a full-hit pair over three chunks of the wavefront
    form.  Row 2: 65 entries, none of them in row 1.  Vertex 3: isolated (no row, in no row).  Row 4: 2000 entries (under 4 times
    shorter than row 0: a lane merges), row 5: 600 (a lane searches).  Rows 10 .. 14: 1, 63, 64, 65, 129 entries.  Rows 20 and 21
    hold 20, 21 and 22 each, and row 22 holds 22: self loops on u, on v and on a common neighbour.  The other rows: 0 .. 8
    entries."""
    rng = np.random.default_rng(20240611)
    n = HUBS_N
    pool = np.array([x for x in range(4, n)], dtype=np.int64)   # (vertex 3 is in no row)
    rows = {r: rng.choice(pool, size=int(rng.integers(0, 9)), replace=False) for r in range(23, n)}
    rows[0] = range(4, 4101)
    rows[1] = [4, 4100] + rng.choice(np.arange(5, 4100), size=128, replace=False).tolist()
    free = np.setdiff1d(pool, np.array(rows[1]))
    rows[2] = rng.choice(free, size=65, replace=False)
    rows[4] = rng.choice(pool, size=2000, replace=False)
    rows[5] = rng.choice(pool, size=600, replace=False)
    for r, k in ((10, 1), (11, 63), (12, 64), (13, 65), (14, 129)):
        rows[r] = rng.choice(pool, size=k, replace=False)
    rows[20] = [20, 21, 22, 30, 31]
    rows[21] = [20, 21, 22, 31, 40]
    rows[22] = [22, 50]
    return _csr(n, rows)


def _er_loops():
    rng = np.random.default_rng(300)
    n = 300
    upper = np.triu(rng.random((n, n)) < 0.1, 1)
    adj = upper | upper.T
    loops = rng.choice(n, size=20, replace=False)
    adj[loops, loops] = True
    return _csr(n, {r: np.flatnonzero(adj[r]) for r in range(n)})


def _directed():
    rng = np.random.default_rng(200)
    n = 200
    adj = rng.random((n, n)) < 0.06
    adj[170:] = False          # sinks: no out-row
    adj[7, 7] = True           # (the diagonal is random as well: a dozen loops)
    return _csr(n, {r: np.flatnonzero(adj[r]) for r in range(n)})


@functools.lru_cache(maxsize=None)
def graph(name):
    """``(indptr, indices)``, read-only"""
    g = {"hubs": _hubs, "er-loops": _er_loops, "directed": _directed}[name]()
    for a in g:
        a.setflags(write=False)
    return g


def rows_of(name):
    indptr, indices = graph(name)
    return [indices[indptr[r]:indptr[r + 1]] for r in range(indptr.size - 1)]


@functools.lru_cache(maxsize=None)
def pairs(name, m):
    """``(u, v)`` uint32 ``[m]``.  In front, as far as m reaches: the hub-hub pair (the two longest rows) in both orders, ``u ==
    v`` on the hub, an edge, a non-edge, one pair three times, and for ``hubs`` the planted pairs of its docstring; behind them
    random pairs, every second one between endpoints of random entries (degree-biased: the hubs come often)."""
    indptr, indices = graph(name)
    n = indptr.size - 1
    rng = np.random.default_rng(1000 * len(name) + m)
    length = np.diff(indptr.astype(np.int64))
    h0, h1 = (int(x) for x in np.argsort(-length, kind="stable")[:2])
    rows = rows_of(name)
    edge = next((r, int(rows[r][-1])) for r in range(n) if rows[r].size and int(rows[r][-1]) != r)
    non_edge = next((r, c) for r in range(n - 1, -1, -1) for c in range(n) if r != c and c not in set(rows[r].tolist()))
    planted = [(h0, h1), (h1, h0), (h0, h0), edge, non_edge, (h1, 6), (h1, 6), (h1, 6)]
    if name == "hubs":
        planted += [(0, 1), (1, 0), (1, 2), (0, 2), (20, 21), (21, 20), (3, 0), (3, 3), (0, 5), (5, 4), (10, 0), (11, 0), (0, 12), (13, 0), (14, 1),
                    (12, 13), (22, 20), (1, 1)]
    row_of_entry = np.repeat(np.arange(n), length)
    u, v = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    biased = rng.integers(0, indices.size, size=(2, m))
    u[1::2], v[1::2] = row_of_entry[biased[0]][1::2], indices[biased[1]][1::2]
    for i, (a, b) in enumerate(planted[:m]):
        u[i], v[i] = a, b
    u, v = u.astype(np.uint32), v.astype(np.uint32)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


@functools.lru_cache(maxsize=None)
def table(name, kind):
    """The float64 ``[N]`` table of a weighted kind: the two degree tables, and ``wide``: both signs, magnitudes spread over 40
    binades, so that the order of the additions shows in the bits."""
    indptr, indices = graph(name)
    if kind == "wide":
        rng = np.random.default_rng(40)
        n = indptr.size - 1
        t = rng.choice([-1.0, 1.0], size=n) * (1.0 + rng.random(n)) * 2.0 ** rng.integers(-20, 21, size=n)
    else:
        t = linkpred.degree_table_host(indptr, indices, kind)
    t.setflags(write=False)
    return t


def abi_kind(kind):
    """``(PW_NBR_* number, statement's kind, needs a table)`` of a case kind"""
    weighted = kind in ("adamic_adar", "resource_allocation", "wide")
    return _lib.NBR_KINDS["weighted" if weighted else kind], "weighted" if weighted else kind, weighted


def selftest(name, u, v, kind, on_device, short_max=-1, tab="case", kind_number=None):
    """``(rc, score)`` of pw_selftest_nbr_scores; ``score`` is born NaN, so a refused call shows that nothing was written."""
    indptr, indices = graph(name)
    number, _, weighted = abi_kind(kind)
    t = (table(name, kind) if weighted else None) if isinstance(tab, str) else tab
    u, v = np.ascontiguousarray(u, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
    score = np.full(len(u), np.nan)
    rc = _lib.load().pw_selftest_nbr_scores(int(on_device), 0, _ptr(indptr), _ptr(indices), indptr.size - 1, _ptr(u), _ptr(v), len(u),
                                            number if kind_number is None else kind_number, _ptr(t), short_max, _ptr(score))
    return rc, score


def degrees_selftest(name, on_device):
    indptr, indices = graph(name)
    deg = np.full(indptr.size - 1, 0xDEADBEEF, dtype=np.uint32)
    rc = _lib.load().pw_selftest_nbr_degrees(int(on_device), 0, _ptr(indptr), _ptr(indices), indptr.size - 1, _ptr(deg))
    return rc, deg


@functools.lru_cache(maxsize=None)
def statement(name, m, kind):
    """``neighbour_scores_host`` of the case, computed once, read-only"""
    indptr, indices = graph(name)
    _, host_kind, weighted = abi_kind(kind)
    s = linkpred.neighbour_scores_host(indptr, indices, *pairs(name, m), host_kind, table=table(name, kind) if weighted else None)
    s.setflags(write=False)
    return s


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def last_error():
    return _lib.load().pw_last_error()
