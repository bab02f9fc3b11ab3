"""Link prediction in device memory (csrc/linkpred.hip.h): the score of given pairs of rows, the exact AUC of two sets of
scores, and non-edges of a sparse graph drawn from the seeded stream -- each by one written definition that host and device
answer identically, bit for bit and integer for integer.

    with embed.KnnIndex(vectors) as index:
        pos = index.score_pairs(eu, ev, metric="dot")            # float64 tensor on the index's device
        nu, nv, used = g.sample_non_edges(len(eu), seed=7)       # g: SparseOTF / PreComp / ...
        value, wins, ties = linkpred.auc(pos, index.score_pairs(nu, nv, metric="dot"))

``holdout_edges`` (csrc/holdout.hip.h) is the stage in front of them: a seeded split of a sparse graph into a train graph and
held-out pairs, in device memory, so that graph -> split -> walks -> vectors -> scores -> AUC is a function of ``(graph, seed,
fraction)``:

        train, (eu, ev, ew), used = g.holdout_edges(0.5, seed=7)    # train: a graph of g's class, its walk handle installed
        nu, nv, _ = g.sample_non_edges(len(eu), seed=7, ...)        # negatives from the ORIGINAL graph g, not from train

``neighbour_scores`` (csrc/nbr_scores.hip.h) scores pairs by the graph alone -- common neighbours, Jaccard's coefficient,
Adamic-Adar, resource allocation, preferential attachment: the baseline rows of the protocol's table -- and ``baseline_auc`` is
their AUC.  In the protocol they are computed on the TRAIN graph: the original's edges include the answers.

        value, wins, ties = linkpred.baseline_auc(train, (eu, ev), (nu, nv), "adamic_adar")

``score_pairs_host``, ``auc_host``, ``sample_non_edges_host``, ``holdout_edges_host`` and ``neighbour_scores_host`` state the
definitions in NumPy, to be checked by eye; tests/test_linkpred_host.py, tests/test_gpu_linkpred.py, tests/test_holdout_host.py,
tests/test_gpu_holdout.py, tests/test_nbr_host.py and tests/test_gpu_nbr.py hold the library to them.  There is no CPU fallback: without a GPU
the device entry points raise ``PwError`` as every other one does."""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib

__all__ = ["score_pairs", "auc", "sample_non_edges", "link_auc", "score_pairs_host", "auc_host", "sample_non_edges_host",
           "candidate_cap", "holdout_edges", "holdout_edges_host", "holdout_threshold", "neighbour_scores", "neighbour_degrees",
           "degree_table", "neighbour_scores_host", "neighbour_degrees_host", "degree_table_host", "baseline_auc", "classifier_auc", "HEURISTICS"]

# the kinds of ``neighbour_scores``; the two after the first three are ``weighted`` with a table of the degrees
HEURISTICS = ("common_neighbours", "jaccard", "preferential_attachment", "adamic_adar", "resource_allocation", "weighted")


def _check_value(rc):
    """``_lib.check`` with PW_ERR_INVALID as a ``ValueError`` and PW_ERR_UNSUPPORTED as a ``NotImplementedError``."""
    if rc in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED):
        msg = _lib.load().pw_last_error()
        raise (ValueError if rc == _lib.ERR_INVALID else NotImplementedError)(msg.decode() if msg else "invalid argument")
    _lib.check(rc)


def _need_device(lib):
    if int(lib.pw_device_count()) <= 0:
        raise _lib.PwError("no HIP device visible (libpecanpy_amd needs a GPU; there is no CPU fallback)")


def _metric_id(metric):
    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be 'cosine' or 'dot', not {metric!r}")
    return _lib.KNN_METRICS[metric]


def _rows_host(x, name):
    """Row numbers on the host -- a list, an array or a CPU tensor of integers -- as a uint32 array."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype == object or x.dtype.kind not in "iu" or x.ndim != 1:
        raise ValueError(f"{name} must be a one-dimensional array of integers")
    if x.size and (int(x.min()) < 0 or int(x.max()) >= 2 ** 32):
        bad = int(np.flatnonzero((x < 0) | (x >= 2 ** 32))[0])
        raise ValueError(f"row number {name}[{bad}] = {int(x[bad])} is no row number")
    return np.ascontiguousarray(x, dtype=np.uint32)


def _rows_device(x, name, dev):
    """Row numbers as an int32 tensor on ``dev`` holding the uint32 bits; a CUDA tensor stays on the device."""
    import torch

    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.device != dev:
            raise ValueError(f"{name} must be on the host or on {dev}, not on {x.device}")
        if x.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16, torch.int8) or x.dim() != 1:
            raise ValueError(f"{name} must be a one-dimensional tensor of integers")
        if x.numel():
            lo, hi = int(x.min()), int(x.max())
            if lo < 0 or hi >= 2 ** 32:
                raise ValueError(f"row number {lo if lo < 0 else hi} in {name} is no row number")
        return x.to(torch.int64).to(torch.int32).contiguous()   # (the low 32 bits: uint32 as the library reads them)
    return torch.from_numpy(_rows_host(x, name).view(np.int32)).to(dev)


# ---- the three definitions in NumPy ------------------------------------------------------------------------------------
def _dots(A, B):
    """``dot(A[i], B[i])`` for every i: float64 products of the float32 values, k ascending from +0.0, one rounding per
    addition (``knn_host``'s ``dots`` order)."""
    acc = np.zeros(A.shape[0])
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    for k in range(A.shape[1]):
        acc += A64[:, k] * B64[:, k]
    return acc


def score_pairs_host(vectors, u, v, metric="cosine", other=None):
    """The NumPy statement of the pair score: ``score[i] = score(A[u[i]], B[v[i]])`` with ``A = vectors`` and ``B = other``
    (default ``A``), float64 ``[m]``.  ``dot`` sums the float64 products of the float32 values with k ascending from +0.0;
    ``norm = sqrt(dot(x, x))``; ``cosine = dot / (norm(a) * norm(b))``, +0.0 where that product is 0.  A row number outside
    its matrix is a ``ValueError`` naming the first position (``u`` before ``v``)."""
    A = np.asarray(vectors)
    B = A if other is None else np.asarray(other)
    for X in (A, B):
        if X.dtype != np.float32 or X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("vectors must be float32[n, dim]")
    if A.shape[1] != B.shape[1]:
        raise ValueError(f"the two matrices have dim {A.shape[1]} and {B.shape[1]}")
    metric_id = _metric_id(metric)
    u, v = _rows_host(u, "u"), _rows_host(v, "v")
    if u.shape != v.shape:
        raise ValueError(f"u and v must have one length, not {u.size} and {v.size}")
    bad = np.flatnonzero((u >= A.shape[0]) | (v >= B.shape[0]))
    if bad.size:
        i = int(bad[0])
        which, row, n = ("u", u[i], A.shape[0]) if u[i] >= A.shape[0] else ("v", v[i], B.shape[0])
        raise ValueError(f"row number {which}[{i}] = {int(row)} is outside the {n} rows")
    with np.errstate(all="ignore"):
        s = _dots(A[u], B[v])
        if metric_id == _lib.KNN_METRICS["cosine"]:
            den = np.sqrt(_dots(A[u], A[u])) * np.sqrt(_dots(B[v], B[v]))
            s = np.where(den == 0.0, 0.0, s / np.where(den == 0.0, 1.0, den))
    return s


def _auc_value(wins, ties, m, n):
    return float(Fraction(2 * wins + ties, 2 * m * n))


def auc_host(pos, neg):
    """The NumPy statement of the exact AUC: ``(auc, wins, ties)`` with ``wins = #{(i, j): pos[i] > neg[j]}`` and ``ties =
    #{(i, j): pos[i] == neg[j]}`` as Python integers (IEEE comparison: ``-0.0 == +0.0``, infinities are ordinary values) and
    ``auc = float(Fraction(2 wins + ties, 2 m n))``: one rounding, so a function of the inputs alone.  A NaN is a
    ``ValueError`` naming the first (``pos`` before ``neg``)."""
    pos, neg = np.asarray(pos, dtype=np.float64).ravel(), np.asarray(neg, dtype=np.float64).ravel()
    m, n = pos.size, neg.size
    if m < 1 or n < 1:
        raise ValueError("both arrays need at least one score")
    for name, x in (("pos", pos), ("neg", neg)):
        bad = np.flatnonzero(np.isnan(x))
        if bad.size:
            raise ValueError(f"{name}[{int(bad[0])}] is a NaN")
    s = np.sort(neg + 0.0)   # (-0.0 + 0.0 = +0.0: one zero, as the comparison sees them)
    lb = np.searchsorted(s, pos + 0.0, side="left")
    ub = np.searchsorted(s, pos + 0.0, side="right")
    wins = sum(int(x) for x in lb)
    ties = sum(int(x) for x in ub) - wins
    return _auc_value(wins, ties, m, n), wins, ties


def candidate_cap(m, n_nodes, acceptable):
    """The most candidates a call for ``m`` non-edges examines: ``16 * ceil(m N^2 / A) + 64``, at most ``2^62``."""
    need = -(-(m * n_nodes * n_nodes) // acceptable)
    return 2 ** 62 if need >= 2 ** 57 else 16 * need + 64


def sample_non_edges_host(indptr, indices, m, seed, first_candidate=0):
    """The plain-loop statement of the non-edge sampler: ``(u, v, candidates_used)``.  With ``w`` the tempered words of
    ``RandomState(seed)`` (``pw_mt_words``) candidate ``c``, counted from ``first_candidate``, is ``u = (w[2c] * N) >> 32``,
    ``v = (w[2c+1] * N) >> 32``; it is accepted when ``u != v`` and ``v`` is not in row ``u``.  The first ``m`` accepted
    candidates, in order -- pairs may repeat -- and one past the last candidate examined, minus ``first_candidate``.  A graph
    without an off-diagonal non-edge and a call that would pass ``candidate_cap`` are ``ValueError``s."""
    indptr, indices = np.asarray(indptr).astype(np.int64), np.asarray(indices).astype(np.int64)
    n = indptr.size - 1
    rows = [set(indices[indptr[r]:indptr[r + 1]].tolist()) for r in range(n)]
    loops = sum(1 for r in range(n) if r in rows[r])
    acceptable = n * (n - 1) - (int(indptr[n]) - loops)
    if acceptable == 0:
        raise ValueError(f"the graph of {n} vertices has no off-diagonal non-edge")
    m = int(m)
    if m == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0
    cap = candidate_cap(m, n, acceptable)
    lib = _lib.load()
    us, vs, c = [], [], 0
    words, have0 = np.zeros(0, np.uint32), 0
    while len(us) < m:
        if c >= cap:
            raise ValueError(f"{cap} candidates examined (the cap) gave {len(us)} of the {m} non-edges asked for")
        if c >= have0 + words.size // 2:
            have0, words = c, np.zeros(2 * min(1 << 14, cap - c), dtype=np.uint32)
            _lib.check(lib.pw_mt_words(int(seed) & 0xFFFFFFFF, 2 * (int(first_candidate) + c), words.size, C.c_void_p(words.ctypes.data)))
        cu = (int(words[2 * (c - have0)]) * n) >> 32
        cv = (int(words[2 * (c - have0) + 1]) * n) >> 32
        if cu != cv and cv not in rows[cu]:
            us.append(cu)
            vs.append(cv)
        c += 1
    return np.array(us, dtype=np.uint32), np.array(vs, dtype=np.uint32), c


def holdout_threshold(fraction):
    """``int(Fraction(fraction) * 2**32)`` for ``0 <= fraction < 1``: the uint32 a stream word is compared with.  Exact integer
    arithmetic (a float is taken for the binary fraction it is), no float multiply."""
    f = Fraction(fraction)
    if not 0 <= f < 1:
        raise ValueError(f"fraction must lie in [0, 1), not {fraction!r}")
    return int(f * 2 ** 32)


def holdout_edges_host(indptr, indices, data, fraction, seed, directed=False, protect=True, first_word=0):
    """The plain-loop statement of the edge hold-out: ``((train_indptr, train_indices, train_data), (u, v, weight),
    words_used)``.  ``data`` may be ``None`` (every weight 1.0).

    With ``w`` the tempered words of ``RandomState(seed)`` (``pw_mt_words``) and ``threshold = holdout_threshold(fraction)``:
    a UNIT is an entry ``r -> c`` with ``r != c`` of a directed graph, and an entry with ``r < c`` of an undirected one, whose
    mate ``c -> r`` must exist (``ValueError`` naming the first entry position without one) and shares its fate.  Self loops
    stay.  With ``protect`` a unit is protected when it sits at the first non-loop entry of its row -- for an undirected unit:
    of either of its two rows, the mate's position counting for the lower one -- so every row that had a non-loop entry keeps
    one.  The unit at entry position ``e`` is held out iff ``w[first_word + e] < threshold`` and it is not protected.  The
    train CSR keeps every other entry in order; the list has the held units in ascending position, ``weight`` the unit's own
    entry's; ``words_used = nnz``.  ``holdout_edges_host.last_stats``: ``units`` and ``protected`` of the last call."""
    indptr, indices = np.asarray(indptr).astype(np.int64), np.asarray(indices).astype(np.int64)
    n = indptr.size - 1
    nnz = int(indptr[n])
    weights = np.ones(nnz, dtype=np.float32) if data is None else np.asarray(data, dtype=np.float32)
    threshold = holdout_threshold(fraction)
    words = np.zeros(nnz, dtype=np.uint32)
    if nnz:
        _lib.check(_lib.load().pw_mt_words(int(seed) & 0xFFFFFFFF, int(first_word), nnz, C.c_void_p(words.ctypes.data)))
    row_of = np.repeat(np.arange(n), np.diff(indptr))
    position = {(int(row_of[e]), int(indices[e])): e for e in range(nnz)}

    def first(r):   # the position of the first non-loop entry of row r, None when there is none
        s = int(indptr[r])
        if s < indptr[r + 1] and indices[s] == r:
            s += 1
        return s if s < indptr[r + 1] else None

    keep, held, units, protected = np.ones(nnz, dtype=bool), [], 0, 0
    for e in range(nnz):
        r, c = int(row_of[e]), int(indices[e])
        if r == c:
            continue
        if directed:
            mate, safe = None, e == first(r)
        else:
            mate = position.get((c, r))
            if mate is None:
                raise ValueError(f"the CSR is not symmetric: the entry at position {e} has no mate")
            if r > c:
                continue
            safe = e == first(r) or mate == first(c)
        safe = bool(protect) and safe
        units += 1
        protected += int(safe)
        if int(words[e]) < threshold and not safe:
            held.append(e)
            keep[e] = False
            if mate is not None:
                keep[mate] = False
    train_indptr = np.zeros(n + 1, dtype=np.uint32)
    train_indptr[1:] = np.cumsum(np.bincount(row_of[keep], minlength=n)) if nnz else 0
    held = np.array(held, dtype=np.int64)
    holdout_edges_host.last_stats = {"units": units, "protected": protected}
    return ((train_indptr, indices[keep].astype(np.uint32), weights[keep]),
            (row_of[held].astype(np.uint32), indices[held].astype(np.uint32), weights[held]), nnz)


# ---- the neighbourhood heuristics, stated plainly (csrc/nbr_scores.hip.h) ---------------------------------------------------------
def _degree_function(kind, degrees):
    """``f(d)`` of the DISTINCT degrees ``d >= 2`` given, in NumPy on the host: ``1 / ln d`` (Adamic-Adar) or ``1 / d`` (resource
    allocation), float64.  The one place either function is evaluated, for the device path and the statement alike."""
    x = np.asarray(degrees).astype(np.float64)
    if kind == "adamic_adar":
        return 1.0 / np.log(x)
    if kind == "resource_allocation":
        return 1.0 / x
    raise ValueError(f"a degree table is 'adamic_adar' or 'resource_allocation', not {kind!r}")


def _check_heuristic(kind, table):
    if kind not in HEURISTICS:
        raise ValueError(f"kind must be one of {', '.join(HEURISTICS)}, not {kind!r}")
    if kind == "weighted" and table is None:
        raise ValueError("kind 'weighted' needs table=, a float64 value per vertex")
    if kind != "weighted" and table is not None:
        raise ValueError(f"table= belongs to kind 'weighted'; {kind!r} builds its own")


def _neighbour_sets(indptr, indices):
    indptr, indices = np.asarray(indptr).astype(np.int64), np.asarray(indices).astype(np.int64)
    n = indptr.size - 1
    return [set(indices[indptr[x]:indptr[x + 1]].tolist()) - {x} for x in range(n)]


def neighbour_degrees_host(indptr, indices):
    """``d(x) = |N(x)|`` as uint32 ``[N]``: the entries of row ``x`` other than ``x`` itself."""
    return np.array([len(s) for s in _neighbour_sets(indptr, indices)], dtype=np.uint32)


def degree_table_host(indptr, indices, kind):
    """The statement of ``degree_table``: float64 ``[N]``, ``t[z] = f(d(z))`` -- ``1 / ln d`` (``adamic_adar``) or ``1 / d``
    (``resource_allocation``), NumPy's value on the distinct degrees -- and ``0.0`` where ``d(z) < 2``."""
    deg = neighbour_degrees_host(indptr, indices)
    distinct = np.unique(deg)
    distinct = distinct[distinct >= 2]
    value = dict(zip(distinct.tolist(), _degree_function(kind, distinct).tolist()))
    return np.array([value.get(int(d), 0.0) for d in deg], dtype=np.float64)


def neighbour_scores_host(indptr, indices, u, v, kind, table=None):
    """The plain-loop statement of the neighbourhood heuristics: float64 ``[m]``.  ``N(x)`` = the entries of row ``x`` other
    than ``x`` itself (a Python set; weights are not looked at; a directed graph's out-row), ``d(x) = |N(x)|``, ``C = N(u) & N(v)``,
    ``cn = |C|``:

    ``common_neighbours``         ``float(cn)``
    ``jaccard``                   ``cn / (d(u) + d(v) - cn)``, one division; ``0.0`` when the denominator is 0
    ``preferential_attachment``   ``float(d(u) * d(v))``: the integer product, one rounding
    ``weighted``                  ``s = 0.0; for z in sorted(C): s = s + table[z]`` -- ascending, one rounding per addition
    ``adamic_adar`` / ``resource_allocation``   ``weighted`` with ``degree_table_host``

    ``u[i] == v[i]``, repeated pairs and edges are pairs like any other.  A row number outside the graph is a ``ValueError`` naming
    the first position (``u`` before ``v``)."""
    _check_heuristic(kind, table)
    nbrs = _neighbour_sets(indptr, indices)
    n = len(nbrs)
    u, v = _rows_host(u, "u"), _rows_host(v, "v")
    if u.shape != v.shape:
        raise ValueError(f"u and v must have one length, not {u.size} and {v.size}")
    bad = np.flatnonzero((u >= n) | (v >= n))
    if bad.size:
        i = int(bad[0])
        which, row = ("u", u[i]) if u[i] >= n else ("v", v[i])
        raise ValueError(f"row number {which}[{i}] = {int(row)} is outside the {n} rows")
    if kind in ("adamic_adar", "resource_allocation"):
        table = degree_table_host(indptr, indices, kind)
    if table is not None:
        table = np.asarray(table, dtype=np.float64)
        if table.shape != (n,):
            raise ValueError(f"table must hold one float64 per vertex ({n}), not shape {list(table.shape)}")
    score = np.zeros(u.size, dtype=np.float64)
    with np.errstate(all="ignore"):
        for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
            common = nbrs[a] & nbrs[b]
            cn, da, db = len(common), len(nbrs[a]), len(nbrs[b])
            if kind == "common_neighbours":
                score[i] = float(cn)
            elif kind == "jaccard":
                score[i] = cn / (da + db - cn) if da + db - cn else 0.0
            elif kind == "preferential_attachment":
                score[i] = float(da * db)
            else:
                s = np.float64(0.0)
                for z in sorted(common):
                    s = s + table[z]
                score[i] = s
    return score


# ---- the device entry points -------------------------------------------------------------------------------------------
def score_pairs(index, u, v, metric="cosine", other=None):
    """``KnnIndex.score_pairs``: a float64 ``[m]`` tensor on the index's device, ``score(A[u[i]], B[v[i]])`` with ``A`` the index's
    rows and ``B`` those of ``other`` (another ``KnnIndex`` of the same ``dim`` on the same device; default: the index
    itself).  ``u`` / ``v``: row numbers, torch or NumPy integer arrays, on the GPU or not.  ``u[i] == v[i]`` and repeated
    pairs are pairs like any other."""
    import torch

    handle = index._open()
    metric_id = _metric_id(metric)
    if other is not None and other.dim != index.dim:
        raise ValueError(f"the two indexes have dim {index.dim} and {other.dim}")
    if other is not None and other.device != index.device:
        raise ValueError(f"the two indexes are on devices {index.device} and {other.device}")
    dev = index._torch_device()
    d_u, d_v = _rows_device(u, "u", dev), _rows_device(v, "v", dev)
    if d_u.shape != d_v.shape:
        raise ValueError(f"u and v must have one length, not {d_u.numel()} and {d_v.numel()}")
    score = torch.empty(d_u.numel(), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()   # the row numbers were produced on torch's stream
    _check_value(_lib.load().pw_knn_score_pairs_device(handle, other._open() if other is not None else None, C.c_void_p(d_u.data_ptr()),
                                                       C.c_void_p(d_v.data_ptr()), d_u.numel(), metric_id, C.c_void_p(score.data_ptr())))
    return score


def _scores_device(x, name, dev):
    import torch

    if isinstance(x, torch.Tensor):
        if x.is_cuda and dev is not None and x.device != dev:
            raise ValueError(f"{name} must be on the host or on {dev}, not on {x.device}")
        if not x.dtype.is_floating_point:
            raise ValueError(f"{name} must hold floating-point scores, not {x.dtype}")
        t = x
    else:
        a = np.asarray(x)
        if a.dtype.kind != "f":
            raise ValueError(f"{name} must hold floating-point scores, not {a.dtype}")
        t = torch.from_numpy(np.array(a, dtype=np.float64, order="C"))   # (a copy: torch wants a writable array)
    return t.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()


def auc(pos, neg, device=None):
    """``(auc, wins, ties)`` of the positives' and the negatives' scores, counted on the GPU (``pw_auc_device``): ``wins =
    #{pos[i] > neg[j]}``, ``ties = #{pos[i] == neg[j]}`` as Python integers, ``auc = float(Fraction(2 wins + ties, 2 m n))``.
    Inputs already on the device stay there; host arrays are uploaded (to ``device``, default that of a CUDA input, else 0).
    A NaN is a ``ValueError`` naming the first."""
    import torch

    lib = _lib.load()
    _need_device(lib)
    dev = next((x.device for x in (pos, neg) if isinstance(x, torch.Tensor) and x.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", int(device or 0))
    elif device is not None and int(device) != dev.index:
        raise ValueError(f"the scores live on {dev}, the call was asked for device {int(device)}")
    d_pos, d_neg = _scores_device(pos, "pos", dev), _scores_device(neg, "neg", dev)
    m, n = d_pos.numel(), d_neg.numel()
    out = (C.c_uint64 * 2)()
    torch.cuda.current_stream(dev).synchronize()   # the scores were produced on torch's stream
    _check_value(lib.pw_auc_device(dev.index, C.c_void_p(d_pos.data_ptr()), m, C.c_void_p(d_neg.data_ptr()), n, out))
    wins, ties = int(out[0]), int(out[1])
    return _auc_value(wins, ties, m, n), wins, ties


def sample_non_edges(graph, m, seed, first_candidate=0):
    """``Base.sample_non_edges``: ``(u, v, candidates_used)`` -- two int64 ``[m]`` tensors on the graph's device and a Python
    integer -- the first ``m`` candidates of ``seed``'s stream from ``first_candidate`` on that are neither a loop nor an edge
    (``sample_non_edges_host`` states the rule).  The draws are independent, so accepted pairs MAY REPEAT.  A second call with
    ``first_candidate`` advanced by ``candidates_used`` continues the sequence.  Dense graphs: ``NotImplementedError``."""
    import torch

    eng = graph._get_engine()
    if eng.kind != "csr":
        raise NotImplementedError("sample_non_edges needs a sparse (CSR) graph")
    m = int(m)
    if not 0 <= m < 2 ** 32:
        raise ValueError(f"m = {m} outside 0 .. 2^32 - 1")
    dev = torch.device("cuda", eng.device)
    d_u = torch.empty(m, dtype=torch.int32, device=dev)
    d_v = torch.empty(m, dtype=torch.int32, device=dev)
    used = C.c_uint64(0)
    torch.cuda.current_stream(dev).synchronize()
    _check_value(_lib.load().pw_sample_non_edges_device(eng._h, int(seed) & 0xFFFFFFFF, int(first_candidate), m, C.c_void_p(d_u.data_ptr()),
                                                        C.c_void_p(d_v.data_ptr()), C.byref(used)))
    return d_u.to(torch.int64) & 0xFFFFFFFF, d_v.to(torch.int64) & 0xFFFFFFFF, int(used.value)


def holdout_edges(graph, fraction, seed, directed=False, protect=True, first_word=0):
    """``Base.holdout_edges``: ``(train_graph, (u, v, weight), words_used)`` -- a seeded split of a sparse graph's edges on the GPU
    (``pw_holdout_edges_device``; ``holdout_edges_host`` states the rule).  Each edge -- each undirected edge once, both of its
    entries together; ``directed=True``: each entry -- is held out when its word of ``seed``'s stream lies below ``fraction``,
    unless ``protect`` keeps it as the first non-loop entry of a row: no vertex that had an edge loses all of them.

    ``train_graph`` is an object of ``graph``'s class with the same ``p``, ``q``, ``workers``, ``extend``, ``gamma``,
    ``random_state``, device and node IDs, its host ``indptr`` / ``indices`` / ``data`` filled from the device CSR and the walk
    handle installed: its first ``simulate_walks`` uploads nothing.  ``u``, ``v`` (int64; ``u < v`` unless ``directed``) and
    ``weight`` (float32) are tensors on the graph's device in ascending entry position, directly what ``score_pairs`` takes.
    ``words_used`` added to ``first_word`` draws an independent split in a later call.  ``graph`` is not modified;
    ``graph.last_holdout_stats`` records the counts and the stage times.

    NEGATIVES come from ``sample_non_edges`` of the ORIGINAL graph: the train graph's non-edges include the held-out edges.
    Dense graphs: ``NotImplementedError``; an undirected call on a CSR that is not symmetric: ``ValueError``."""
    import time

    import torch

    from .engine import WalkEngine, _csr_dev_shape, _csr_engine

    eng = graph._get_engine()
    if eng.kind != "csr":
        raise NotImplementedError("holdout_edges needs a sparse (CSR) graph")
    threshold = holdout_threshold(fraction)
    words_used = int(graph.indptr[-1])
    lib = _lib.load()
    dev = torch.device("cuda", eng.device)
    c, h = C.c_void_p(), C.c_void_p()
    stage = (C.c_double * 3)()
    t0 = time.perf_counter()
    _check_value(lib.pw_holdout_edges_device(eng._h, int(bool(directed)), int(seed) & 0xFFFFFFFF, int(first_word), threshold, int(bool(protect)),
                                             C.byref(c), C.byref(h), stage))
    t1 = time.perf_counter()
    try:
        counts = [C.c_uint64(0) for _ in range(3)]
        _lib.check(lib.pw_holdout_dev_shape(h, *[C.byref(x) for x in counts]))
        held, units, protected = (int(x.value) for x in counts)
        d_u = torch.empty(held, dtype=torch.int32, device=dev)
        d_v = torch.empty(held, dtype=torch.int32, device=dev)
        d_w = torch.empty(held, dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(lib.pw_holdout_dev_fill(h, C.c_void_p(d_u.data_ptr()), C.c_void_p(d_v.data_ptr()), C.c_void_p(d_w.data_ptr())))
        n, nnz = _csr_dev_shape(lib, c)[:2]
        t2 = time.perf_counter()
        train_eng, _, _ = _csr_engine(WalkEngine, lib, c, n, nnz, eng.device)
    finally:
        lib.pw_holdout_dev_destroy(h)
        lib.pw_csr_dev_destroy(c)
    train = type(graph)(graph.p, graph.q, graph.workers, graph.verbose, graph.extend, graph.gamma, graph.random_state)
    train.device = graph.device
    train.indptr, train.indices, train.data = train_eng.csr
    train.set_node_ids(graph.nodes)
    train._engine = train_eng
    train._engine_key = (train._graph_key(), train._device_index())
    graph.last_holdout_stats = {"held": held, "units": units, "protected": protected, "train_nnz": nnz, "words_used": words_used,
                                "expand_ms": stage[0], "flag_ms": stage[1], "scan_compact_ms": stage[2], "split_call_ms": (t1 - t0) * 1e3,
                                "handle_ms": (time.perf_counter() - t2) * 1e3}
    return train, (d_u.to(torch.int64) & 0xFFFFFFFF, d_v.to(torch.int64) & 0xFFFFFFFF, d_w), words_used


def _csr_engine_of(graph, what):
    eng = graph._get_engine()
    if eng.kind != "csr":
        raise NotImplementedError(f"{what} needs a sparse (CSR) graph")
    return eng


def neighbour_degrees(graph):
    """``d(x) = |N(x)|`` -- the entries of row ``x`` other than ``x`` itself -- as an int64 ``[N]`` tensor on the graph's device
    (``pw_nbr_degrees_device``).  Dense graphs: ``NotImplementedError``."""
    import torch

    eng = _csr_engine_of(graph, "neighbour_degrees")
    dev = torch.device("cuda", eng.device)
    d_deg = torch.empty(eng.n_nodes, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    _check_value(_lib.load().pw_nbr_degrees_device(eng._h, C.c_void_p(d_deg.data_ptr())))
    return d_deg.to(torch.int64) & 0xFFFFFFFF


def degree_table(graph, kind):
    """The table of ``adamic_adar`` (``1 / ln d(z)``) or ``resource_allocation`` (``1 / d(z)``), ``0.0`` where ``d(z) < 2``: a
    float64 ``[N]`` tensor on the graph's device.  The degrees are counted and reduced to their distinct values on the device
    (``neighbour_degrees``, ``torch.unique``); those few values cross to the host, where NumPy evaluates the function -- the
    device's ``log`` is no part of any result -- and the values go back and are gathered there."""
    import torch

    _degree_function(kind, [2])   # (an unknown kind is refused before anything runs)
    deg = neighbour_degrees(graph)
    distinct, inverse = torch.unique(deg, return_inverse=True)
    d_host = distinct.cpu().numpy()
    value = np.zeros(d_host.size, dtype=np.float64)
    value[d_host >= 2] = _degree_function(kind, d_host[d_host >= 2])
    return torch.from_numpy(value).to(deg.device)[inverse].contiguous()


def neighbour_scores(graph, u, v, kind, table=None):
    """``Base.neighbour_scores``: the neighbourhood heuristic ``kind`` of every pair ``(u[i], v[i])`` as a float64 ``[m]`` tensor
    on the graph's device -- what ``auc`` takes (``pw_nbr_scores_device``; ``neighbour_scores_host`` states the rule).  ``kind``:
    ``common_neighbours``, ``jaccard``, ``preferential_attachment``, ``adamic_adar``, ``resource_allocation``, or ``weighted`` with
    ``table=``, a float64 value per vertex (a tensor on the graph's device stays there), summed over the common neighbours in
    ascending order.  ``u`` / ``v``: row numbers as ``score_pairs`` takes them.  Stored weights are not looked at; a self loop is no
    neighbour.  In the link-prediction protocol call it on the TRAIN graph of ``holdout_edges``, not on the original.  Dense
    graphs: ``NotImplementedError``; a row number outside the graph: ``ValueError`` naming the position."""
    import torch

    _check_heuristic(kind, table)
    eng = _csr_engine_of(graph, "neighbour_scores")
    dev = torch.device("cuda", eng.device)
    d_table = None
    if kind in ("adamic_adar", "resource_allocation"):
        d_table = degree_table(graph, kind)
    elif kind == "weighted":
        d_table = _scores_device(table, "table", dev)
        if d_table.numel() != eng.n_nodes:
            raise ValueError(f"table must hold one float64 per vertex ({eng.n_nodes}), not {d_table.numel()}")
    d_u, d_v = _rows_device(u, "u", dev), _rows_device(v, "v", dev)
    if d_u.shape != d_v.shape:
        raise ValueError(f"u and v must have one length, not {d_u.numel()} and {d_v.numel()}")
    score = torch.empty(d_u.numel(), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()   # the row numbers and the table were produced on torch's stream
    _check_value(_lib.load().pw_nbr_scores_device(eng._h, C.c_void_p(d_u.data_ptr()), C.c_void_p(d_v.data_ptr()), d_u.numel(),
                                                  _lib.NBR_KINDS.get(kind, _lib.NBR_KINDS["weighted"]),
                                                  C.c_void_p(d_table.data_ptr()) if d_table is not None else None, C.c_void_p(score.data_ptr())))
    return score



def _pairs(p, name):
    if isinstance(p, (tuple, list)) and len(p) == 2:
        return p[0], p[1]
    if hasattr(p, "shape") and len(p.shape) == 2 and p.shape[1] == 2:
        return p[:, 0], p[:, 1]
    if hasattr(p, "shape") and len(p.shape) == 2 and p.shape[0] == 2:
        return p[0], p[1]
    raise ValueError(f"{name} must be (u, v) or an integer array of shape [m, 2] or [2, m]")


def link_auc(index_or_session, pos_pairs, neg_pairs, metric="dot", against="context"):
    """``(auc, wins, ties)`` of the scores of ``pos_pairs`` against those of ``neg_pairs`` -- each ``(u, v)`` or an integer
    array ``[m, 2]`` / ``[2, m]`` -- scored by a ``KnnIndex`` (``against`` is ignored) or an ``SgnsSession`` (``against`` as
    ``SgnsSession.score_pairs``): ``score_pairs`` twice, then ``auc``."""
    from . import embed

    if isinstance(index_or_session, embed.KnnIndex):
        def score(u, v):
            return index_or_session.score_pairs(u, v, metric=metric)
    else:
        def score(u, v):
            return index_or_session.score_pairs(u, v, metric=metric, against=against)
    if not isinstance(index_or_session, embed.KnnIndex) and against == "context":
        with index_or_session.knn_index("vectors") as a, index_or_session.knn_index("context") as b:   # one snapshot for both calls
            return auc(a.score_pairs(*_pairs(pos_pairs, "pos_pairs"), metric=metric, other=b),
                       a.score_pairs(*_pairs(neg_pairs, "neg_pairs"), metric=metric, other=b))
    return auc(score(*_pairs(pos_pairs, "pos_pairs")), score(*_pairs(neg_pairs, "neg_pairs")))


def baseline_auc(graph, pos_pairs, neg_pairs, kind, table=None):
    """``(auc, wins, ties)`` of the neighbourhood heuristic ``kind`` on ``graph``: ``neighbour_scores`` of ``pos_pairs`` and of
    ``neg_pairs`` -- each ``(u, v)`` or an integer array ``[m, 2]`` / ``[2, m]`` -- then ``auc``.  ``graph`` is the TRAIN graph of
    ``holdout_edges``; the negatives come from ``sample_non_edges`` of the original."""
    return auc(neighbour_scores(graph, *_pairs(pos_pairs, "pos_pairs"), kind, table=table),
               neighbour_scores(graph, *_pairs(neg_pairs, "neg_pairs"), kind, table=table))


def _pair_rows(p, name, dev):
    u, v = _pairs(p, name)
    return _rows_device(u, f"{name}.u", dev), _rows_device(v, f"{name}.v", dev)


def classifier_auc(index, train_pos, train_neg, test_pos, test_neg, op, l2, other=None):
    """``(auc, wins, ties, model)``: the classifier row of the protocol's table.  ``classify.fit`` on ``op`` of the train pairs --
    label 1 for ``train_pos``, 0 for ``train_neg``, concatenated positives first -- then the model's decision values of
    ``test_pos`` against those of ``test_neg`` through ``auc``.  Each pair set is ``(u, v)`` or an integer array ``[m, 2]`` /
    ``[2, m]``, on the GPU or not; ``index`` is a ``KnnIndex`` (``other``: a second one for ``v``'s rows)."""
    import torch

    from . import classify

    dev = index._torch_device()
    (pu, pv), (nu, nv) = _pair_rows(train_pos, "train_pos", dev), _pair_rows(train_neg, "train_neg", dev)
    y = torch.cat([torch.ones(pu.numel(), dtype=torch.uint8, device=dev), torch.zeros(nu.numel(), dtype=torch.uint8, device=dev)])
    model = classify.fit(index, torch.cat([pu, nu]), torch.cat([pv, nv]), y, op, l2=l2, other=other)
    value, wins, ties = auc(model.decision_function(index, *_pair_rows(test_pos, "test_pos", dev), other=other),
                            model.decision_function(index, *_pair_rows(test_neg, "test_neg", dev), other=other))
    return value, wins, ties, model
