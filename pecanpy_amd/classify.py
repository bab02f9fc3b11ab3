"""Exact binary logistic regression on embedding rows and pair operators (csrc/logit.hip.h): the classifier row of the
link-prediction table -- a binary operator on the two end points' vectors (average, Hadamard, weighted-L1, weighted-L2), a
logistic regression on the result, its decision value the score -- and node classification, the same trainer with the
operator "take the first row as it is" (``row``).

    with embed.KnnIndex(vectors) as index:
        model = classify.fit(index, u, v, y, "hadamard", l2=1e-3)        # pairs and labels stay in device memory
        z = model.decision_function(index, tu, tv)                         # float64 CUDA tensor
        value, wins, ties, model = linkpred.classifier_auc(index, train_pos, train_neg, test_pos, test_neg, "hadamard", 1e-3)
        models = classify.fit_one_vs_rest(index, rows, Y)                  # Y: [n, C] of 0 / 1

One evaluation -- loss, gradient, decision values -- is ONE written definition (the header of csrc/logit.hip.h)
that the kernels, the library's host build and ``logit_eval_host`` below answer bit for bit: the order of every sum is part
of it, and so are its own ``exp`` and ``log1p`` (``lg_exp_host``, ``lg_log1p_host``: ``+ - * /`` only, because libm's and the
device's do not agree in the last bit).  The optimiser (``_minimise``: L-BFGS, history 10, backtracking Armijo) is written once
in NumPy float64 over an ``evaluate(theta) -> (loss, grad)`` callable, so ``fit`` (device evaluations) and ``fit_host`` (the
NumPy statement) return the same theta bit for bit.  There is no CPU fallback: without a GPU the device entry points raise
``PwError`` as every other one does."""
import ctypes as C

import numpy as np

from . import _lib
from .linkpred import _check_value, _need_device, _rows_device, _rows_host

__all__ = ["OPERATORS", "lg_exp_host", "lg_log1p_host", "logit_eval_host", "logit_eval", "fit", "fit_host", "fit_one_vs_rest",
           "fit_one_vs_rest_host", "LogisticModel"]

OPERATORS = ("row", "average", "hadamard", "l1", "l2")
CHUNK = _lib.LOGIT_CHUNK
MAX_DIM = _lib.LOGIT_MAX_DIM
_BLOCK = 1 << 15   # samples whose features the statement holds at a time

_LOG2E, _LN2_HI, _LN2_LO = 1.4426950408889634, 6.93147180369123816490e-01, 1.90821492927058770002e-10
_EXP_COEF = (1.6059043836821613e-10, 2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06,
             2.48015873015873e-05, 0.0001984126984126984, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664,
             0.16666666666666666, 0.5, 1.0, 1.0)   # 1/13! .. 1/0!
_LOG1P_TERMS = 16


# ---- the definition in NumPy ---------------------------------------------------------------------------------------------
def lg_exp_host(x):
    """The definition's ``exp`` on ``[-708, 0]`` (``+0.0`` below): ``k = rint(x log2e)``, ``r = (x - k ln2_hi) - k ln2_lo``, the
    degree-13 Taylor polynomial by Horner, times ``2^k`` from the exponent bits.  Every operation is one NumPy ufunc: rounded
    on its own."""
    x = np.asarray(x, dtype=np.float64)
    xc = np.maximum(x, -708.0)
    k = np.rint(xc * _LOG2E)
    r = (xc - k * _LN2_HI) - k * _LN2_LO
    p = np.full(x.shape, _EXP_COEF[0])
    for c in _EXP_COEF[1:]:
        p = p * r + c
    two_k = ((k.astype(np.int64) + 1023) << 52).view(np.float64)
    return np.where(x < -708.0, 0.0, p * two_k)


def lg_log1p_host(t):
    """The definition's ``log1p`` on ``[0, 1]``: ``s = t / (2 + t)``, ``(2 s) (1 + s^2/3 + ... + s^30/31)`` by Horner, sixteen
    terms."""
    t = np.asarray(t, dtype=np.float64)
    s = t / (2.0 + t)
    w = s * s
    q = np.full(t.shape, 1.0 / (2 * _LOG1P_TERMS - 1))
    for n in range(_LOG1P_TERMS - 2, -1, -1):
        q = q * w + 1.0 / (2 * n + 1)
    return (2.0 * s) * q


def _feat(op, a, b):
    if op == "row":
        return a
    if op == "average":
        return (a + b) * 0.5
    if op == "hadamard":
        return a * b
    if op == "l1":
        return np.abs(a - b)
    d = a - b
    return d * d


def _sample(z, y):
    """``(r, l)`` of the definition: the residual ``d loss / d z`` and the loss of every sample."""
    x = np.where(y, -z, z)
    t = lg_exp_host(-np.abs(x))
    den = 1.0 + t
    q = np.where(x >= 0.0, 1.0 / den, t / den)
    return np.where(y, -q, q), np.where(x > 0.0, x, 0.0) + lg_log1p_host(t)


def _op_name(op):
    if op not in _lib.LOGIT_OPS:
        raise ValueError(f"op must be one of {', '.join(OPERATORS)}, not {op!r}")
    return op


def _theta_checked(theta, dim, l2):
    if dim > MAX_DIM:
        raise NotImplementedError(f"dim {dim} is above the trainer's cap of {MAX_DIM}")
    l2 = float(l2)
    if not (np.isfinite(l2) and l2 >= 0.0):
        raise ValueError("l2 must be finite and >= 0")
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.shape != (dim + 1,):
        raise ValueError(f"theta must be float64[{dim + 1}] = (w, bias), not shape {list(theta.shape)}")
    bad = np.flatnonzero(~np.isfinite(theta))
    if bad.size:
        raise ValueError(f"theta[{int(bad[0])}] is not finite")
    return theta, l2


def _labels_host(y, m):
    if hasattr(y, "detach"):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.dtype == object or y.dtype.kind not in "iub" or y.ndim != 1:
        raise ValueError("y must be a one-dimensional array of 0 / 1 integers")
    if y.size != m:
        raise ValueError(f"y must hold one label per sample ({m}), not {y.size}")
    return y


def logit_eval_host(A, B, u, v, y, op, theta, l2, return_z=False, _chunk=CHUNK, _descending=False):
    """The NumPy statement of one evaluation (the header of csrc/logit.hip.h): ``(loss, grad)`` -- a float and float64
    ``[dim + 1]`` -- and with ``return_z`` also ``z`` float64 ``[m]``; with ``y=None`` ``z`` alone.  ``A`` float32 ``[na, dim]``,
    ``B`` float32 ``[nb, dim]`` or ``None`` (``A``); ``v`` is not looked at by ``op="row"`` and may be ``None`` there.

    ``f = feat(op, A[u[i]], B[v[i]])`` in float64; ``z[i] = (((bias + w[0] f[0]) + w[1] f[1]) + ...)``; ``(r, l)`` of a sample by
    ``_sample``; inside a chunk of 1024 samples, i ascending from +0.0, ``P[c][k] += r[i] * f[i][k]``, ``P[c][dim] += r[i]``,
    ``PL[c] += l[i]``; the chunks added with c ascending from +0.0; ``grad[k] = G[k] / m + l2 w[k]``, ``grad[dim] = G[dim] / m``,
    ``loss = Lsum / m + (0.5 l2) (((0 + w[0]^2) + w[1]^2) + ...)``.  It is vectorised across chunks and columns and loops where
    the order matters: over the positions of a chunk, over k, over the chunks.  Every refusal of the definition is a
    ``ValueError`` naming the first offending element (``dim > 512``: ``NotImplementedError``).  (``_chunk`` / ``_descending``
    state a DIFFERENT order of the additions: what tests/test_logit_host.py shows to differ in bits.)"""
    op = _op_name(op)
    A = np.asarray(A)
    B = A if B is None else np.asarray(B)
    for X in (A, B):
        if X.dtype != np.float32 or X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("vectors must be float32[n, dim]")
    if A.shape[1] != B.shape[1]:
        raise ValueError(f"the two matrices have dim {A.shape[1]} and {B.shape[1]}")
    dim = A.shape[1]
    u = _rows_host(u, "u")
    m = u.size
    if not 1 <= m < 2 ** 40:
        raise ValueError("m must be in 1 .. 2^40 - 1")
    theta, l2 = _theta_checked(theta, dim, l2)
    if op == "row":
        v = u
    else:
        v = _rows_host(v, "v")
        if u.shape != v.shape:
            raise ValueError(f"u and v must have one length, not {u.size} and {v.size}")
    bad = np.flatnonzero((u >= A.shape[0]) | ((v >= B.shape[0]) if op != "row" else False))
    if bad.size:
        i = int(bad[0])
        which, row, n = ("u", u[i], A.shape[0]) if u[i] >= A.shape[0] else ("v", v[i], B.shape[0])
        raise ValueError(f"row number {which}[{i}] = {int(row)} is outside the {n} rows")
    if y is not None:
        y = _labels_host(y, m)
        bad = np.flatnonzero((y != 0) & (y != 1))
        if bad.size:
            raise ValueError(f"label y[{int(bad[0])}] = {int(y[bad[0]])} is neither 0 nor 1")
        y = y.astype(bool)
    w, bias = theta[:dim], theta[dim]

    def features(rows):
        if op == "row":
            return A[u[rows]].astype(np.float64)
        return _feat(op, A[u[rows]].astype(np.float64), B[v[rows]].astype(np.float64))

    with np.errstate(all="ignore"):
        z = np.empty(m)
        for i0 in range(0, m, _BLOCK):
            F = features(slice(i0, i0 + _BLOCK))
            acc = np.full(F.shape[0], bias)
            for k in range(dim):
                acc = acc + w[k] * F[:, k]
            z[i0:i0 + _BLOCK] = acc
        bad = np.flatnonzero(~np.isfinite(z))
        if bad.size:
            raise ValueError(f"the decision value z[{int(bad[0])}] is not finite")
        if y is None:
            return z
        r, ell = _sample(z, y)
        n_chunks = -(-m // _chunk)
        P = np.zeros((n_chunks, dim + 2))
        positions = range(_chunk - 1, -1, -1) if _descending else range(_chunk)
        for p in positions:   # position p of every chunk that has one
            rows = np.arange(p, m, _chunk)
            if rows.size == 0:
                continue
            rp = r[rows]
            P[:rows.size, :dim] += rp[:, None] * features(rows)
            P[:rows.size, dim] += rp
            P[:rows.size, dim + 1] += ell[rows]
        G = np.zeros(dim + 2)
        for c in (range(n_chunks - 1, -1, -1) if _descending else range(n_chunks)):
            G = G + P[c]
        grad = np.empty(dim + 1)
        grad[:dim] = G[:dim] / float(m) + l2 * w
        grad[dim] = G[dim] / float(m)
        pen = 0.0
        for k in range(dim):
            pen = pen + w[k] * w[k]
        loss = float(G[dim + 1] / float(m) + (0.5 * l2) * pen)
    return (loss, grad, z) if return_z else (loss, grad)


# ---- the device route ----------------------------------------------------------------------------------------------------
def _labels_device(y, m, dev):
    """Labels as a uint8 tensor on ``dev``; a value outside 0 .. 255 becomes 255, which the library refuses like any other
    label that is neither 0 nor 1."""
    import torch

    if isinstance(y, torch.Tensor) and y.is_cuda:
        if y.device != dev:
            raise ValueError(f"y must be on the host or on {dev}, not on {y.device}")
        if y.dtype.is_floating_point or y.dtype.is_complex or y.dim() != 1:
            raise ValueError("y must be a one-dimensional tensor of 0 / 1 integers")
        t = y
    else:
        t = torch.from_numpy(np.array(_labels_host(y, m), copy=True)).to(dev)
    if t.numel() != m:
        raise ValueError(f"y must hold one label per sample ({m}), not {t.numel()}")
    if t.dtype not in (torch.uint8, torch.bool):
        t = t.to(torch.int64)   # (255 does not fit every integer type)
        t = torch.where((t < 0) | (t > 255), torch.full_like(t, 255), t)
    return t.to(torch.uint8).contiguous()


class _DeviceProblem:
    """The pairs and labels of one problem in device memory, uploaded once for the evaluations of a fit."""

    def __init__(self, index, u, v, y, op, other=None):
        import torch

        self.index, self.other, self.op = index, other, _op_name(op)
        index._open()
        if other is not None and other.dim != index.dim:
            raise ValueError(f"the two indexes have dim {index.dim} and {other.dim}")
        if other is not None and other.device != index.device:
            raise ValueError(f"the two indexes are on devices {index.device} and {other.device}")
        self.dev = index._torch_device()
        self.d_u = _rows_device(u, "u", self.dev)
        self.m = self.d_u.numel()
        self.d_v = None
        if self.op != "row":
            self.d_v = _rows_device(v, "v", self.dev)
            if self.d_u.shape != self.d_v.shape:
                raise ValueError(f"u and v must have one length, not {self.d_u.numel()} and {self.d_v.numel()}")
        self.d_y = _labels_device(y, self.m, self.dev) if y is not None else None
        torch.cuda.current_stream(self.dev).synchronize()   # the pairs and labels were produced on torch's stream
        self.last_kernel_ms = None

    def evaluate(self, theta, l2, return_z=False, blocks=-1):
        import torch

        dim = self.index.dim
        theta, l2 = _theta_checked(theta, dim, l2)
        want_z = return_z or self.d_y is None
        z = torch.empty(self.m, dtype=torch.float64, device=self.dev) if want_z else None
        loss, grad, ms = C.c_double(float("nan")), np.full(dim + 1, np.nan), C.c_float(0.0)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        _check_value(_lib.load().pw_logit_eval_device_grid(
            self.index._open(), self.other._open() if self.other is not None else None, ptr(self.d_u), ptr(self.d_v), ptr(self.d_y), self.m,
            _lib.LOGIT_OPS[self.op], C.c_void_p(theta.ctypes.data), l2, C.byref(loss), C.c_void_p(grad.ctypes.data), ptr(z), int(blocks),
            C.byref(ms)))
        self.last_kernel_ms = float(ms.value)
        if self.d_y is None:
            return z
        return (loss.value, grad, z) if return_z else (loss.value, grad)


def logit_eval(index, u, v, y, op, theta, l2, other=None, return_z=False, blocks=-1):
    """One evaluation on the GPU over a ``KnnIndex`` (``other``: a second index for ``v``'s rows): ``(loss, grad)`` -- a float
    and a float64 NumPy ``[dim + 1]`` -- with ``return_z`` also ``z``, a float64 ``[m]`` CUDA tensor; with ``y=None`` ``z``
    alone.  ``u`` / ``v`` / ``y`` may be CUDA tensors, CPU tensors, arrays or lists.  ``logit_eval_host`` states what it answers,
    bit for bit; ``blocks`` forces the grid (no result depends on it)."""
    return _DeviceProblem(index, u, v, y, op, other).evaluate(theta, l2, return_z=return_z, blocks=blocks)


# ---- the optimiser: written once ---------------------------------------------------------------------------------------
def _minimise(evaluate, n, max_iter=200, gtol=1e-8, history=10):
    """L-BFGS (two-loop recursion, ``history`` pairs) in NumPy float64 from theta = 0 with a backtracking Armijo search: c1 =
    1e-4, halving, at most 30 trials, the first trial step ``1 / |g|_2`` in the first iteration and 1 afterwards.  Stops on
    ``|grad|_inf <= gtol`` (converged), on ``max_iter`` or on a failed line search.  A pair with ``s.y <= 0`` is not stored; a
    direction that does not descend is replaced by ``-g`` and the history dropped.  Returns ``(theta, converged, n_iter,
    n_eval, loss)``.  (The first trial step is 1 in every iteration but the first, also right after the history was dropped.)"""
    theta = np.zeros(n)
    loss, g = evaluate(theta)
    n_eval, n_iter, pairs = 1, 0, []
    converged = bool(np.max(np.abs(g)) <= gtol)
    while not converged and n_iter < max_iter:
        q = g.copy()
        alphas = []
        for s, yv, rho in reversed(pairs):
            a = rho * np.dot(s, q)
            alphas.append(a)
            q = q - a * yv
        if pairs:
            s, yv, _ = pairs[-1]
            q = q * (np.dot(s, yv) / np.dot(yv, yv))
        for (s, yv, rho), a in zip(pairs, reversed(alphas)):
            q = q + (a - rho * np.dot(yv, q)) * s
        d = -q
        slope = float(np.dot(g, d))
        if not slope < 0.0:
            pairs, d = [], -g
            slope = float(np.dot(g, d))
        step = 1.0 / float(np.sqrt(np.dot(g, g))) if n_iter == 0 else 1.0
        found = False
        for _ in range(30):
            cand = theta + step * d
            cand_loss, cand_g = evaluate(cand)
            n_eval += 1
            if cand_loss <= loss + 1e-4 * step * slope:
                found = True
                break
            step *= 0.5
        if not found:
            break
        s, yv = cand - theta, cand_g - g
        sy = float(np.dot(s, yv))
        if sy > 0.0:
            pairs.append((s, yv, 1.0 / sy))
            pairs = pairs[-history:]
        theta, loss, g = cand, cand_loss, cand_g
        n_iter += 1
        converged = bool(np.max(np.abs(g)) <= gtol)
    return theta, converged, n_iter, n_eval, float(loss)


class LogisticModel:
    """A fitted model: ``theta`` float64 ``[dim + 1]`` = (w, bias), ``op``, ``l2``, and what the optimiser reports --
    ``converged``, ``n_iter``, ``n_eval``, ``loss``."""

    def __init__(self, theta, op, l2, converged=False, n_iter=0, n_eval=0, loss=float("nan")):
        self.theta = np.ascontiguousarray(theta, dtype=np.float64)
        self.op, self.l2 = _op_name(op), float(l2)
        self.converged, self.n_iter, self.n_eval, self.loss = bool(converged), int(n_iter), int(n_eval), float(loss)

    def decision_function(self, index, u, v=None, other=None):
        """The decision values ``z`` of the pairs (of the rows ``u`` for ``op="row"``): a float64 ``[m]`` CUDA tensor."""
        return logit_eval(index, u, v, None, self.op, self.theta, 0.0, other=other)

    def decision_function_host(self, vectors, u, v=None, other=None):
        """The NumPy statement of ``decision_function``: float64 ``[m]``."""
        return logit_eval_host(vectors, other, u, v, None, self.op, self.theta, 0.0)

    def save(self, path):
        """A text file of settings: one ``name<TAB>value`` line for ``op``, ``l2``, ``converged``, ``n_iter``, ``n_eval``,
        ``loss``, then one line ``w<TAB>k<TAB>repr(float)`` per coefficient and ``bias<TAB>repr(float)``."""
        with open(path, "w") as f:
            f.write(f"op\t{self.op}\nl2\t{self.l2!r}\nconverged\t{int(self.converged)}\nn_iter\t{self.n_iter}\nn_eval\t{self.n_eval}\n"
                    f"loss\t{self.loss!r}\n")
            for k, w in enumerate(self.theta[:-1].tolist()):
                f.write(f"w\t{k}\t{w!r}\n")
            f.write(f"bias\t{float(self.theta[-1])!r}\n")

    @classmethod
    def load(cls, path):
        head, w, bias = {}, [], None
        with open(path) as f:
            for n, line in enumerate(f, 1):
                parts = line.rstrip("\n").split("\t")
                if parts[0] == "w" and len(parts) == 3 and int(parts[1]) == len(w):
                    w.append(float(parts[2]))
                elif parts[0] == "bias" and len(parts) == 2:
                    bias = float(parts[1])
                elif len(parts) == 2 and parts[0] in ("op", "l2", "converged", "n_iter", "n_eval", "loss"):
                    head[parts[0]] = parts[1]
                else:
                    raise ValueError(f"{path}:{n}: not a line of a model file: {line.rstrip()!r}")
        if bias is None or "op" not in head:
            raise ValueError(f"{path}: a model file needs an op line and a bias line")
        return cls(np.array(w + [bias]), head["op"], float(head.get("l2", 0.0)), bool(int(head.get("converged", 0))),
                   int(head.get("n_iter", 0)), int(head.get("n_eval", 0)), float(head.get("loss", "nan")))


def _fit(evaluate, dim, op, l2, max_iter, gtol):
    theta, converged, n_iter, n_eval, loss = _minimise(evaluate, dim + 1, max_iter=max_iter, gtol=gtol)
    return LogisticModel(theta, op, l2, converged, n_iter, n_eval, loss)


def fit(index, u, v, y, op, l2=1e-3, other=None, max_iter=200, gtol=1e-8):
    """A ``LogisticModel`` fitted on the GPU: the minimiser of ``mean log-loss + (l2 / 2) |w|^2`` over the features ``feat(op,
    A[u[i]], B[v[i]])`` of a ``KnnIndex`` (``other``: a second index for ``v``), labels ``y`` of 0 / 1.  The pairs and labels
    are uploaded once; every evaluation is ``logit_eval``.  ``fit_host`` returns the same model bit for bit."""
    problem = _DeviceProblem(index, u, v, y, op, other)
    if problem.d_y is None:
        raise ValueError("fit needs labels")
    return _fit(lambda theta: problem.evaluate(theta, l2), index.dim, op, l2, max_iter, gtol)


def fit_host(vectors, u, v, y, op, l2=1e-3, other=None, max_iter=200, gtol=1e-8):
    """``fit`` with every evaluation by the NumPy statement ``logit_eval_host`` (``vectors`` / ``other``: float32 matrices)."""
    if y is None:
        raise ValueError("fit needs labels")
    return _fit(lambda theta: logit_eval_host(vectors, other, u, v, y, op, theta, l2), np.asarray(vectors).shape[1], op, l2, max_iter, gtol)


def _label_matrix(Y, n):
    if hasattr(Y, "detach"):
        Y = Y.detach().cpu().numpy()
    Y = np.asarray(Y)
    if Y.ndim != 2 or Y.shape[0] != n or Y.dtype.kind not in "iub":
        raise ValueError(f"Y must be an integer [n, C] matrix of 0 / 1 with one row per sample ({n})")
    return Y


def fit_one_vs_rest(index, rows, Y, l2=1e-3, max_iter=200, gtol=1e-8):
    """Node classification: one ``fit`` with ``op="row"`` per column of the 0 / 1 label matrix ``Y`` ``[n, C]`` on the rows
    ``rows`` of the index, independently, in a loop.  Returns the list of the C models."""
    Y = _label_matrix(Y, len(rows))
    return [fit(index, rows, None, np.ascontiguousarray(Y[:, c]), "row", l2=l2, max_iter=max_iter, gtol=gtol) for c in range(Y.shape[1])]


def fit_one_vs_rest_host(vectors, rows, Y, l2=1e-3, max_iter=200, gtol=1e-8):
    """``fit_one_vs_rest`` by ``fit_host``."""
    Y = _label_matrix(Y, len(rows))
    return [fit_host(vectors, rows, None, np.ascontiguousarray(Y[:, c]), "row", l2=l2, max_iter=max_iter, gtol=gtol) for c in range(Y.shape[1])]
