"""The case list of the logistic-regression tests (tests/test_logit_host.py, tests/test_gpu_logit.py): matrices from a fixed
``default_rng``, every dim / m / label kind / theta kind / l2 / op / second-matrix choice of the issue, and the three ways to
answer a case -- ``statement`` (NumPy, pecanpy_amd.classify.logit_eval_host), ``selftest`` (the library's host build or its
kernels through pw_selftest_logit) -- with ``same_bits`` to compare them."""
import ctypes as C
import functools
import itertools

import numpy as np

from pecanpy_amd import _lib, classify

NA, NB = 300, 200
DIMS = (1, 3, 32, 33, 128, 130)
MS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
LABELS = ("zeros", "ones", "mixed")
THETAS = ("zero", "random", "scaled")
L2S = (0.0, 0.01)
OPS = classify.OPERATORS


@functools.lru_cache(maxsize=None)
def matrices(dim):
    rng = np.random.default_rng(1000 + dim)
    return rng.standard_normal((NA, dim)).astype(np.float32), rng.standard_normal((NB, dim)).astype(np.float32)


class Case:
    def __init__(self, dim, m, op, labels, theta_kind, l2, second):
        self.dim, self.m, self.op, self.labels, self.theta_kind, self.l2, self.second = dim, m, op, labels, theta_kind, l2, second
        self.id = f"d{dim}-m{m}-{op}-{labels}-{theta_kind}-l2_{l2}-{'AB' if second else 'AA'}"
        self.A, b = matrices(dim)
        self.B = b if second else None
        nb = NB if second else NA
        rng = np.random.default_rng([dim, m, OPS.index(op), int(second)])
        u = rng.integers(0, NA, m).astype(np.uint32)
        v = rng.integers(0, nb, m).astype(np.uint32)
        u[0], v[0] = NA - 1, nb - 1                      # the last row of each matrix
        if m >= 2:
            u[1] = v[1] = 5                              # u == v
        if m >= 4:
            u[3], v[3] = u[2], v[2]                      # a repeated pair
        self.u, self.v = u, v
        self.y = {"zeros": np.zeros(m, np.uint8), "ones": np.ones(m, np.uint8), "mixed": (rng.random(m) < 0.5).astype(np.uint8)}[labels]
        theta = np.zeros(dim + 1) if theta_kind == "zero" else rng.standard_normal(dim + 1)
        if theta_kind == "scaled":   # some |z| beyond 40 and beyond 708: the saturated branches, t = +0.0
            z = classify.logit_eval_host(self.A, self.B, u, v, None, op, theta, 0.0)
            theta = theta * (2000.0 / np.abs(z).max())
            z = classify.logit_eval_host(self.A, self.B, u, v, None, op, theta, 0.0)
            assert (np.abs(z) > 40).any() and (np.abs(z) > 708).any(), self.id
        self.theta = theta

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for i, (dim, m) in enumerate(itertools.product(DIMS, MS)):          # every (dim, m), the other choices cycling
        out.append(Case(dim, m, OPS[i % 5], LABELS[i % 3], THETAS[(i + i // 9) % 3], L2S[i % 2], bool((i // 2) % 2)))
    for op, theta_kind, second in itertools.product(OPS, THETAS, (False, True)):   # every (op, theta, second matrix)
        out.append(Case(33, 1025, op, "mixed", theta_kind, 0.01, second))
    for labels, l2 in itertools.product(LABELS, L2S):                    # every (labels, l2)
        out.append(Case(3, 2049, "hadamard", labels, "random", l2, False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def statement(case):
    """``(loss, grad, z)`` of the NumPy statement, computed once per case and shared: treat as read-only."""
    loss, grad, z = classify.logit_eval_host(case.A, case.B, case.u, case.v, case.y, case.op, case.theta, case.l2, return_z=True)
    grad.setflags(write=False)
    z.setflags(write=False)
    return loss, grad, z


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def selftest_raw(on_device, A, B, u, v, y, op_id, theta, l2, blocks=-1, want_z=True, dim=None):
    """pw_selftest_logit on host arrays: ``(rc, message, loss, grad, z)``, the outputs born as NaN."""
    lib = _lib.load()
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = None if B is None else np.ascontiguousarray(B, dtype=np.float32)
    dim = A.shape[1] if dim is None else dim
    u = np.ascontiguousarray(u, dtype=np.uint32)
    v = None if v is None else np.ascontiguousarray(v, dtype=np.uint32)
    y = None if y is None else np.ascontiguousarray(y, dtype=np.uint8)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    m = u.size
    loss, grad, z = C.c_double(float("nan")), np.full(dim + 1, np.nan), np.full(m, np.nan)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None   # noqa: E731
    rc = lib.pw_selftest_logit(int(on_device), 0, ptr(A), A.shape[0], ptr(B), 0 if B is None else B.shape[0], dim, ptr(u), ptr(v), ptr(y), m,
                               int(op_id), ptr(theta), float(l2), int(blocks), C.byref(loss), ptr(grad), ptr(z) if want_z else None)
    msg = lib.pw_last_error().decode() if rc else ""
    return rc, msg, loss.value, grad, z


def selftest(case, on_device, blocks=-1, with_y=True, want_z=True):
    rc, msg, loss, grad, z = selftest_raw(on_device, case.A, case.B, case.u, case.v, case.y if with_y else None, _lib.LOGIT_OPS[case.op],
                                          case.theta, case.l2, blocks, want_z)
    assert rc == 0, msg
    return loss, grad, z


def independent(A, B, u, v, y, op, theta, l2):
    """``(loss, grad)`` by a vectorised ``np.exp`` / ``np.log1p`` float64 expression that shares nothing with the definition
    but the model: the independent check of the gradient and the objective."""
    A = np.asarray(A)
    B = A if B is None else np.asarray(B)
    a = A[np.asarray(u)].astype(np.float64)
    b = a if op == "row" else B[np.asarray(v)].astype(np.float64)
    F = {"row": a, "average": (a + b) / 2, "hadamard": a * b, "l1": np.abs(a - b), "l2": (a - b) ** 2}[op]
    theta = np.asarray(theta, dtype=np.float64)
    w, bias = theta[:-1], theta[-1]
    z = F @ w + bias
    s = 2.0 * np.asarray(y, dtype=np.float64) - 1.0
    loss = np.mean(np.logaddexp(0.0, -s * z)) + 0.5 * l2 * float(w @ w)
    with np.errstate(over="ignore"):
        r = -s / (1.0 + np.exp(s * z))
    grad = np.concatenate([F.T @ r / len(z) + l2 * w, [r.mean()]])
    return float(loss), grad


@functools.lru_cache(maxsize=None)
def planted(m=2000, dim=16, seed=7):
    """The planted problem of the fit tests: labels from a noisy linear rule of Hadamard features."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((500, dim)).astype(np.float32)
    u, v = rng.integers(0, 500, m).astype(np.uint32), rng.integers(0, 500, m).astype(np.uint32)
    F = X[u].astype(np.float64) * X[v].astype(np.float64)
    w = rng.standard_normal(dim)
    y = ((F @ w + 0.3 + 0.5 * rng.standard_normal(m)) > 0).astype(np.uint8)
    return X, u, v, y
