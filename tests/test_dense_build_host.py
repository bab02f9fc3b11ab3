"""Host side of the device dense build: the row routine of pw_dense_noise_thresholds in its host instantiation
(pw_selftest_thresholds_row) against pw_noise_thresholds_dense and against NumPy's own expression, and the metadata checker
of from_dense_tensor / from_tensor.  All comparisons are bitwise."""
import ctypes as C
import warnings

import numpy as np
import pytest

from pecanpy_amd import _lib
from pecanpy_amd.engine import check_dense_matrix

LENGTHS = [0, 1, 7, 8, 9, 127, 128, 129, 1000, 8191, 8192, 8193, 20_000]
GAMMAS = [0.0, 0.5, 1.3]
KINDS = ["uniform", "ones", "magnitudes"]


def _row(kind, n):
    rs = np.random.RandomState(1000 + n)
    if kind == "uniform":
        return rs.random_sample(n) + 0.25
    if kind == "ones":
        return np.ones(n)
    return 10.0 ** rs.uniform(-8, 8, size=n)   # very different magnitudes: the order of the additions shows in the sum


def _row_threshold(w, gamma):
    out = C.c_float(0)
    w = np.ascontiguousarray(w, dtype=np.float64)
    assert _lib.load().pw_selftest_thresholds_row(w.ctypes.data, w.size, float(gamma), C.byref(out)) == 0
    return np.float32(out.value)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


_DENSE = {}


def _dense_thresholds(n, gamma):
    """pw_noise_thresholds_dense on a matrix whose rows 0..2 hold the three kinds of row with n non-zeros each (the other rows
    are empty); computed once per (n, gamma)."""
    if (n, gamma) not in _DENSE:
        size = max(n, 4)
        mat = np.zeros((size, size))
        for r, kind in enumerate(KINDS):
            mat[r, size - n:] = _row(kind, n)   # (zeros in front: the routine sees the non-zeros only)
        thr = np.zeros(size, dtype=np.float32)
        assert _lib.load().pw_noise_thresholds_dense(mat.ctypes.data, size, float(gamma), thr.ctypes.data) == 0
        _DENSE[(n, gamma)] = thr
    return _DENSE[(n, gamma)]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("gamma", GAMMAS)
def test_row_routine_equals_the_dense_host_thresholds(n, gamma):
    want = _dense_thresholds(n, gamma)
    for r, kind in enumerate(KINDS):
        got = _row_threshold(_row(kind, n), gamma)
        assert _bits(got) == _bits(want[r]), (kind, n, gamma, got, want[r])
    assert np.isnan(want[3])   # an empty row


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("gamma", GAMMAS)
def test_row_routine_equals_numpy(n, gamma):
    for kind in KINDS:
        w = _row(kind, n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # (mean of an empty slice)
            with np.errstate(all="ignore"):
                want = np.zeros(1, dtype=np.float32)
                want[0] = w.mean() + gamma * w.std()
                want = np.maximum(want, 0)
        got = _row_threshold(w, gamma)
        if n == 0:
            assert np.isnan(got) and np.isnan(want[0])
        else:
            assert _bits(got) == _bits(want[0]), (kind, n, gamma, got, want[0])


def test_row_routine_rejects_null_pointers():
    out = C.c_float(0)
    assert _lib.load().pw_selftest_thresholds_row(None, 3, 0.0, C.byref(out)) != 0
    assert _lib.load().pw_selftest_thresholds_row(None, 0, 0.0, C.byref(out)) == 0 and np.isnan(out.value)


# ---- the metadata checker ---------------------------------------------------------------------------------------------------
class _FakeDevice:
    def __init__(self, index):
        self.index = index


class _FakeCudaTensor:
    """What the checker looks at in a CUDA tensor, without a GPU: shape, dtype predicates, is_cuda, device.index."""
    is_cuda = True
    dtype = "torch.float64"

    def __init__(self, shape, index):
        self.shape = shape
        self.device = _FakeDevice(index)

    def is_floating_point(self):
        return True

    def is_complex(self):
        return False


@pytest.fixture
def no_library(monkeypatch):
    """The checker must not reach the library: loading it is an error while this fixture is active."""
    def boom():
        raise AssertionError("the metadata checker loaded the library")

    monkeypatch.setattr(_lib, "load", boom)


def test_checker_accepts_square_real_matrices(no_library):
    import torch

    assert check_dense_matrix(np.zeros((5, 5))) == 5
    assert check_dense_matrix(np.zeros((1, 1), dtype=np.float32)) == 1
    assert check_dense_matrix(np.zeros((3, 3), dtype=np.int16)) == 3
    assert check_dense_matrix(torch.zeros((4, 4), dtype=torch.float32)) == 4
    assert check_dense_matrix(torch.zeros((4, 4), dtype=torch.int64).t()) == 4
    assert check_dense_matrix(_FakeCudaTensor((6, 6), 2)) == 6
    assert check_dense_matrix(_FakeCudaTensor((6, 6), 2), device=2) == 6


@pytest.mark.parametrize("make", [
    lambda np_, torch: np_.zeros((3, 4)),
    lambda np_, torch: np_.zeros(9),
    lambda np_, torch: np_.zeros((3, 3, 3)),
    lambda np_, torch: np_.zeros((0, 0)),
    lambda np_, torch: np_.zeros((3, 3), dtype=np_.complex128),
    lambda np_, torch: np_.zeros((3, 3), dtype=bool),
    lambda np_, torch: torch.zeros((3, 4)),
    lambda np_, torch: torch.zeros(9),
    lambda np_, torch: torch.zeros((3, 3, 3)),
    lambda np_, torch: torch.zeros((3, 3), dtype=torch.complex64),
    lambda np_, torch: torch.zeros((3, 3), dtype=torch.bool),
    lambda np_, torch: [[0.0, 1.0], [1.0, 0.0]],
], ids=["np-nonsquare", "np-1d", "np-3d", "np-empty", "np-complex", "np-bool", "torch-nonsquare", "torch-1d", "torch-3d",
        "torch-complex", "torch-bool", "list"])
def test_checker_rejects_shape_and_dtype(make, no_library):
    import torch

    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.engine import WalkEngine
    from pecanpy_amd.experimental import Node2vecPlusPlus

    bad = make(np, torch)
    with pytest.raises(ValueError):
        check_dense_matrix(bad)
    with pytest.raises(ValueError):   # ... and the entries that use it raise before the library or a device is touched
        WalkEngine.from_dense_tensor(bad)
    for cls in (node2vec.DenseOTF, Node2vecPlusPlus):
        with pytest.raises(ValueError):
            cls.from_tensor(bad)


def test_checker_rejects_a_device_that_contradicts_the_tensor(no_library):
    from pecanpy_amd.engine import WalkEngine

    t = _FakeCudaTensor((6, 6), 1)
    with pytest.raises(ValueError, match="cuda:1"):
        check_dense_matrix(t, device=0)
    with pytest.raises(ValueError, match="cuda:1"):
        WalkEngine.from_dense_tensor(t, device=0)


def test_assigning_a_matrix_to_a_dense_object_still_works():
    """The lazy ``data`` / ``nonzero`` of the dense classes leave the reference's attribute behaviour alone."""
    from pecanpy_amd import pecanpy as node2vec

    g = node2vec.DenseOTF.from_mat(np.array([[0, 2], [2, 0]]), ["a", "b"])
    assert g.data.dtype == np.float64 and np.array_equal(g.data, [[0, 2], [2, 0]])
    assert np.array_equal(g.nonzero, [[False, True], [True, False]]) and g.num_edges == 2
    old, key = g.data, g._graph_key()   # (old stays referenced: ids are not reused)
    g.data = np.eye(2)
    assert old is not g.data and g._graph_key() != key and np.array_equal(g.nonzero, np.eye(2, dtype=bool))
    empty = node2vec.DenseOTF()
    assert empty.data is None and empty.nonzero is None
