"""from_edge_index without a GPU: the classmethod exists on every sparse class, its argument checks fire before the library
or a device is touched, and the host oracle the GPU tests compare with (tests/edge_index_oracle.py) is itself pinned to
``from_mat``."""
import numpy as np
import pytest
import torch

import edge_index_oracle as eo
from pecanpy_amd import experimental
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.engine import WalkEngine, check_edge_index
from pecanpy_amd.graph import SparseGraph

SPARSE_CLASSES = [node2vec.SparseOTF, node2vec.PreComp, node2vec.PreCompFirstOrder, node2vec.FirstOrderUnweighted,
                  experimental.SparseNode2vecPlusPlus]


@pytest.mark.parametrize("cls", SPARSE_CLASSES, ids=lambda c: c.__name__)
def test_every_sparse_class_has_from_edge_index(cls):
    assert callable(getattr(cls, "from_edge_index", None))
    assert callable(getattr(WalkEngine, "from_edge_index", None))


def _no_device(monkeypatch):
    """Any use of the library or of a device fails the test."""
    from pecanpy_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library / a device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "warmup_async", boom)
    monkeypatch.setattr(torch.Tensor, "to", boom)
    monkeypatch.setattr(torch.Tensor, "cuda", boom)


BAD = {
    "one row": (np.zeros((1, 4), dtype=np.int64), None, "shape"),
    "three rows": (torch.zeros((3, 4), dtype=torch.int64), None, "shape"),
    "transposed [m, 2]": (np.zeros((4, 2), dtype=np.int64), None, "shape"),
    "one-dimensional": (torch.zeros(4, dtype=torch.int64), None, "shape"),
    "float ids (numpy)": (np.zeros((2, 4), dtype=np.float32), None, "integers"),
    "float ids (torch)": (torch.zeros((2, 4), dtype=torch.float64), None, "integers"),
    "bool ids": (torch.zeros((2, 4), dtype=torch.bool), None, "integers"),
    "uint64 ids": (np.zeros((2, 4), dtype=np.uint64), None, "uint64"),
    "weight too short": (np.zeros((2, 4), dtype=np.int64), np.ones(3, dtype=np.float32), "one weight per edge"),
    "weight too long": (torch.zeros((2, 4), dtype=torch.int64), torch.ones(5), "one weight per edge"),
    "weight two-dimensional": (np.zeros((2, 4), dtype=np.int64), np.ones((4, 1), dtype=np.float32), "one weight per edge"),
    "integer weights": (np.zeros((2, 4), dtype=np.int64), np.ones(4, dtype=np.int64), "floats"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments_raise_value_error_without_a_device(name, monkeypatch):
    edge_index, weight, match = BAD[name]
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        node2vec.SparseOTF.from_edge_index(edge_index, weight, p=1, q=1)
    with pytest.raises(ValueError, match=match):
        WalkEngine.from_edge_index(edge_index, weight)


def test_num_nodes_is_checked_without_a_device(monkeypatch):
    _no_device(monkeypatch)
    e = np.zeros((2, 4), dtype=np.int64)
    for bad in (-1, 2.5, 0):
        with pytest.raises(ValueError, match="num_nodes"):
            node2vec.SparseOTF.from_edge_index(e, num_nodes=bad)
    assert check_edge_index(e, np.ones(4, dtype=np.float32), 7) == 4
    assert check_edge_index(torch.zeros((2, 0), dtype=torch.int32), None, 0) == 0


def test_oracle_agrees_with_from_mat():
    """The yardstick of the GPU tests: on a small dense matrix (asymmetric weights, a self loop, an empty row) the
    edge-by-edge oracle gives the CSR ``SparseGraph.from_mat`` gives."""
    rng = np.random.RandomState(2)
    n = 9
    mat = np.where(rng.rand(n, n) < 0.35, rng.randint(1, 64, size=(n, n)) / 8.0, 0.0)
    mat[4, :] = 0.0
    mat[:, 4] = 0.0
    mat[2, 2] = 1.25
    ids = [str(i) for i in range(n)]
    want = SparseGraph.from_mat(mat, ids)
    src, dst = np.nonzero(mat)
    order = rng.permutation(src.size)   # (edge order must not matter when no pair repeats)
    e = np.stack([src[order], dst[order]])
    indptr, indices, data, insertions, dropped = eo.oracle_csr(e, mat[src, dst][order].astype(np.float32), n, directed=True)
    assert np.array_equal(indptr, want.indptr) and np.array_equal(indices, want.indices) and np.array_equal(data, want.data)
    assert indptr.dtype == np.uint32 and indices.dtype == np.uint32 and data.dtype == np.float32
    assert insertions == src.size and dropped == 0 and indptr[4] == indptr[5]
    # undirected: the symmetrised matrix, the later of the two orientations winning
    sym = np.triu(mat) + np.triu(mat, 1).T
    src, dst = np.nonzero(np.triu(mat))
    indptr, indices, data, insertions, _ = eo.oracle_csr(np.stack([src, dst]), mat[src, dst].astype(np.float32), n, directed=False)
    want = SparseGraph.from_mat(sym, ids)
    assert np.array_equal(indptr, want.indptr) and np.array_equal(indices, want.indices) and np.array_equal(data, want.data)
    assert insertions == 2 * src.size


def test_oracle_keeps_the_last_insertion_and_counts_drops():
    e = np.array([[0, 1, 2, 1], [1, 0, 2, 2]])
    w = np.array([1.0, 2.0, 3.0, -1.0], dtype=np.float32)
    indptr, indices, data, insertions, dropped = eo.oracle_csr(e, w, 4, directed=False)
    assert indptr.tolist() == [0, 1, 2, 3, 3] and indices.tolist() == [1, 0, 2] and data.tolist() == [2.0, 2.0, 3.0]
    assert insertions == 6 and dropped == 1
