"""The smallest inputs that reach what the creators and the two text readers share: the flags word of every dense route, the
id table at its minimum size with and without a repeated key, and a CSR creation refused half-way."""
import numpy as np
import pytest
import torch

from pecanpy_amd import graph
from pecanpy_amd.engine import PwError, WalkEngine

pytestmark = pytest.mark.gpu

SLACK = 32 << 20   # other work on the device may come and go (tests/test_gpu_memory_owners.py)


def _flags_word(eng):
    a = eng.dense_arrays(rows=False)
    return (1 if a["unit"] else 0) | (2 if a["dense_nonneg"] else 0)


def test_flags_word_of_every_dense_route(tmp_path):
    """n = 65: one full word and one partial word per row.  A handle from packed bits has no values: unit, and never
    dense_nonneg (word 1); the all-ones matrix gives 3 by the host, the tensor and the edge-list routes."""
    n = 65
    ones = np.ones((n, n))
    bits = np.zeros((n, 2), dtype=np.uint64)
    bits[:, 0], bits[:, 1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1)
    src, dst = np.divmod(np.arange(n * n, dtype=np.int64), n)
    path = tmp_path / "ones.edg"
    path.write_text("".join(f"{a}\t{b}\n" for a, b in zip(src.tolist(), dst.tolist()) if a <= b))
    routes = {
        "bits": (WalkEngine.from_dense_bits(bits, n), 1),
        "host": (WalkEngine.from_dense(ones), 3),
        "tensor": (WalkEngine.from_dense_tensor(torch.from_numpy(ones).cuda()), 3),
        "edge index": (WalkEngine.dense_from_edge_index(np.stack([src, dst]), None, num_nodes=n, directed=True), 3),
        "edge-list file": (WalkEngine.dense_from_edgelist_file(str(path), False, False), 3),
    }
    want = routes["host"][0].dense_arrays(rows=False)
    for name, (eng, word) in routes.items():
        assert eng is not None, name
        a = eng.dense_arrays(rows=False)
        assert _flags_word(eng) == word, name
        for key in ("indptr", "adjbits", "deg"):
            assert a[key].tobytes() == want[key].tobytes(), (name, key)
        assert (a["nnz"], a["max_degree"]) == (n * n, n), name
        eng.close()


@pytest.mark.parametrize("name,text", [("self loop", "a\ta\na\tb\nb\tc\n"), ("all distinct", "a\tb\nc\td\ne\tf\n")])
def test_small_edgelist_files_through_both_readers(name, text, tmp_path):
    """The id table at its minimum of 1024 slots, with a key repeated on one line and without any repeat: names as read_edg
    numbers them, arrays as the host route builds them."""
    path = str(tmp_path / "small.edg")
    with open(path, "w") as f:
        f.write(text)
    host = graph.SparseGraph()
    host.read_edg(path, False, False)
    eng = WalkEngine.from_edgelist_file(path, False, False)
    assert eng is not None and eng.ids == host.nodes
    indptr, indices, data = eng.csr
    assert indptr.tobytes() == np.asarray(host.indptr, dtype=np.uint32).tobytes()
    assert indices.tobytes() == np.asarray(host.indices, dtype=np.uint32).tobytes()
    assert np.array_equal(data, np.asarray(host.data, dtype=np.float32))
    eng.close()

    dense_host = graph.DenseGraph()
    dense_host.read_edg(path, False, False)
    want_eng = WalkEngine.from_dense(dense_host.data)
    eng = WalkEngine.dense_from_edgelist_file(path, False, False)
    assert eng is not None and eng.ids == dense_host.nodes
    got, want = eng.dense_arrays(), want_eng.dense_arrays()
    for key in ("indptr", "indices", "data", "adjbits", "deg"):
        assert got[key].tobytes() == want[key].tobytes(), key
    assert (got["unit"], got["dense_nonneg"], got["nnz"]) == (want["unit"], want["dense_nonneg"], want["nnz"])
    eng.close()
    want_eng.close()


def test_csr_creation_refused_half_way_releases_the_handle():
    """Unsorted column indices in a 4-vertex CSR: refused by the validation kernel, with the CSR on the device, the streams and
    events made and the helper threads started.  The refusals repeat and the next creation succeeds.  This is no leak
    coverage: twenty leaked handles of this size stay far below the slack that other work on the device imposes on the
    free-memory comparison, which here only catches a gross loss.  The guard that can see a leaked handle is
    tests/test_gpu_memory_owners.py::test_refused_csr_handles_release_what_they_allocated on R-MAT 17."""
    indptr = np.array([0, 2, 4, 6, 8], dtype=np.uint32)
    sorted_cols = np.array([1, 2, 0, 3, 0, 3, 1, 2], dtype=np.uint32)
    unsorted = sorted_cols.copy()
    unsorted[[0, 1]] = unsorted[[1, 0]]
    free = []
    for _ in range(20):
        with pytest.raises(PwError, match="strictly ascending"):
            WalkEngine.from_csr(indptr, unsorted, None)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[0] - free[-1] < SLACK, free
    eng = WalkEngine.from_csr(indptr, sorted_cols, None)
    assert eng.n_nodes == 4
    eng.close()
