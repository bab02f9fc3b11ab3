"""Every exported entry that takes a device index answers a missing or out-of-range device the same way, in the place among its
checks where it always did: PW_ERR_NO_DEVICE with the one long sentence on a box without a GPU, PW_ERR_INVALID "device index
out of range" on a box with one -- and the process stays usable after each refusal."""
import ctypes as C

import numpy as np
import pytest

from pecanpy_amd import _lib

NO_DEVICE = b"no HIP device visible (libpecanpy_amd needs a GPU; there is no CPU fallback)"
ERR_INVALID, ERR_NO_DEVICE = -1, -3


def _p(a):
    return C.c_void_p(a.ctypes.data)


# host arrays that every call below may point at: never read as device memory, the device check comes first
INDPTR, INDICES = np.array([0, 1, 2], dtype=np.uint32), np.array([1, 0], dtype=np.uint32)
DENSE = np.array([[0.0, 1.0], [1.0, 0.0]])
BITS = np.array([2, 1], dtype=np.uint64)
WALKS = np.array([[0, 1, 2]], dtype=np.uint32)          # one walk of length 1: two cells and the length
VEC = np.zeros((2, 4), dtype=np.float32)
ID_CHARS, ID_OFF = np.frombuffer(b"ab", dtype=np.uint8).copy(), np.array([0, 1, 2], dtype=np.uint64)
CLS, R = np.array([0, 1, 2], dtype=np.uint8), np.array([0.5])
OUT = [np.zeros(64, dtype=np.uint32) for _ in range(5)]
X32 = np.array([1.0], dtype=np.float32)


def _entries(tmp_path):
    """(name, call(lib, device) -> rc) for every exported entry that takes a device index, with valid minimal arguments
    (pw_graph_replicate needs a source handle, so only the GPU test below can call it)."""
    edg, corpus = tmp_path / "g.edg", tmp_path / "c.txt"
    edg.write_bytes(b"a\tb\nb\tc\nc\ta\n")
    corpus.write_bytes(b"a b\nb a\n")
    out = str(tmp_path / "out.txt").encode()
    h, h2 = C.c_void_p(), C.c_void_p()
    sgns = (1, 1, 2, 4, 1, 1, 1, 0.025, 0.0001, 0.0, 1, 1)   # n_walks, walk_length, n_nodes, dim, window, negative, epochs, ...
    return [
        ("pw_warmup", lambda lib, d: lib.pw_warmup(d, None)),
        ("pw_csr_create", lambda lib, d: lib.pw_csr_create(_p(INDPTR), _p(INDICES), None, 2, 2, d, C.byref(h))),
        ("pw_dense_create", lambda lib, d: lib.pw_dense_create(_p(DENSE), 2, d, C.byref(h))),
        ("pw_dense_create_bits", lambda lib, d: lib.pw_dense_create_bits(_p(BITS), 2, 0, d, C.byref(h))),
        ("pw_dense_create_device", lambda lib, d: lib.pw_dense_create_device(d, _p(DENSE), 0, 2, C.byref(h), None)),
        ("pw_coo_to_csr_device", lambda lib, d: lib.pw_coo_to_csr_device(d, None, None, None, 0, 0, 0, C.byref(h))),
        ("pw_edgelist_read_device", lambda lib, d: lib.pw_edgelist_read_device(str(edg).encode(), 0, 0, b"\t", d, C.byref(h), C.byref(h2), None)),
        ("pw_edgelist_read_device_ex", lambda lib, d: lib.pw_edgelist_read_device_ex(str(edg).encode(), 0, 0, b"\t", d, 1, C.byref(h), C.byref(h2), None)),
        ("pw_corpus_read_device", lambda lib, d: lib.pw_corpus_read_device(str(corpus).encode(), d, C.byref(h), C.byref(h2), None)),
        ("pw_vectors_write_text_device", lambda lib, d: lib.pw_vectors_write_text_device(d, _p(VEC), 2, 4, _p(ID_CHARS), _p(ID_OFF), out, None)),
        ("pw_vectors_write_text", lambda lib, d: lib.pw_vectors_write_text(d, _p(VEC), 2, 4, _p(ID_CHARS), _p(ID_OFF), out, None)),
        ("pw_walks_write_text_device", lambda lib, d: lib.pw_walks_write_text_device(d, _p(WALKS), 1, 1, _p(ID_CHARS), _p(ID_OFF), 2, out, None)),
        ("pw_walks_write_text", lambda lib, d: lib.pw_walks_write_text(d, _p(WALKS), 1, 1, _p(ID_CHARS), _p(ID_OFF), 2, out, None)),
        ("pw_sgns_create_device", lambda lib, d: lib.pw_sgns_create_device(d, _p(WALKS), *sgns, 0, C.byref(h))),
        ("pw_sgns_train_device", lambda lib, d: lib.pw_sgns_train_device(d, _p(WALKS), *sgns, _p(VEC), None)),
        ("pw_sgns_train", lambda lib, d: lib.pw_sgns_train(d, _p(WALKS), *sgns, _p(VEC))),
        ("pw_selftest_format_f6", lambda lib, d: lib.pw_selftest_format_f6(1, d, _p(X32), 1, _p(OUT[0]), _p(OUT[1]))),
        ("pw_selftest_exclusive_scan", lambda lib, d: lib.pw_selftest_exclusive_scan(d, 32, _p(OUT[0]), 1, C.byref(C.c_uint64(0)))),
        ("pw_selftest_lane", lambda lib, d: lib.pw_selftest_lane(1, d, _p(CLS), 3, 0.5, 2.0, _p(R), 1, *(_p(a) for a in OUT))),
        ("pw_selftest_lane_floats", lambda lib, d: lib.pw_selftest_lane_floats(1, d, _p(CLS), 3, 0.5, 2.0, _p(R), 1, *(_p(a) for a in OUT[:3]))),
    ]


@pytest.mark.skipif(_lib.load().pw_device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_every_device_entry_reports_the_missing_device_with_one_sentence(tmp_path):
    lib = _lib.load()
    for name, call in _entries(tmp_path):
        assert call(lib, 0) == ERR_NO_DEVICE, name
        assert lib.pw_last_error() == NO_DEVICE, name


@pytest.mark.skipif(_lib.load().pw_device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_the_checks_in_front_of_the_device_check_still_come_first(tmp_path):
    lib = _lib.load()
    edg = tmp_path / "g.edg"
    edg.write_bytes(b"a\tb\n")
    c, ids = C.c_void_p(), C.c_void_p()
    # an unusable delimiter is the host reader's business, device or no device
    assert lib.pw_edgelist_read_device(str(edg).encode(), 0, 0, b"", 0, C.byref(c), C.byref(ids), None) == _lib.EDGELIST_NEEDS_HOST_READER
    # the names are checked before the device is looked at
    descending = np.array([0, 2, 1], dtype=np.uint64)
    rc = lib.pw_walks_write_text_device(0, _p(WALKS), 1, 1, _p(ID_CHARS), _p(descending), 2, str(tmp_path / "w.txt").encode(), None)
    assert rc == ERR_INVALID and b"id_offsets do not ascend" in lib.pw_last_error()
    assert not (tmp_path / "w.txt").exists()


@pytest.mark.gpu
def test_device_index_out_of_range_and_the_next_call_still_works(tmp_path):
    """device = pw_device_count() is refused by every entry with PW_ERR_INVALID, and after each refusal a valid call of one of
    the reader / builder paths succeeds in the same process."""
    from pecanpy_amd.corpus import read_walks_device
    from pecanpy_amd.engine import WalkEngine

    lib = _lib.load()
    edg, corpus = tmp_path / "ok.edg", tmp_path / "ok.txt"
    edg.write_bytes(b"a\tb\nb\tc\nc\ta\n")
    corpus.write_bytes(b"a b\nb a\n")

    def edgelist():
        eng = WalkEngine.from_edgelist_file(str(edg), False, False)
        assert eng is not None and eng.ids == ["a", "b", "c"]
        eng.close()

    def corpus_file():
        d_walks, names = read_walks_device(corpus)
        assert read_walks_device.last_stats["reader"] == "device" and names == ["a", "b"]
        assert d_walks.cpu().tolist() == [[0, 1, 2], [1, 0, 2]]

    def dense():
        eng = WalkEngine.from_dense(DENSE)
        assert eng.dense_arrays()["deg"].tolist() == [1, 1]
        eng.close()

    valid = [edgelist, corpus_file, dense]
    beyond = int(lib.pw_device_count())
    source = WalkEngine.from_csr(INDPTR, INDICES, None)   # a replica goes through the same check as a new handle
    replica = C.c_void_p()
    entries = _entries(tmp_path) + [("pw_graph_replicate", lambda lib, d: lib.pw_graph_replicate(source._h, d, C.byref(replica)))]
    for k, (name, call) in enumerate(entries):
        assert call(lib, beyond) == ERR_INVALID, name
        assert lib.pw_last_error() == b"device index out of range", name
        valid[k % 3]()
    assert not replica.value
    source.close()
