"""Every device allocation of the host driver has one owner: a call that is refused after it has allocated, and a handle
that is created, used and closed, give back what they took.

Each test synchronises, repeats a call and compares the free device memory (``torch.cuda.mem_get_info()[0]``) behind the
first and behind the last repetition against a slack of 32 MiB, as ``test_graph_handle_releases_its_device_memory`` does.
A leak shows only if the lost bytes exceed the slack, so ``_repeat`` is told the smallest per-entry array the repeated call
allocates and asserts that it, times the repetitions behind the first reading, is at least twice the slack.  What this
cannot see: word-sized buffers (flags, counters, the probes' argument blocks) and per-vertex arrays of small graphs; a case
whose shape the arithmetic does not cover says so where it is written."""
import ctypes as C

import numpy as np
import pytest
import torch

from pecanpy_amd import _lib
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.corpus import save_walks_device
from pecanpy_amd.embed import save_word2vec_format_device
from pecanpy_amd.engine import MultiWalkEngine, PwError, WalkEngine
from pecanpy_amd.synth import rmat_csr

pytestmark = pytest.mark.gpu

SLACK = 32 << 20
REFUSALS = 20
ROUNDS = 4


def _repeat(call, reps, smallest_bytes):
    """`call(i)` reps times; the free memory behind call 0 and behind the last one differ by less than the slack.
    smallest_bytes: the smallest per-entry array one call allocates (None: the case is below what the slack can show)."""
    if smallest_bytes is not None:   # a leak of that array in each of the reps - 1 later calls is at least twice the slack
        assert smallest_bytes * (reps - 1) >= 2 * SLACK, (smallest_bytes, reps)
    free = []
    for i in range(reps):
        call(i)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[0] - free[-1] < SLACK, free


@pytest.fixture(scope="module")
def rmat17():
    """R-MAT 17, weighted: 1.94 M entries -- 7.4 MiB per uint32 / float32 array of entries, 19 x 7.4 = 141 MiB >= 64 MiB."""
    indptr, indices, data = rmat_csr(17, seed=2, weighted=True)
    return indptr, indices, data


@pytest.fixture(scope="module")
def rmat19():
    """R-MAT 19, unit weights: 7.9 M entries -- 30 MiB per uint32 array of entries, 3 x 30 = 90 MiB >= 64 MiB."""
    indptr, indices, _ = rmat_csr(19, seed=2)
    return indptr, indices


def _refused(make, match):
    def call(_):
        with pytest.raises(PwError, match=match):
            make()
    return call


def test_refused_csr_handles_release_what_they_allocated(rmat17):
    """pw_csr_create refuses after the CSR is on the device and the rows of its entries are computed (two arrays of
    nnz words, and the edge lines allocated beside them): a row out of order, a column index >= n_nodes, a negative weight."""
    indptr, indices, data = rmat17
    n, entry_bytes = indptr.size - 1, indices.nbytes
    row = int(np.flatnonzero(np.diff(indptr.astype(np.int64)) >= 2)[0])
    unsorted = indices.copy()
    k = int(indptr[row])
    unsorted[k], unsorted[k + 1] = indices[k + 1], indices[k]
    _repeat(_refused(lambda: WalkEngine.from_csr(indptr, unsorted, data), "strictly ascending"), REFUSALS, entry_bytes)
    oob = indices.copy()
    oob[indices.size // 2] = n
    _repeat(_refused(lambda: WalkEngine.from_csr(indptr, oob, data), "column index >= n_nodes"), REFUSALS, entry_bytes)
    neg = data.copy()
    neg[indices.size // 3] = -1.0
    _repeat(_refused(lambda: WalkEngine.from_csr(indptr, indices, neg), "finite and >= 0"), REFUSALS, entry_bytes)


def test_refused_edge_lists_release_their_scratch(rmat17):
    """pw_coo_to_csr_device refuses behind its validation kernel; a weighted list has its kept-edge ranks (m + 1 words)
    allocated by then: one NaN weight, one id >= n_nodes."""
    indptr, indices, data = rmat17
    n, m = indptr.size - 1, indices.size
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    ei = torch.from_numpy(np.stack([src, indices.astype(np.int64)])).cuda()
    w = torch.from_numpy(data).cuda()
    w_nan = w.clone()
    w_nan[m // 2] = float("nan")
    _repeat(_refused(lambda: WalkEngine.from_edge_index(ei, w_nan, num_nodes=n, directed=True), f"edge {m // 2}: edge weights must be finite"),
            REFUSALS, 4 * (m + 1))
    ei_bad = ei.clone()
    ei_bad[1, m // 3] = n
    _repeat(_refused(lambda: WalkEngine.from_edge_index(ei_bad, w, num_nodes=n, directed=True), f"edge {m // 3}: vertex id negative or >= n_nodes"),
            REFUSALS, 4 * (m + 1))


def test_refused_text_writers_release_their_buffers(tmp_path):
    """The walk writer refuses behind its count pass (row offsets: 8 bytes per row, 2^20 rows = 8 MiB; 19 x 8 = 152 MiB): one
    node index without a name, one row length beyond walk_length + 1.  The embedding writer cannot open its file: the
    host entry has uploaded the matrix by then (2^21 rows of one float32 = 8 MiB)."""
    L, rows = 4, 1 << 20
    names = [str(i) for i in range(50)]
    mat = np.zeros((rows, L + 2), dtype=np.int32)
    mat[:, L + 1] = L + 1
    bad_index, bad_length = mat.copy(), mat.copy()
    bad_index[6, 3] = 50
    bad_length[8, L + 1] = L + 2
    d_index, d_length = torch.from_numpy(bad_index).cuda(), torch.from_numpy(bad_length).cuda()
    out = tmp_path / "walks.txt"
    _repeat(_refused(lambda: save_walks_device(out, names, d_index), "node index 50 at position 3 of row 6 outside the 50 names"),
            REFUSALS, 8 * (rows + 1))
    _repeat(_refused(lambda: save_walks_device(out, names, d_length), r"row length 6 in row 8 exceeds walk_length \+ 1 = 5"),
            REFUSALS, 8 * (rows + 1))
    assert out.read_bytes() == b""
    lib = _lib.load()
    n_rows = 1 << 21
    vec = np.zeros((n_rows, 1), dtype=np.float32)
    offsets = np.zeros(n_rows + 1, dtype=np.uint64)                       # (names of no characters)
    path = str(tmp_path / "no_such_directory" / "x.emb").encode()
    _repeat(_refused(lambda: _lib.check(lib.pw_vectors_write_text(0, vec.ctypes.data_as(C.c_void_p), n_rows, 1, None,
                                                                  offsets.ctypes.data_as(C.c_void_p), path, None)),
                     "cannot open .*No such file or directory"), REFUSALS, vec.nbytes)
    d_vec = torch.from_numpy(vec[:4097]).cuda()                           # the device entry: refused before it allocates
    _repeat(_refused(lambda: save_word2vec_format_device(tmp_path / "no_such_directory" / "x.emb", names[:1] * 4097, d_vec),
                     "cannot open .*No such file or directory"), REFUSALS, None)


def test_weighted_lane_tables_go_with_their_handle(monkeypatch):
    """A weighted R-MAT 12 handle through the weighted lane form, node2vec and node2vec+, and a second (p, q) that rebuilds
    the per-(p, q) tables in place.  53 k entries: the handle's largest buffer, the edge lines, is 3.7 MiB -- four rounds of
    this graph stay below the slack whatever is lost, so this case pins the walks (bit for bit across the rounds) and that
    creating, rebuilding and closing run; the slack would show only a leak of a whole other handle."""
    indptr, indices, data = rmat_csr(12, seed=5, weighted=True)
    n = indptr.size - 1
    g = node2vec.SparseOTF.from_csr(indptr, indices, data, extend=True, gamma=0)
    with np.errstate(all="ignore"):
        thr = np.nan_to_num(g.get_noise_thresholds(), nan=0.0)
    starts = np.concatenate([np.arange(n, dtype=np.uint32)] * 10)
    monkeypatch.setenv("PECANPY_AMD_CHAIN_TAIL", "0")
    first = []

    def round_(i):
        eng = WalkEngine.from_csr(indptr, indices, data)
        eng.set_thresholds(thr)
        got = []
        for extend, p, q in ((False, 0.5, 2), (True, 0.5, 2), (True, 1.5, 0.3), (False, 0.3, 1.7)):
            got.append(eng.simulate("SparseOTF", p, q, extend, starts, 40, seed=2))
            assert eng.last_stats["lane_kernel"] == 3, eng.last_stats
        eng.close()
        first.extend(got if i == 0 else [])
        assert all(np.array_equal(a, b) for a, b in zip(got, first))

    _repeat(round_, ROUNDS, None)


def test_unit_handles_with_row_totals_and_alias_tables_go_with_their_handle(rmat19, monkeypatch):
    """A unit R-MAT 19 handle with p = 0.3, q = 1.7 (the FLOATS form's row totals: one float32 per edge line, 32 MiB) and an
    alias-mode handle on the same graph (first-order tables: one slot per entry -- alias_j, alias_q, the build's two work
    lists and the entries' rows are 30 MiB each, 3 x 30 = 90 MiB >= 64 MiB; alias_indptr, 8 bytes per vertex, is 4 MiB)."""
    indptr, indices = rmat19
    n = indptr.size - 1
    starts = np.arange(0, n, 64, dtype=np.uint32)
    monkeypatch.setenv("PECANPY_AMD_FORCE_TOT", "1")          # the totals are built whatever the size of the job array
    first = []

    def unit_round(i):
        eng = WalkEngine.from_csr(indptr, indices, None)
        got = eng.simulate("SparseOTF", 0.3, 1.7, False, starts, 20, seed=3)
        assert eng.last_stats["lane_kernel"] == 2 and eng.last_stats["param_index_ms"] > 0, eng.last_stats
        eng.close()
        first.extend([got] if i == 0 else [])
        assert np.array_equal(got, first[0])

    _repeat(unit_round, ROUNDS, indices.nbytes)
    st_alias = np.arange(0, n, 1024, dtype=np.uint32)      # (a seeded alias walk is one sequential stream: few walks)
    first_alias = []

    def alias_round(i):
        eng = WalkEngine.from_csr(indptr, indices, None)
        eng.precomp_build(1.0, 1.0, False, True)
        got = eng.simulate("PreCompFirstOrder", 1, 1, False, st_alias, 10, seed=4)
        eng.close()
        first_alias.extend([got] if i == 0 else [])
        assert np.array_equal(got, first_alias[0])

    _repeat(alias_round, ROUNDS, indices.nbytes)


def test_dense_handles_and_replicas_go_with_their_handle(rmat19):
    """Dense handles built on the device from a matrix and from a pw_csr_dev, exported and closed: 4096 vertices at density
    0.4, 6.7 M entries -- 25.6 MiB of column indices, 51 MiB of float64 values (3 x 25.6 = 77 MiB).  A replica on device 0
    of the R-MAT 19 handle (30 MiB per array of entries), walked and closed."""
    rng = np.random.default_rng(7)
    n = 4096
    mat = np.where(rng.random((n, n)) < 0.4, rng.random((n, n)) + 0.5, 0.0)
    d_mat = torch.from_numpy(mat).cuda()
    nnz = int(np.count_nonzero(mat))
    src, dst = np.nonzero(mat)
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64)).cuda()
    w = torch.from_numpy(mat[src, dst].astype(np.float32)).cuda()
    starts = np.arange(n, dtype=np.uint32)
    first = {}

    def dense_round(i):
        for name, make in (("matrix", lambda: WalkEngine.from_dense_tensor(d_mat)),
                           ("csr", lambda: WalkEngine.dense_from_edge_index(ei, w, num_nodes=n, directed=True))):
            eng = make()
            arrays = eng.dense_arrays()
            assert arrays["nnz"] == nnz and not arrays["unit"]
            got = eng.simulate("DenseOTF", 0.5, 2, False, starts, 10, seed=5)
            eng.close()
            assert np.array_equal(got, first.setdefault(name, got))

    _repeat(dense_round, ROUNDS, 4 * nnz)
    indptr, indices = rmat19
    eng = WalkEngine.from_csr(indptr, indices, None)
    st19 = np.arange(0, indptr.size - 1, 64, dtype=np.uint32)
    want = eng.simulate("SparseOTF", 0.5, 2, False, st19, 20, seed=6)

    def replica_round(_):
        multi = MultiWalkEngine.from_engine(eng, [0, 0])
        rep = multi.engines[1]
        assert np.array_equal(rep.simulate("SparseOTF", 0.5, 2, False, st19, 20, seed=6), want)
        rep.close()

    _repeat(replica_round, ROUNDS, indices.nbytes)
    eng.close()


def test_probes_and_text_writers_leave_nothing(tmp_path):
    """50 single-step probes on a CSR handle, a dense node2vec++ handle and a sparse node2vec++ handle, and both text writers on
    4097 rows, four rounds each.  A probe allocates three small blocks and the writers a few hundred KiB: all of it is below
    what the slack can show (no arithmetic) -- the rounds pin that the values do not change and that nothing fails."""
    indptr, indices, data = rmat_csr(10, seed=3, weighted=True)
    n = indptr.size - 1
    g = node2vec.SparseOTF.from_csr(indptr, indices, data, extend=True, gamma=0)
    with np.errstate(all="ignore"):
        thr = np.nan_to_num(g.get_noise_thresholds(), nan=0.0)
    csr = WalkEngine.from_csr(indptr, indices, data)
    csr.set_thresholds(thr)
    rng = np.random.default_rng(9)
    mat = np.where(rng.random((200, 200)) < 0.3, rng.random((200, 200)) + 0.5, 0.0)
    mat[np.arange(200), (np.arange(200) + 1) % 200] = 1.0                 # (every vertex has a neighbour)
    dense = WalkEngine.from_dense_tensor(torch.from_numpy(mat).cuda())
    dense.compute_thresholds(0.0)
    curs = [int(v) for v in np.flatnonzero(np.diff(indptr.astype(np.int64)) > 0)[:50]]
    first = {}

    def probe_round(_):
        got = [csr.probs("SparseOTF", 0.5, 2, False, v).tobytes() for v in curs]
        got += [csr.probs("SparseNode2vecPlusPlus", 0.5, 2, False, v).tobytes() for v in curs]
        got += [dense.probs("Node2vecPlusPlus", 0.5, 2, False, v % 200).tobytes() for v in curs]
        got += [csr.step("SparseOTF", 0.5, 2, False, v, r=0.25) for v in curs]
        assert got == first.setdefault("probes", got)

    _repeat(probe_round, ROUNDS, None)
    csr.close()
    dense.close()
    rows = 4097
    names = [f"node{i}" for i in range(rows)]
    d_vec = torch.from_numpy(np.random.default_rng(1).standard_normal((rows, 16)).astype(np.float32)).cuda()
    walks = np.zeros((rows, 12), dtype=np.int32)
    walks[:, :11] = np.random.default_rng(2).integers(0, rows, (rows, 11))
    walks[:, 11] = 11
    d_walks = torch.from_numpy(walks).cuda()

    def writer_round(_):
        save_word2vec_format_device(tmp_path / "x.emb", names, d_vec)
        save_walks_device(tmp_path / "x.walks", names, d_walks)
        got = ((tmp_path / "x.emb").read_bytes(), (tmp_path / "x.walks").read_bytes())
        assert got == first.setdefault("files", got)

    _repeat(writer_round, ROUNDS, None)
