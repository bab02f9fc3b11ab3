"""The dense classes' read_edg_device on the GPU: an edge-list file parsed in device memory, its CSR keeping the float64 weights
as parsed, and the dense handle built from them give, bit for bit, the matrix of the reference's ``to_dense()`` (the golden
vectors of tests/golden) and the handle ``pw_dense_create`` makes of that matrix on the host -- without an N x N host array.
Every comparison is bitwise."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

from pecanpy_amd import _lib, cli, graph
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.engine import WalkEngine
from pecanpy_amd.experimental import Node2vecPlusPlus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = ("indptr", "indices", "data", "adjbits", "deg")
SCALARS = ("unit", "dense_nonneg", "nnz", "words_per_row", "max_degree")


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return [dict(c, fixture=name.split(".")[0]) for c in json.load(f)]


DENSE_CASES = _load("edgelist_dense_cases.json")
ALL_CASES = _load("edgelist_cases.json") + _load("edgelist_device_cases.json") + DENSE_CASES
ERRORS = {"ValueError": ValueError, "IndexError": IndexError}


def _write(tmp_path, case):
    path = tmp_path / (case["name"] + ".edg")
    with open(path, "w", newline="") as f:
        f.write(case["text"])
    return str(path)


def scattered(a):
    """The matrix a dense handle's compressed rows (``dense_arrays()``) stand for."""
    n = a["deg"].size
    mat = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(a["indptr"].astype(np.int64)))
    mat[rows, a["indices"]] = a["data"]
    return mat


def host_handle(mat):
    """dense_arrays() of the handle pw_dense_create makes from `mat` on the host: the yardstick."""
    eng = WalkEngine.from_dense(mat)
    try:
        return eng.dense_arrays()
    finally:
        eng.close()


def assert_same_export(got, want):
    for k in SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def host_matrix(path, case):
    g = graph.DenseGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g.read_edg(path, case["weighted"], case["directed"], case["delimiter"])
    return g.data


# ---- golden cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=[c["fixture"] + "-" + c["name"] for c in ALL_CASES])
def test_golden_cases(tmp_path, case):
    path = _write(tmp_path, case)
    args = (path, case["weighted"], case["directed"], case["delimiter"])
    g = node2vec.DenseOTF()
    if case["error"]:
        with pytest.raises(ERRORS[case["error"]]):
            g.read_edg_device(*args)
        return
    sparse = node2vec.SparseOTF()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sparse.read_edg_device(*args)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        g.read_edg_device(*args)
    assert len(caught) == case["n_warnings"], [str(w.message) for w in caught]
    reader = g.last_build_stats["reader"]
    if case["n_warnings"]:
        assert reader == "host"
    assert reader == sparse.last_build_stats["reader"]      # the dense route declines nothing the sparse route takes
    assert list(g.nodes) == case["ids"]
    n = len(case["ids"])
    if "dense_bits" in case:
        want = np.array(case["dense_bits"], dtype=np.uint64).view(np.float64).reshape(n, n)
    else:
        want = host_matrix(path, case)
    if reader == "host":
        assert g.data.tobytes() == want.tobytes()
        return
    assert g._data is None and g._engine is not None
    a = g._engine.dense_arrays()
    assert scattered(a).tobytes() == want.tobytes()
    assert_same_export(a, host_handle(want))
    if n % 64:
        assert not np.any(a["adjbits"][:, -1] >> np.uint64(n % 64))
    st = g.last_build_stats
    assert st["matrix_host_bytes"] == 0 and st["n_nodes"] == n and st["nnz"] == int((want != 0).sum()) and st["unit"] == a["unit"]
    assert st["insertions"] == case["num_edges"] and st["file_bytes"] == len(case["text"])
    for k in ("upload_ms", "scan_ms", "ids_ms", "build_ms", "csr_kernels_ms", "dense_build_ms", "handle_ms"):
        assert st[k] >= 0, k
    assert st["dense_build_ms"] > 0


def test_the_cases_that_must_run_on_the_device_do(tmp_path):
    """Unit and non-unit handles from float64 values that float32 cannot tell apart; none of these files may decline."""
    want_unit = {"all_weights_1_00000001": False, "all_weights_exactly_one": True, "one_weight_not_one": False,
                 "float32_equal_float64_distinct": False, "same_pair_other_spelling": False, "one_vertex_self_loop": False,
                 "one_vertex_self_loop_unweighted": True, "ring_64": False, "ring_65": False, "ring_65_unweighted_directed": True,
                 "directed_sinks_first_seen_as_id2": False, "unweighted_undirected": True, "one_line_no_trailing_newline": False,
                 "no_trailing_newline_directed": False}
    by_name = {c["name"]: c for c in DENSE_CASES}
    for name, unit in want_unit.items():
        case = by_name[name]
        g = node2vec.DenseOTF()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            g.read_edg_device(_write(tmp_path, case), case["weighted"], case["directed"])
        assert g.last_build_stats["reader"] == "device", name
        a = g._engine.dense_arrays()
        assert a["unit"] is unit and g.last_build_stats["unit"] is unit, name
        if case["weighted"]:     # the float32 CSR of three cases is all ones: widened, two of them would wrongly be unit handles
            sparse = node2vec.SparseOTF()
            sparse.read_edg_device(_write(tmp_path, case), True, case["directed"])
            assert bool(np.all(sparse.data == 1.0)) == (name in ("all_weights_1_00000001", "all_weights_exactly_one", "one_weight_not_one"))


# ---- the float64 weights of the device CSR ---------------------------------------------------------------------------------------
def _read_c(path, weighted, directed, flags=None):
    lib = _lib.load()
    c, ids = C.c_void_p(), C.c_void_p()
    if flags is None:
        rc = lib.pw_edgelist_read_device(path.encode(), int(weighted), int(directed), b"\t", 0, C.byref(c), C.byref(ids), None)
    else:
        rc = lib.pw_edgelist_read_device_ex(path.encode(), int(weighted), int(directed), b"\t", 0, flags, C.byref(c), C.byref(ids), None)
    return rc, c, ids


def _nnz(c):
    shape = [C.c_uint64(0) for _ in range(4)]
    _lib.check(_lib.load().pw_csr_dev_shape(c, *[C.byref(s) for s in shape], None))
    return int(shape[1].value)


def test_float64_weights_are_kept_on_request_only(tmp_path):
    lib = _lib.load()
    case = next(c for c in DENSE_CASES if c["name"] == "float32_equal_float64_distinct")
    path = _write(tmp_path, case)
    n = len(case["ids"])
    want = np.array(case["dense_bits"], dtype=np.uint64).view(np.float64).reshape(n, n)
    sparse = node2vec.SparseOTF()
    sparse.read_edg_device(path, True, False)
    assert sparse.last_build_stats["reader"] == "device"

    rc, c, ids = _read_c(path, True, False)                  # the plain entry: no float64 weights, nothing to export
    assert rc == _lib.EDGELIST_OK
    try:
        nnz = _nnz(c)
        out = np.full(nnz, -1.0)
        assert lib.pw_csr_dev_export_f64(c, out.ctypes.data) == _lib.ERR_UNSUPPORTED and np.all(out == -1.0)
        plain32 = np.zeros(nnz, dtype=np.float32)
        _lib.check(lib.pw_csr_dev_export(c, None, None, plain32.ctypes.data))
    finally:
        lib.pw_csr_dev_destroy(c)
        lib.pw_edgelist_ids_destroy(ids)

    rc, c, ids = _read_c(path, True, False, _lib.EDGELIST_KEEP_F64)
    assert rc == _lib.EDGELIST_OK
    try:
        assert _nnz(c) == nnz == int((want != 0).sum())
        got64, got32 = np.zeros(nnz), np.zeros(nnz, dtype=np.float32)
        _lib.check(lib.pw_csr_dev_export_f64(c, got64.ctypes.data))
        _lib.check(lib.pw_csr_dev_export(c, None, None, got32.ctypes.data))
    finally:
        lib.pw_csr_dev_destroy(c)
        lib.pw_edgelist_ids_destroy(ids)
    assert got64.tobytes() == want[want != 0].tobytes()       # row-major non-zeros = CSR order: the winners as parsed
    assert {0.1, 0.10000000001} == set(got64.tolist())
    assert got32.tobytes() == plain32.tobytes() == sparse.data.tobytes() == got64.astype(np.float32).tobytes()

    rc, c, ids = _read_c(path, False, False, _lib.EDGELIST_KEEP_F64)     # unweighted: there are no weights to keep
    assert rc == _lib.EDGELIST_OK
    try:
        assert lib.pw_csr_dev_export_f64(c, out.ctypes.data) == _lib.ERR_UNSUPPORTED
    finally:
        lib.pw_csr_dev_destroy(c)
        lib.pw_edgelist_ids_destroy(ids)
    rc, c, ids = _read_c(path, True, False, 2)                           # an unknown flag bit
    assert rc == -1 and not c.value and not ids.value


# ---- files shared by the tests below: the 65-vertex golden graph and one larger file -----------------------------------------------
class _File:
    def __init__(self, path, directed):
        self.path, self.directed = path, directed
        host = node2vec.DenseOTF()
        host.read_edg(path, True, directed)
        self.nodes, self.data, self.nonzero = list(host.nodes), host.data, host.nonzero
        self.data.setflags(write=False)
        self.num_edges, self.density = host.num_edges, host.density


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """ring_65 of the fixture, and 300 vertices at density 0.3 (about 13 000 lines, 27 000 insertions: more than one 2 048-element
    block of the sort and more than one 4 096-element tile of the scans) with weights spelled in four ways."""
    tmp = tmp_path_factory.mktemp("dense_edg")
    ring = _write(tmp, next(c for c in DENSE_CASES if c["name"] == "ring_65"))
    rng = np.random.default_rng(300)
    n = 300
    lines = []
    for i in range(n):
        for j in range(i + 1, n):
            if rng.random() < 0.3:
                k, d = int(rng.integers(1, 100_000)), int(rng.integers(0, 7))
                text = (f"{k}e-{d}", repr(k / 10 ** d), f"+{k / 10 ** d:.6f}", f"{k}E-0{d}")[(i + j) % 4]
                lines.append(f"v{j}\tv{i}\t{text}" if (i * j) % 3 == 0 else f"v{i}\tv{j}\t{text}")
    assert 12_000 < len(lines) < 15_000
    big = tmp / "er300.edg"
    with open(big, "w") as f:
        f.write("\n".join(lines))       # (no trailing newline)
    return {"ring_65": _File(ring, False), "er_300": _File(str(big), False)}


def device_object(f, cls=node2vec.DenseOTF, **kw):
    g = cls(**kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g.read_edg_device(f.path, True, f.directed)
    assert g.last_build_stats["reader"] == "device"
    return g


def test_larger_file_equals_the_host_route(files):
    f = files["er_300"]
    assert len(f.nodes) == 300 and 0.25 < f.density < 0.35
    g = device_object(f)
    st = g.last_build_stats
    assert st["insertions"] > 2 * 4096 and st["nnz"] == f.num_edges and st["unit"] is False
    a = g._engine.dense_arrays()
    assert g._data is None and g.nodes == f.nodes
    assert scattered(a).tobytes() == f.data.tobytes()
    assert_same_export(a, host_handle(f.data))
    b = device_object(f)._engine.dense_arrays()      # a second run: the same words
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- walks and thresholds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring_65", "er_300"])
@pytest.mark.parametrize("cls,kw", [(node2vec.DenseOTF, dict(p=0.5, q=2)),
                                    (node2vec.DenseOTF, dict(p=0.5, q=2, extend=True, gamma=0)),
                                    (node2vec.DenseOTF, dict(p=0.5, q=2, extend=True, gamma=0.5)),
                                    (Node2vecPlusPlus, dict(p=0.5, q=2, gamma=0.5))],
                         ids=["node2vec", "node2vec_plus_g0", "node2vec_plus_g0.5", "node2vec_plusplus"])
def test_same_walks_and_thresholds_as_read_edg(files, name, cls, kw):
    f = files[name]
    a = device_object(f, cls=cls, random_state=7, **kw)
    eng = a._engine
    b = cls(random_state=7, **kw)
    b.read_edg(f.path, True, f.directed)
    wa, wb = a.simulate_walks(2, 8), b.simulate_walks(2, 8)
    assert a._engine is eng and a._data is None      # the handle of the read walked, and no matrix was made for it
    assert wa == wb and len(wa) == 2 * len(f.nodes)
    ta, tb = a.get_noise_thresholds(), b.get_noise_thresholds()
    assert ta.dtype == tb.dtype == np.float32 and not np.any(np.isnan(tb)) and ta.tobytes() == tb.tobytes()


# ---- no N x N host array -------------------------------------------------------------------------------------------------------------
def test_num_edges_density_and_walks_leave_the_matrix_on_the_device(files):
    f = files["er_300"]
    g = device_object(f, p=0.5, q=2, random_state=1)
    eng = g._engine
    assert g.num_edges == f.num_edges and type(g.num_edges) is type(f.num_edges)
    assert g.density == f.density
    assert len(g.simulate_walks(1, 4)) == 300
    assert g._data is None and g._nonzero is None and g.last_build_stats["matrix_host_bytes"] == 0
    assert g.data.tobytes() == f.data.tobytes() and g.nonzero.tobytes() == f.nonzero.tobytes()     # filled on first read
    assert g.num_edges == f.num_edges and g._engine is eng
    # the same object reads another file through the host reader: the matrix replaces the device-built graph
    conflict = next(c for c in DENSE_CASES if c["name"] == "same_pair_conflict")
    path = os.path.join(os.path.dirname(f.path), "conflict.edg")
    with open(path, "w") as out:
        out.write(conflict["text"])
    with pytest.warns(RuntimeWarning):
        g.read_edg_device(path, True, False)
    assert g.last_build_stats == {"reader": "host"} and g.nodes == conflict["ids"] and g.num_edges == 2
    assert len(g.simulate_walks(1, 3)) == 2


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_dense_walks_are_byte_identical_with_either_reader(files, tmp_path, monkeypatch, capsys):
    made = []
    materialize = node2vec._DenseBase._materialize

    def counting(self):
        if self._data is None and self._device_built is not None:
            made.append(1)
        return materialize(self)

    monkeypatch.setattr(node2vec._DenseBase, "_materialize", counting)
    common = ["--input", files["ring_65"].path, "--task", "walks", "--mode", "DenseOTF", "--weighted", "--p", "0.5", "--q", "2",
              "--num-walks", "2", "--walk-length", "12", "--random_state", "9", "--verbose"]
    monkeypatch.delenv("PECANPY_AMD_HOST_READER", raising=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cli.main(common + ["--output", str(tmp_path / "device.txt")])
        assert "edge list read by the device reader" in capsys.readouterr().out
        assert not made                                   # check_mode's density did not bring the matrix down
        monkeypatch.setenv("PECANPY_AMD_HOST_READER", "1")
        cli.main(common + ["--output", str(tmp_path / "host.txt")])
        assert "device reader" not in capsys.readouterr().out
    got, want = (tmp_path / "device.txt").read_bytes(), (tmp_path / "host.txt").read_bytes()
    assert got == want and got.count(b"\n") == 130
