"""Dense graph handles built on the device (pw_dense_create_device, pw_dense_create_from_csr, pw_dense_noise_thresholds):
array for array the handle pw_dense_create makes on one host thread, the host thresholds bit for bit, and the same walks.
Every comparison is bitwise."""
import glob
import os
import warnings

import numpy as np
import pytest
import torch

import edge_index_oracle as eo
from pecanpy_amd import _lib
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd._lib import PwError
from pecanpy_amd.engine import WalkEngine
from pecanpy_amd.experimental import Node2vecPlusPlus

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARRAYS = ("indptr", "indices", "data", "adjbits", "deg")
SCALARS = ("unit", "dense_nonneg", "nnz", "words_per_row", "max_degree")

_CACHE = {}


def cached(key, make):
    """A reference computed once per process; arrays are made read-only."""
    if key not in _CACHE:
        val = make()
        for a in (val.values() if isinstance(val, dict) else val if isinstance(val, tuple) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


def matrix(n, density, seed=0):
    """float64[n, n], not symmetric, non-zero with probability `density` (1.0: every entry, the diagonal included)."""
    def make():
        rng = np.random.default_rng(1000 * n + seed)
        w = rng.random((n, n)) * 4.0 + 0.001
        return np.where(rng.random((n, n)) < density, w, 0.0) if density < 1.0 else w
    return cached(("matrix", n, density, seed), make)


def host_export(mat, key=None):
    """dense_arrays() of the handle pw_dense_create makes from `mat` on the host: the yardstick."""
    def make():
        eng = WalkEngine.from_dense(mat)
        try:
            return eng.dense_arrays()
        finally:
            eng.close()
    return cached(("export", key), make) if key is not None else make()


def device_export(src, **kw):
    eng = WalkEngine.from_dense_tensor(src, **kw)
    try:
        return eng.dense_arrays(), eng.build_stats
    finally:
        eng.close()


def assert_same_export(got, want):
    for k in SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k   # (bytes: NaN payloads and signed zeros count)


def assert_same_thresholds(got, want):
    """Bit for bit, except that a NaN only has to be a NaN in the same place: the sign and payload of 0 / 0 are not defined
    by IEEE 754 and differ between the host's arithmetic and the device's."""
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert got[~nan].tobytes() == want[~nan].tobytes()


def assert_tail_bits_zero(exp, n):
    if n % 64:
        assert not np.any(exp["adjbits"][:, -1] >> np.uint64(n % 64))


# ---- export equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.25, 1.0])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 200, 3000])
def test_export_equals_the_host_built_handle(n, density):
    mat = matrix(n, density)
    want = host_export(mat, key=(n, density))
    got, st = device_export(torch.from_numpy(mat).cuda())
    assert_same_export(got, want)
    assert_tail_bits_zero(got, n)
    assert st["matrix_host_bytes"] == 0 and st["n_nodes"] == n and st["nnz"] == want["nnz"] and st["unit"] == want["unit"]
    assert st["build_ms"] > 0
    assert np.array_equal(got["deg"], (mat != 0).sum(axis=1))
    if density == 1.0:
        assert got["nnz"] == n * n and got["max_degree"] == n


def _special(name):
    n = 200
    m = matrix(n, 0.25, seed=7).copy()
    if name == "all-zero":
        m[:] = 0.0
    elif name == "zero-row":
        m[17, :] = 0.0
        m[199, :] = 0.0
    elif name == "full-row":
        m[0, :] = 2.5
        m[64, :] = 0.75
    elif name == "negative-zero":
        m[m == 0.0] = -0.0          # -0.0 is not an entry
        m[3, :] = -0.0
    elif name == "all-ones":
        m = (m != 0) * 1.0          # unit: the values are dropped
    elif name == "negative":
        m[5, 9] = -1.5
    elif name == "infinite":
        m[5, 9] = np.inf
    elif name == "nan":
        m[5, 9] = np.nan            # a NaN is a non-zero entry and clears dense_nonneg
        m[6, 199] = np.nan
    else:
        raise KeyError(name)
    return m


@pytest.mark.parametrize("name", ["all-zero", "zero-row", "full-row", "negative-zero", "all-ones", "negative", "infinite", "nan"])
def test_export_of_special_matrices(name):
    mat = _special(name)
    want = host_export(mat)
    got, st = device_export(torch.from_numpy(mat).cuda())
    assert_same_export(got, want)
    assert_tail_bits_zero(got, 200)
    assert st["matrix_host_bytes"] == 0
    assert got["unit"] == (name in ("all-zero", "all-ones"))
    assert got["dense_nonneg"] == (name not in ("negative", "infinite", "nan"))
    if name == "all-zero":
        assert got["nnz"] == 0 and got["max_degree"] == 0 and not got["adjbits"].any()
    if name == "all-ones":
        assert np.all(got["data"] == 1.0)
    if name == "negative-zero":
        assert got["deg"][3] == 0 and got["nnz"] == int((mat != 0).sum())
    # float32 source with the same special entries (all of them are float32 values or become one)
    m32 = mat.astype(np.float32)
    got32, _ = device_export(torch.from_numpy(m32).cuda())
    assert_same_export(got32, host_export(m32.astype(np.float64)))


@pytest.mark.parametrize("n", [129, 200])
def test_every_source_kind_gives_the_same_handle(n):
    mat = matrix(n, 0.25)
    want = host_export(mat, key=(n, 0.25))
    d64 = torch.from_numpy(mat).cuda()
    got, st = device_export(d64)
    assert_same_export(got, want)
    assert st["matrix_host_bytes"] == 0
    assert torch.equal(d64.cpu(), torch.from_numpy(mat))            # the source is only read
    # float32 on the device: widened inside the kernels, which is exact
    m32 = mat.astype(np.float32)
    got, st = device_export(torch.from_numpy(m32).cuda())
    assert_same_export(got, host_export(m32.astype(np.float64)))
    assert st["matrix_host_bytes"] == 0
    # a transposed view: made contiguous on the device, still without a host copy
    view = torch.from_numpy(np.ascontiguousarray(mat.T)).cuda().t()
    assert not view.is_contiguous()
    got, st = device_export(view)
    assert_same_export(got, want)
    assert st["matrix_host_bytes"] == 0
    # host input is uploaded and takes the same path, and says so
    got, st = device_export(torch.from_numpy(mat))
    assert_same_export(got, want)
    assert st["matrix_host_bytes"] == mat.nbytes
    got, st = device_export(mat, device=0)
    assert_same_export(got, want)
    assert st["matrix_host_bytes"] == mat.nbytes
    got, st = device_export(m32)
    assert_same_export(got, host_export(m32.astype(np.float64)))
    assert st["matrix_host_bytes"] == m32.nbytes
    # other real dtypes are converted to float64
    ints = (mat * 3).astype(np.int32)
    want_int = host_export(ints.astype(np.float64))
    assert_same_export(device_export(ints)[0], want_int)
    assert_same_export(device_export(torch.from_numpy(ints).cuda())[0], want_int)
    with pytest.raises(ValueError, match="cuda:0"):
        WalkEngine.from_dense_tensor(d64, device=1)


def test_c_abi_argument_checks():
    import ctypes as C

    lib = _lib.load()
    h = C.c_void_p()
    d = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    assert lib.pw_dense_create_device(0, C.c_void_p(d.data_ptr()), 0, 0, C.byref(h), None) == -1      # PW_ERR_INVALID: n_nodes == 0
    assert lib.pw_dense_create_device(0, None, 0, 2, C.byref(h), None) == -1
    assert lib.pw_dense_create_device(0, C.c_void_p(d.data_ptr()), 0, 2, C.byref(h), None) == 0      # build_ms is optional
    lib.pw_graph_destroy(h)


# ---- thresholds -------------------------------------------------------------------------------------------------------------------
THR_ROWS = [0, 1, 7, 8, 9, 127, 128, 129, 1000, 4096, 8191, 8192, 8193]


def test_thresholds_equal_the_host_thresholds():
    n = 8200
    gen = torch.Generator(device="cuda").manual_seed(5)
    d = torch.rand((n, n), generator=gen, device="cuda", dtype=torch.float64) * 3.0 + 0.01
    d *= torch.rand((n, n), generator=gen, device="cuda") < 0.25
    for r, k in enumerate(THR_ROWS):   # row r holds exactly k non-zeros, at random columns
        row = torch.zeros(n, dtype=torch.float64, device="cuda")
        cols = torch.randperm(n, generator=gen, device="cuda")[:k]
        row[cols] = torch.rand(k, generator=gen, device="cuda", dtype=torch.float64) * 100.0 + 1e-3
        d[r] = row
    eng = WalkEngine.from_dense_tensor(d)
    mat = d.cpu().numpy()
    assert [int(x) for x in (mat[:len(THR_ROWS)] != 0).sum(axis=1)] == THR_ROWS
    lib = _lib.load()
    try:
        for gamma in (0.0, 0.5):
            want = np.zeros(n, dtype=np.float32)
            assert lib.pw_noise_thresholds_dense(mat.ctypes.data, n, float(gamma), want.ctypes.data) == 0
            got = eng.compute_thresholds(gamma)
            assert_same_thresholds(got, want)
            assert np.isnan(got[0]) and got[1] == np.float32(mat[1][mat[1] != 0][0])
    finally:
        eng.close()


def test_thresholds_of_unit_csr_and_bits_handles():
    mat = _special("all-ones").copy()
    mat[11, :] = 0.0
    eng = WalkEngine.from_dense_tensor(torch.from_numpy(mat).cuda())
    assert eng.build_stats["unit"]
    for gamma in (0.0, 0.5):
        thr = eng.compute_thresholds(gamma)
        empty = ~(mat != 0).any(axis=1)
        assert empty[11] and np.all(np.isnan(thr[empty])) and np.all(thr[~empty] == 1.0)
    eng.close()
    csr = WalkEngine.from_csr(np.array([0, 1, 2], dtype=np.uint32), np.array([1, 0], dtype=np.uint32), None)
    with pytest.raises(PwError, match="error -4"):
        csr.compute_thresholds(0.0)
    with pytest.raises(PwError, match="error -4"):
        csr.dense_arrays()
    csr.close()
    from oracle import pyoracle as orc

    bits = WalkEngine.from_dense_bits(orc.pack_adjacency(mat != 0), 200)
    with pytest.raises(PwError, match="error -4"):
        bits.compute_thresholds(0.0)
    with pytest.raises(PwError, match="error -4"):
        bits.dense_arrays()
    part = bits.dense_arrays(rows=False)     # a handle made from packed bits has adjacency rows and degrees only
    assert np.array_equal(part["deg"], (mat != 0).sum(axis=1)) and "indices" not in part
    bits.close()


# ---- walks ------------------------------------------------------------------------------------------------------------------------
def _er_weighted(n=3000, density=0.25, seed=3):
    def make():
        rng = np.random.default_rng(seed)
        mask = np.triu(rng.random((n, n)) < density, 1)
        w = np.triu(rng.random((n, n)) * 0.999 + 0.001, 1)
        mat = np.where(mask, w, 0.0)
        mat = mat + mat.T
        mat[n // 2, :] = 0.0    # one isolated vertex
        mat[:, n // 2] = 0.0
        return mat
    return cached(("er", n, density, seed), make)


@pytest.mark.parametrize("cls,extend,gamma", [("DenseOTF", False, 0.0), ("DenseOTF", True, 0.0), ("DenseOTF", True, 0.5),
                                              ("Node2vecPlusPlus", False, 0.5)],
                         ids=["node2vec", "node2vec+g0", "node2vec+g0.5", "node2vec++"])
def test_walks_equal_from_mat(cls, extend, gamma):
    mat = _er_weighted()
    n = mat.shape[0]
    klass = node2vec.DenseOTF if cls == "DenseOTF" else Node2vecPlusPlus
    kw = dict(p=0.5, q=2, extend=extend, gamma=gamma, random_state=11)
    a = klass.from_tensor(torch.from_numpy(mat).cuda(), **kw)
    eng = a._engine
    b = klass.from_mat(mat, [str(i) for i in range(n)], **kw)
    b.device = 0
    wa = a.simulate_walks_array(4, 20)
    wb = b.simulate_walks_array(4, 20)
    assert wa.shape == (4 * n, 22) and np.array_equal(wa, wb)
    assert a._data is None and a._nonzero is None      # the host matrix was never materialised
    assert a._engine is eng                            # ... and the handle built from the tensor walked
    assert a.last_build_stats["matrix_host_bytes"] == 0 and a.nodes == b.nodes
    if extend or cls == "Node2vecPlusPlus":
        assert_same_thresholds(a.get_noise_thresholds(), b.get_noise_thresholds())
        assert a._data is None
    eng.close()
    b._engine.close()


def _dense_from_csr(z):
    n = z["indptr"].size - 1
    mat = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        sl = slice(z["indptr"][i], z["indptr"][i + 1])
        mat[i, z["indices"][sl]] = z["data"][sl]
    return mat


@pytest.mark.parametrize("path", sorted(f for f in glob.glob(os.path.join(GOLDEN, "*.npz")) if "_DenseOTF_" in os.path.basename(f)),
                         ids=lambda f: os.path.basename(f)[:-4])
def test_golden_dense_otf_from_a_tensor(path):
    """The reference-generated DenseOTF fixtures (loaded as tests/test_gpu_parity.py loads them), the handle built from a CUDA
    tensor and -- for the node2vec+ ones -- the thresholds computed on the device."""
    z = np.load(path)
    eng = WalkEngine.from_dense_tensor(torch.from_numpy(_dense_from_csr(z)).cuda())
    extend = bool(z["extend"])
    if extend:
        thr = eng.compute_thresholds(float(z["gamma"]))
        assert_same_thresholds(thr, z["thr"])
    got = eng.simulate("DenseOTF", float(z["p"]), float(z["q"]), extend, z["starts"], int(z["walk_length"]), seed=int(z["seed"]))
    assert np.array_equal(got, z["walks"])
    eng.close()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "n2vpp", "n2vpp_*.npz"))), ids=lambda f: os.path.basename(f)[:-4])
def test_golden_node2vec_plusplus_from_a_tensor(path):
    """The reference-generated node2vec++ fixtures (loaded as tests/test_gpu_n2vpp.py loads them) through from_tensor."""
    z = np.load(path)
    g = Node2vecPlusPlus.from_tensor(torch.from_numpy(z["data"]).cuda(), p=float(z["p"]), q=float(z["q"]), gamma=float(z["gamma"]),
                                     random_state=int(z["seed"]))
    mat = g.simulate_walks_array(int(z["num_walks"]), int(z["walk_length"]))
    assert np.array_equal(mat, z["walks"])
    assert g._data is None
    assert_same_thresholds(g.get_noise_thresholds(), z["thr"])
    g._engine.close()


# ---- lazy attributes ----------------------------------------------------------------------------------------------------------------
def test_data_and_nonzero_are_filled_on_first_read_and_keep_the_engine(tmp_path):
    mat = _er_weighted(n=700, seed=9)
    n = mat.shape[0]
    ids = [f"v{i}" for i in range(n)]
    kw = dict(p=0.5, q=2, extend=True, gamma=0.5, random_state=4)
    g = node2vec.DenseOTF.from_tensor(torch.from_numpy(mat).cuda(), node_ids=ids, **kw)
    eng = g._engine
    before = g.simulate_walks_array(2, 15)
    thr_device = g.get_noise_thresholds()
    assert g._data is None
    assert g.data.dtype == np.float64 and g.data.tobytes() == mat.tobytes()
    assert g.nonzero.dtype == bool and np.array_equal(g.nonzero, mat != 0)
    assert g._get_engine() is eng                      # reading the attributes did not replace the engine
    assert np.array_equal(g.simulate_walks_array(2, 15), before) and g._engine is eng
    assert_same_thresholds(thr_device, g.get_noise_thresholds())   # (now from the host matrix, as before this route existed)
    ref = node2vec.DenseOTF.from_mat(mat, ids, **kw)
    ref.device = 0
    assert np.array_equal(ref.simulate_walks_array(2, 15), before)
    assert g.num_edges == ref.num_edges and g.nodes == ids
    has = g.get_has_nbrs()
    assert has(0) and not has(n // 2)
    np.random.seed(3)
    nxt = g.get_move_forward()(0, None)
    np.random.seed(3)
    assert nxt == ref.get_move_forward()(0, None)
    fn, thr = g.setup_get_normalized_probs()
    fn_ref, thr_ref = ref.setup_get_normalized_probs()
    assert_same_thresholds(thr, thr_ref)
    assert fn(None, None, None, 0.5, 2, 0, 1).tobytes() == fn_ref(None, None, None, 0.5, 2, 0, 1).tobytes()
    g.save(str(tmp_path / "g.npz"))
    z = np.load(tmp_path / "g.npz")
    assert z["data"].tobytes() == mat.tobytes() and list(z["IDs"]) == ids
    emb = g.embed_array(dim=8, num_walks=1, walk_length=5, window_size=2, epochs=1, workers=1)
    assert emb.shape == (n, 8) and g._engine is eng
    with pytest.raises(ValueError, match="node_ids"):
        node2vec.DenseOTF.from_tensor(torch.from_numpy(mat).cuda(), node_ids=ids[:-1])
    eng.close()
    ref._engine.close()


# ---- edge list --------------------------------------------------------------------------------------------------------------------
def _hub_small():
    return eo.hub(n=6000, hub_degree=5000, background=4007)   # the hub graph at a size whose n x n float64 form is 288 MB


GRAPHS = {"small": eo.small_unweighted, "conflicts": eo.weighted_conflicts, "dropped": eo.dropped_rows, "hub": _hub_small,
          "sinks": eo.directed_sinks}


def _oracle(name, directed):
    def make():
        e, w, n = GRAPHS[name]()
        return eo.oracle_csr(e, w, n, directed)
    return cached(("oracle", name, directed), make)


def _matrix_of_csr(indptr, indices, data):
    """The dense float64 form of a float32 CSR: the weights widened."""
    n = indptr.size - 1
    mat = np.zeros((n, n))
    mat[np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))), indices] = data.astype(np.float64)
    return mat


@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_edge_list_export_equals_the_matrix_route(name, directed):
    e, w, n = GRAPHS[name]()
    indptr, indices, data, insertions, dropped = _oracle(name, directed)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        g = node2vec.DenseOTF.from_edge_index(torch.from_numpy(e).cuda(), None if w is None else torch.from_numpy(w).cuda(),
                                              num_nodes=n, directed=directed)
    mine = [r for r in rec if issubclass(r.category, RuntimeWarning) and "non-positive" in str(r.message)]
    assert len(mine) == (1 if dropped else 0)
    if dropped:
        assert str(mine[0].message) == f"{dropped} non-positive edge(s) ignored"
    st = g.last_build_stats
    assert st["edge_list_host_bytes"] == 0 and st["dropped"] == dropped and st["insertions"] == insertions
    assert st["n_nodes"] == n and st["nnz"] == indices.size and st["build_ms"] > 0
    assert g.num_nodes == n and g._data is None
    got = g._engine.dense_arrays()
    want, _ = device_export(_matrix_of_csr(indptr, indices, data), device=0)
    assert_same_export(got, want)
    assert np.array_equal(got["indptr"], indptr) and np.array_equal(got["indices"], indices)
    assert got["unit"] == (w is None or indices.size == 0)
    g._engine.close()


def test_edge_list_warning_and_stats_match_the_sparse_route():
    e, w, n = eo.dropped_rows()
    out = {}
    for cls in (node2vec.SparseOTF, node2vec.DenseOTF, Node2vecPlusPlus):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            g = cls.from_edge_index(e, w, num_nodes=n, p=1, q=1)
        out[cls.__name__] = ([str(r.message) for r in rec if "non-positive" in str(r.message)], g.last_build_stats)
        g._engine.close()
    msgs, st = out["SparseOTF"]
    assert msgs == ["4 non-positive edge(s) ignored"]
    for name in ("DenseOTF", "Node2vecPlusPlus"):
        assert out[name][0] == msgs
        assert set(st) <= set(out[name][1])                                   # the sparse route's keys, all of them
        for k in ("edge_list_host_bytes", "n_nodes", "nnz", "insertions", "dropped"):
            assert out[name][1][k] == st[k], k
    with pytest.raises(ValueError):
        node2vec.DenseOTF.from_edge_index(np.zeros((3, 4), dtype=np.int64))
    with pytest.raises(PwError, match="finite"):
        node2vec.DenseOTF.from_edge_index(e, np.full(e.shape[1], np.nan, dtype=np.float32), num_nodes=n)


def test_edge_list_hub_at_full_size_against_the_oracle_csr():
    """eo.hub() as it stands: 80 000 vertices, a row of 70 000 entries.  Its float64 matrix would take 51 GB, so the handle's
    arrays are compared with what the oracle CSR says they must be instead of with a matrix-built handle."""
    e, w, n = eo.hub()
    indptr, indices, data, insertions, dropped = cached(("oracle-hub-full",), lambda: eo.oracle_csr(e, w, n, False))
    eng = WalkEngine.dense_from_edge_index(torch.from_numpy(e).cuda(), torch.from_numpy(w).cuda(), num_nodes=n)
    got = eng.dense_arrays()
    eng.close()
    assert np.array_equal(got["indptr"], indptr) and np.array_equal(got["indices"], indices)
    assert got["data"].tobytes() == data.astype(np.float64).tobytes()
    deg = np.diff(indptr.astype(np.int64))
    assert np.array_equal(got["deg"], deg) and got["max_degree"] == deg.max() >= 70_000
    assert got["nnz"] == indices.size and not got["unit"] and got["dense_nonneg"] and got["words_per_row"] == 1250
    want_bits = np.zeros((n, 1250), dtype=np.uint64)
    rows = np.repeat(np.arange(n), deg)
    np.bitwise_or.at(want_bits, (rows, indices >> 6), np.uint64(1) << (indices & 63).astype(np.uint64))
    assert np.array_equal(got["adjbits"], want_bits)


def test_edge_list_walks_equal_from_mat():
    e, w, n = eo.small_unweighted()
    indptr, indices, data, _, _ = _oracle("small", False)
    kw = dict(p=0.5, q=2, random_state=7)
    a = node2vec.DenseOTF.from_edge_index(e, None, num_nodes=n, **kw)
    eng = a._engine
    b = node2vec.DenseOTF.from_mat(_matrix_of_csr(indptr, indices, data), [str(i) for i in range(n)], **kw)
    b.device = 0
    wa, wb = a.simulate_walks_array(4, 20), b.simulate_walks_array(4, 20)
    assert wa.shape == (4 * n, 22) and np.array_equal(wa, wb)
    assert a._engine is eng and a._data is None and a.nodes == b.nodes
    assert a.data.tobytes() == b.data.tobytes() and np.array_equal(a.nonzero, b.nonzero) and a._engine is eng
    eng.close()
    b._engine.close()
