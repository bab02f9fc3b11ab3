"""node2vec++ on CSR graphs without a GPU: the CSR restatement (tests/n2vpp_sparse_restated.py) against the dense one and
the reference's fixtures, the dense-formula thresholds of a CSR (pw_noise_thresholds_csr_f64), and the public surface of
pecanpy.experimental.SparseNode2vecPlusPlus."""
import glob
import os
import re

import numpy as np
import pytest

import n2vpp_restated as rs
import n2vpp_sparse_restated as srs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
SPARSE_FIXTURES = sorted(glob.glob(os.path.join(GOLD, "n2vpp_sparse", "n2vpp_sparse_*.npz")))


def _f32_exact(mat):
    return np.array_equal(mat.astype(np.float32).astype(np.float64), mat)


def f32_fixtures():
    """Every node2vec++ fixture whose matrix is float32-exact (the CSR contract's domain)."""
    out = []
    for f in sorted(glob.glob(os.path.join(GOLD, "n2vpp", "n2vpp_*.npz"))) + SPARSE_FIXTURES:
        if _f32_exact(np.load(f)["data"]):
            out.append(f)
    return out


def _random_graph(n, density, seed, *, unit=False, directed=False, loops=False, sink_frac=0.0):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < density
    if not directed:
        mask = np.triu(mask, 1)
        mask = mask | mask.T
    else:
        np.fill_diagonal(mask, False)
        mask[rng.random(n) < sink_frac, :] = False
    if loops:
        d = rng.random(n) < 0.3
        mask[d, d] = True
    w = rng.choice(np.array([0.125, 0.5, 1.0, 1.75, 3.0, 2.0 ** -60, 0.3]).astype(np.float32), size=(n, n)).astype(np.float64)
    if not directed:
        w = np.triu(w) + np.triu(w, 1).T
    return np.where(mask, 1.0 if unit else w, 0.0)


def test_fixtures_present():
    names = {os.path.basename(f)[:-4] for f in SPARSE_FIXTURES}
    assert {"n2vpp_sparse_tiny_p0.5_q2", "n2vpp_sparse_tiny_p0.5_q0.5", "n2vpp_sparse_dirloop_g0.0_p0.5_q2",
            "n2vpp_sparse_dirloop_g0.5_p0.7_q0.4"} <= names
    base = [os.path.basename(f)[:-4] for f in f32_fixtures()]
    assert len([b for b in base if not b.startswith("n2vpp_sparse_")]) == 9   # karate, sink, wdy, wre


def test_sparse_fixtures_reach_nan_and_hold_loops_and_sinks():
    def vectors(z):
        off = z["prob_off"]
        return [z["prob_vals"][off[i]:off[i + 1]] for i in range(off.size - 1)]

    z2 = np.load(os.path.join(GOLD, "n2vpp_sparse", "n2vpp_sparse_tiny_p0.5_q2.npz"))
    z05 = np.load(os.path.join(GOLD, "n2vpp_sparse", "n2vpp_sparse_tiny_p0.5_q0.5.npz"))
    assert any(np.isnan(v).all() for v in vectors(z2))
    assert any(np.isnan(v).any() for v in vectors(z05))
    zd = np.load(os.path.join(GOLD, "n2vpp_sparse", "n2vpp_sparse_dirloop_g0.0_p0.5_q2.npz"))
    m = zd["data"]
    assert (np.diag(m) != 0).any() and not np.array_equal(m, m.T) and (~(m != 0).any(axis=1)).any()
    assert (zd["walks"][:, -1] < zd["walk_length"] + 1).any()   # dead ends


@pytest.mark.parametrize("path", f32_fixtures(), ids=lambda f: os.path.basename(f)[:-4])
def test_restatement_reproduces_fixture(path):
    z = np.load(path)
    indptr, indices, data = srs.csr_of(z["data"])
    thr = srs.noise_thresholds(indptr, data, float(z["gamma"]))
    np.testing.assert_array_equal(thr.view(np.uint32), z["thr"].view(np.uint32))
    starts = rs.start_array(z["data"].shape[0], int(z["num_walks"]), int(z["seed"]))
    mat = srs.random_walks(indptr, indices, data, float(z["p"]), float(z["q"]), float(z["gamma"]), int(z["seed"]), starts,
                           int(z["walk_length"]))
    np.testing.assert_array_equal(mat, z["walks"])
    off = z["prob_off"]
    for i, (cur, prev) in enumerate(zip(z["prob_cur"], z["prob_prev"])):
        got = srs.normalized_probs(indptr, indices, data, float(z["p"]), float(z["q"]), int(cur),
                                   None if prev < 0 else int(prev), thr)
        np.testing.assert_array_equal(got.view(np.uint64), z["prob_vals"][off[i]:off[i + 1]].view(np.uint64))


@pytest.mark.parametrize("kind", ["weighted", "unit", "loops", "directed_sinks", "directed_loops_unit"])
@pytest.mark.parametrize("pq", [(0.5, 2.0), (0.7, 0.4), (1.0, 1.0)], ids=str)
def test_restatement_equals_dense_restatement(kind, pq):
    kw = dict(weighted={}, unit=dict(unit=True), loops=dict(loops=True), directed_sinks=dict(directed=True, sink_frac=0.2),
              directed_loops_unit=dict(directed=True, loops=True, unit=True, sink_frac=0.1))[kind]
    mat = _random_graph(40, 0.15, 3 + len(kind), **kw)
    p, q = pq
    for gamma in (0.0, 0.5):
        starts = rs.start_array(40, 2, 7)
        want = rs.random_walks(mat, p, q, gamma, 7, starts, 15)
        indptr, indices, data = srs.csr_of(mat)
        got = srs.random_walks(indptr, indices, data, p, q, gamma, 7, starts, 15)
        np.testing.assert_array_equal(got, want)


def _csr_rows(lengths, seed):
    """A CSR whose rows have the given lengths (weights float32, some rows with repeated values)."""
    rng = np.random.default_rng(seed)
    n = max(len(lengths), max(lengths) + 1)
    rows, data = [], []
    for i, d in enumerate(lengths):
        rows.append(np.sort(rng.choice(n, size=d, replace=False)))
        data.append(rng.choice(np.array([0.1, 0.7, 1.0, 3.3, 1e-3, 2.0 ** -60], np.float32), size=d) if i % 3 == 0
                    else (rng.random(d) * 7 + 1e-6).astype(np.float32))
    lengths = list(lengths) + [0] * (n - len(lengths))
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    indices = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.uint32)
    data = np.concatenate(data + [np.zeros(0, np.float32)]).astype(np.float32)
    return indptr, indices, data, n


@pytest.mark.parametrize("gamma", [0.0, 0.5, 0.1, 1.0])
def test_thresholds_csr_f64_equal_dense_formula(gamma):
    """pw_noise_thresholds_csr_f64 equals the dense formula on A.toarray().astype(f64), bit for bit, for rows of every
    length class of NumPy's reductions: empty, < 8, <= 128, pairwise above 128, more than one 8192-element buffer."""
    from pecanpy_amd import _lib

    lib = _lib.load()
    lengths = [0, 1, 2, 7, 8, 9, 16, 127, 128, 129, 300, 1000, 8191, 8192, 8193, 9000, 0, 3]
    indptr, indices, data, n = _csr_rows(lengths, 11)
    mat = np.zeros((n, n))
    for i in range(n):
        mat[i, indices[indptr[i]:indptr[i + 1]]] = data[indptr[i]:indptr[i + 1]]
    want = rs.noise_thresholds(mat, gamma)
    got = np.zeros(n, dtype=np.float32)
    _lib.check(lib.pw_noise_thresholds_csr_f64(indptr.ctypes.data, data.ctypes.data, n, gamma, got.ctypes.data))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(srs.noise_thresholds(indptr, data, gamma).view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[0]) and np.isnan(got[16])
    # unit weights: data = NULL
    got1 = np.zeros(n, dtype=np.float32)
    _lib.check(lib.pw_noise_thresholds_csr_f64(indptr.ctypes.data, None, n, gamma, got1.ctypes.data))
    np.testing.assert_array_equal(got1.view(np.uint32), rs.noise_thresholds((mat != 0) * 1.0, gamma).view(np.uint32))


def test_import_paths_and_surface():
    from pecanpy.experimental import SparseNode2vecPlusPlus
    from pecanpy_amd import experimental
    from pecanpy_amd._lib import MODE_IDS
    from pecanpy_amd.graph import SparseGraph
    from pecanpy_amd.pecanpy import Base, SparseOTF

    assert SparseNode2vecPlusPlus is experimental.SparseNode2vecPlusPlus
    assert issubclass(SparseNode2vecPlusPlus, Base) and issubclass(SparseNode2vecPlusPlus, SparseGraph)
    assert not issubclass(SparseNode2vecPlusPlus, SparseOTF)
    g = SparseNode2vecPlusPlus(p=0.5, q=2, gamma=0.5, random_state=3)
    assert g._mode == "SparseNode2vecPlusPlus" and g._always_thresholds
    hdr = open(os.path.join(REPO, "include", "pecanpy_amd.h")).read()
    enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"(PW_MODE_\w+)\s*=\s*(\d+)", hdr))
    assert enum["PW_MODE_SPARSE_NODE2VEC_PLUSPLUS"] == MODE_IDS["SparseNode2vecPlusPlus"] == 6
    assert sorted(enum.values()) == sorted(MODE_IDS.values())


def test_loaders_and_thresholds_without_gpu(tmp_path):
    from pecanpy.experimental import SparseNode2vecPlusPlus

    z = np.load(os.path.join(GOLD, "n2vpp_sparse", "n2vpp_sparse_dirloop_g0.5_p0.7_q0.4.npz"))
    ids = [str(i) for i in range(z["data"].shape[0])]
    g = SparseNode2vecPlusPlus.from_mat(z["data"], ids, p=0.7, q=0.4, gamma=0.5)
    assert g.num_nodes == z["data"].shape[0]
    np.testing.assert_array_equal(g.get_noise_thresholds().view(np.uint32), z["thr"].view(np.uint32))
    indptr, indices, data = srs.csr_of(z["data"])
    h = SparseNode2vecPlusPlus.from_csr(indptr, indices, data, gamma=0.5)
    np.testing.assert_array_equal(h.get_noise_thresholds().view(np.uint32), z["thr"].view(np.uint32))
    path = str(tmp_path / "g.npz")
    h.save(path)
    k = SparseNode2vecPlusPlus(gamma=0.5)
    k.read_npz(path, weighted=True)
    np.testing.assert_array_equal(k.get_noise_thresholds().view(np.uint32), z["thr"].view(np.uint32))


def test_numpy_fallback_thresholds(monkeypatch):
    """The NumPy loop used when the library is not built gives the same thresholds."""
    from pecanpy.experimental import SparseNode2vecPlusPlus
    from pecanpy_amd import _lib

    z = np.load(os.path.join(GOLD, "n2vpp_sparse", "n2vpp_sparse_dirloop_g0.5_p0.7_q0.4.npz"))
    g = SparseNode2vecPlusPlus.from_mat(z["data"], [str(i) for i in range(z["data"].shape[0])], gamma=0.5)

    def no_lib():
        raise _lib.PwError("not built")

    monkeypatch.setattr(_lib, "load", no_lib)
    np.testing.assert_array_equal(g.get_noise_thresholds().view(np.uint32), z["thr"].view(np.uint32))
