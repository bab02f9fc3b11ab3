"""node2vec++ on CSR handles (PW_MODE_SPARSE_NODE2VEC_PLUSPLUS, walk_sparse_pp_kernel) on the GPU: bit-equal to the fixtures
generated from the reference's experimental.Node2vecPlusPlus on the dense float64 form, to mode 5 on a dense handle of the same
matrix, to the CSR restatement (tests/n2vpp_sparse_restated.py) on graphs too large for a dense form, and to itself with every
step decided by the reference's two loops (PECANPY_AMD_DENSE_EXACT_TEST=1)."""
import os

import numpy as np
import pytest

import n2vpp_restated as rs
import n2vpp_sparse_restated as srs
from pecanpy_amd import synth
from pecanpy_amd._lib import PwError
from pecanpy_amd.engine import WalkEngine
from test_n2vpp_sparse_host import f32_fixtures

pytestmark = pytest.mark.gpu

MODE = "SparseNode2vecPlusPlus"
FIXTURES = f32_fixtures()
_ids = lambda f: os.path.basename(f)[:-4]  # noqa: E731


def _graph(z, **kw):
    from pecanpy.experimental import SparseNode2vecPlusPlus

    args = dict(p=float(z["p"]), q=float(z["q"]), gamma=float(z["gamma"]), random_state=int(z["seed"]))
    args.update(kw)
    g = SparseNode2vecPlusPlus.from_mat(z["data"], [str(i) for i in range(z["data"].shape[0])], **args)
    g.device = 0
    return g


def _simulate(eng, p, q, starts, L, seed, env=None, mode=MODE, **kw):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return eng.simulate(mode, p, q, False, starts, L, seed=seed, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _csr_engine(indptr, indices, data, gamma):
    eng = WalkEngine.from_csr(indptr, indices, data, device=0)
    thr = srs.noise_thresholds(np.asarray(indptr, np.int64), data, gamma)
    eng.set_thresholds(thr)
    return eng, thr


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_walks_equal_fixture(path):
    z = np.load(path)
    g = _graph(z)
    mat = g.simulate_walks_array(int(z["num_walks"]), int(z["walk_length"]))
    np.testing.assert_array_equal(mat, z["walks"])
    walks = g.simulate_walks(int(z["num_walks"]), int(z["walk_length"]))
    assert walks == [[str(v) for v in row[: row[-1]]] for row in z["walks"]]
    mat_ext = _graph(z, extend=True).simulate_walks_array(int(z["num_walks"]), int(z["walk_length"]))
    np.testing.assert_array_equal(mat_ext, z["walks"])


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_probs_and_steps_equal_fixture(path):
    z = np.load(path)
    g = _graph(z)
    fn, thr = g.setup_get_normalized_probs()
    np.testing.assert_array_equal(thr.view(np.uint32), z["thr"].view(np.uint32))
    off = z["prob_off"]
    for i, (cur, prev) in enumerate(zip(z["prob_cur"], z["prob_prev"])):
        got = fn(g.data, g.indices, g.indptr, g.p, g.q, int(cur), None if prev < 0 else int(prev))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got.view(np.uint64), z["prob_vals"][off[i]:off[i + 1]].view(np.uint64))
    indptr, indices, data = g.indptr, g.indices, g.data
    p, q = float(z["p"]), float(z["q"])
    mf = g.get_move_forward()
    eng = g._get_engine()
    rng = np.random.default_rng(5)
    rows = np.nonzero(np.diff(indptr.astype(np.int64)) > 0)[0]
    for _ in range(40):
        cur = int(rng.choice(rows))
        nb = indices[indptr[cur]:indptr[cur + 1]]
        prev = None if rng.random() < 0.2 else int(rng.choice(nb)) if rng.random() < 0.8 else int(rng.integers(g.num_nodes))
        for r in (0.0, float(rng.random()), 1.0 - 2.0 ** -53):
            assert eng.step(MODE, p, q, False, cur, prev, r) == srs.step(indptr, indices, data, p, q, cur, prev, thr, r)
        np.random.seed(11)
        got = mf(cur, prev)
        np.random.seed(11)
        assert got == srs.step(indptr, indices, data, p, q, cur, prev, thr, np.random.random())


def _hashed(indptr, indices, unit):
    if unit:
        return np.ones(indices.size, np.float32)
    return synth.hash_edge_weights(indptr, indices, 3)


def _graphs():
    return {
        "er2000": lambda: synth.gnm_csr(2000, 40000, seed=2),
        "holme_kim4000": lambda: synth.holme_kim_csr(4000, 6, seed=3),
        "rmat14": lambda: synth.rmat_csr(14, seed=4),
    }


@pytest.mark.parametrize("unit", [False, True], ids=["hashed", "unit"])
@pytest.mark.parametrize("name", list(_graphs()))
def test_sparse_handle_equals_dense_handle(name, unit):
    """Whole job arrays: mode 6 on the CSR handle == mode 5 on the dense float64 handle of the same matrix."""
    gen = _graphs()[name]()
    indptr, indices = gen[0], gen[1]
    data = _hashed(indptr, indices, unit)
    n = indptr.size - 1
    dense = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    dense[rows, indices] = data.astype(np.float64)
    ceng = WalkEngine.from_csr(indptr, indices, data, device=0)
    deng = WalkEngine.from_dense(dense, device=0)
    try:
        starts = rs.start_array(n, 2, 31)
        for gamma in (0.0, 0.5):
            thr = srs.noise_thresholds(indptr.astype(np.int64), data, gamma)
            np.testing.assert_array_equal(thr.view(np.uint32), rs.noise_thresholds(dense, gamma).view(np.uint32))
            ceng.set_thresholds(thr)
            deng.set_thresholds(thr)
            for p, q in ((0.5, 2.0), (0.7, 0.4), (1.0, 1.0)):
                got = _simulate(ceng, p, q, starts, 20, 31)
                want = _simulate(deng, p, q, starts, 20, 31, mode="Node2vecPlusPlus")
                np.testing.assert_array_equal(got, want)
    finally:
        ceng.close()
        deng.close()


def test_exact_mode_equals_fast_rmat16():
    indptr, indices, data = synth.rmat_csr(16, weighted=True)
    eng, thr = _csr_engine(indptr, indices, data, 0.0)
    try:
        starts = rs.start_array(indptr.size - 1, 1, 41)
        fast = _simulate(eng, 0.5, 2.0, starts, 30, 41)
        exact = _simulate(eng, 0.5, 2.0, starts, 30, 41, env={"PECANPY_AMD_DENSE_EXACT_TEST": "1"})
        assert eng.last_stats["ambiguous_steps"] == eng.last_stats["total_steps"]
        np.testing.assert_array_equal(fast, exact)
        half = _simulate(eng, 0.5, 2.0, starts, 30, 41, env={"PECANPY_AMD_DENSE_EXACT_TEST": "3"})
        np.testing.assert_array_equal(fast, half)
    finally:
        eng.close()


def test_rmat18_weighted_equals_restatement():
    indptr, indices, data = synth.rmat_csr(18, weighted=True)
    eng, thr = _csr_engine(indptr, indices, data, 0.5)
    try:
        starts = rs.start_array(indptr.size - 1, 1, 43)
        got = _simulate(eng, 0.5, 2.0, starts, 40, 43)
        want = srs.random_walks(indptr, indices, data, 0.5, 2.0, 0.5, 43, starts, 40, n_jobs=200, thr=thr)
        np.testing.assert_array_equal(got[:200], want)
    finally:
        eng.close()


def test_large_hub_equals_restatement():
    """One hub of 140 000 neighbours (more than 131 072: the block prefixes are grouped into super-blocks)."""
    indptr, indices, _ = synth.bipartite_hubs_csr(3, 150000, 140000, seed=5)
    deg = np.diff(indptr.astype(np.int64))
    assert deg.max() > 131072
    data = synth.hash_edge_weights(indptr, indices, 9)
    eng, thr = _csr_engine(indptr, indices, data, 0.0)
    try:
        n = indptr.size - 1
        starts = np.concatenate([np.arange(3, dtype=np.uint32), rs.start_array(n, 1, 47)[:300]])
        for p, q in ((0.5, 2.0), (2.0, 0.5)):
            got = _simulate(eng, p, q, starts, 12, 47)
            want = srs.random_walks(indptr, indices, data, p, q, 0.0, 47, starts, 12, n_jobs=120, thr=thr)
            np.testing.assert_array_equal(got[:120], want)
            exact = _simulate(eng, p, q, starts, 12, 47, env={"PECANPY_AMD_DENSE_EXACT_TEST": "1"})
            np.testing.assert_array_equal(got, exact)
            for cur in range(3):
                v = eng.probs(MODE, p, q, False, cur, int(indices[indptr[cur] + 7]))
                np.testing.assert_array_equal(
                    v.view(np.uint64), srs.normalized_probs(indptr, indices, data, p, q, cur, int(indices[indptr[cur] + 7]), thr).view(np.uint64))
    finally:
        eng.close()


@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed_sinks"])
def test_stream_halves(directed):
    rng = np.random.default_rng(8)
    n = 800
    mask = rng.random((n, n)) < 0.02
    if not directed:
        mask = np.triu(mask, 1)
        mask = mask | mask.T
    else:
        mask[rng.random(n) < 0.3, :] = False
    w = rng.choice(np.array([0.25, 0.5, 1.0, 3.0, 0.75], np.float32), size=(n, n))
    mat = np.where(mask, w.astype(np.float64), 0.0)
    indptr, indices, data = srs.csr_of(mat)
    eng, thr = _csr_engine(indptr, indices, data, 0.5)
    try:
        starts = rs.start_array(n, 3, 51)
        whole = _simulate(eng, 0.7, 0.4, starts, 16, 51)
        h = starts.size // 3 + 5
        a = _simulate(eng, 0.7, 0.4, starts[:h], 16, 51)
        skip = eng.last_stats["total_steps"] if directed else eng.count_stream_draws(starts[:h], 16)
        if directed:
            assert eng.last_stats["dead_end_walks"] > 0
        b = _simulate(eng, 0.7, 0.4, starts[h:], 16, 51, stream_skip=skip)
        np.testing.assert_array_equal(np.concatenate([a, b]), whole)
        np.testing.assert_array_equal(whole[:150], srs.random_walks(indptr, indices, data, 0.7, 0.4, 0.5, 51, starts, 16,
                                                                    n_jobs=150, thr=thr))
    finally:
        eng.close()


def test_error_cases():
    mat = np.where(np.random.default_rng(2).random((60, 60)) < 0.2, 1.5, 0.0)
    mat = np.triu(mat, 1) + np.triu(mat, 1).T
    indptr, indices, data = srs.csr_of(mat)
    starts = np.arange(60, dtype=np.uint32)
    eng = WalkEngine.from_csr(indptr, indices, data, device=0)
    try:
        with pytest.raises(PwError, match="thresholds"):
            eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
        with pytest.raises(PwError, match="thresholds"):
            eng.step(MODE, 1.0, 2.0, False, 0, None, 0.5)
        eng.set_thresholds(srs.noise_thresholds(indptr.astype(np.int64), data, 0.0))
        eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
        with pytest.raises(PwError, match="dense graph handle"):   # mode 5 on a CSR handle: unchanged
            eng.simulate("Node2vecPlusPlus", 1.0, 2.0, False, starts, 5, seed=0)
    finally:
        eng.close()
    zero = data.copy()
    zero[3] = 0.0
    eng = WalkEngine.from_csr(indptr, indices, zero, device=0)
    try:
        eng.set_thresholds(srs.noise_thresholds(indptr.astype(np.int64), zero, 0.0))
        with pytest.raises(PwError, match="positive"):
            eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
        with pytest.raises(PwError, match="positive"):
            eng.probs(MODE, 1.0, 2.0, False, 1, None)
    finally:
        eng.close()
    neg = data.copy()
    neg[3] = -0.5
    with pytest.raises(PwError):   # negative weights: no CSR handle is made at all
        WalkEngine.from_csr(indptr, indices, neg, device=0).close()
    eng = WalkEngine.from_dense(mat, device=0)
    try:
        eng.set_thresholds(rs.noise_thresholds(mat, 0.0))
        with pytest.raises(PwError, match="CSR graph handle"):
            eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
        with pytest.raises(PwError, match="CSR graph handle"):
            eng.step(MODE, 1.0, 2.0, False, 0, None, 0.5)
    finally:
        eng.close()
