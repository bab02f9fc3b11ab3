"""node2vec++ (PW_MODE_NODE2VEC_PLUSPLUS, walk_dense_weighted_kernel's third bias form) on the GPU: bit-equal to the fixtures
generated from the reference's experimental.Node2vecPlusPlus, to the NumPy restatement (tests/n2vpp_restated.py) on larger
graphs, and to itself with every step decided by the reference's two loops (PECANPY_AMD_DENSE_EXACT_TEST=1)."""
import glob
import os

import numpy as np
import pytest

import n2vpp_restated as rs
from pecanpy_amd._lib import PwError
from pecanpy_amd.engine import WalkEngine

pytestmark = pytest.mark.gpu

MODE = "Node2vecPlusPlus"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "n2vpp", "n2vpp_*.npz")))
_ids = lambda f: os.path.basename(f)[:-4]  # noqa: E731


def _graph(z, **kw):
    from pecanpy.experimental import Node2vecPlusPlus

    args = dict(p=float(z["p"]), q=float(z["q"]), gamma=float(z["gamma"]), random_state=int(z["seed"]))
    args.update(kw)
    g = Node2vecPlusPlus.from_mat(z["data"], [str(i) for i in range(z["data"].shape[0])], **args)
    g.device = 0
    return g


def _simulate(eng, p, q, starts, L, seed, env=None, **kw):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return eng.simulate(MODE, p, q, False, starts, L, seed=seed, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_walks_equal_fixture(path):
    z = np.load(path)
    g = _graph(z)
    mat = g.simulate_walks_array(int(z["num_walks"]), int(z["walk_length"]))
    np.testing.assert_array_equal(mat, z["walks"])
    walks = g.simulate_walks(int(z["num_walks"]), int(z["walk_length"]))
    assert walks == [[str(v) for v in row[: row[-1]]] for row in z["walks"]]


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_extend_is_ignored(path):
    z = np.load(path)
    mat = _graph(z, extend=True).simulate_walks_array(int(z["num_walks"]), int(z["walk_length"]))
    np.testing.assert_array_equal(mat, z["walks"])


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_probs_equal_fixture(path):
    z = np.load(path)
    g = _graph(z)
    fn, thr = g.setup_get_normalized_probs()
    np.testing.assert_array_equal(thr.view(np.uint32), z["thr"].view(np.uint32))
    off = z["prob_off"]
    for i, (cur, prev) in enumerate(zip(z["prob_cur"], z["prob_prev"])):
        got = fn(g.data, g.nonzero, g.p, g.q, int(cur), None if prev < 0 else int(prev), thr)
        want = z["prob_vals"][off[i]:off[i + 1]]
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", ["n2vpp_tiny_p0.5_q2", "n2vpp_tiny_p0.5_q0.5", "n2vpp_wre_g0.5_p0.7_q0.4", "n2vpp_sink_p0.5_q2"])
def test_step_equals_restatement(name):
    z = np.load(os.path.join(REPO, "tests", "golden", "n2vpp", name + ".npz"))
    g = _graph(z)
    data, nonzero, thr = g.data, g.nonzero, z["thr"]
    p, q = float(z["p"]), float(z["q"])
    mf = g.get_move_forward()
    rng = np.random.default_rng(5)
    rows = np.nonzero(nonzero.any(axis=1))[0]
    eng = g._get_engine()
    for _ in range(60):
        cur = int(rng.choice(rows))
        nb = np.nonzero(nonzero[cur])[0]
        prev = None if rng.random() < 0.2 else int(rng.choice(nb)) if rng.random() < 0.8 else int(rng.integers(data.shape[0]))
        for r in (0.0, float(rng.random()), 1.0 - 2.0 ** -53):
            assert eng.step(MODE, p, q, False, cur, prev, r) == rs.step(data, nonzero, p, q, cur, prev, thr, r)
        np.random.seed(11)
        got = mf(cur, prev)
        np.random.seed(11)
        assert got == rs.step(data, nonzero, p, q, cur, prev, thr, np.random.random())


def _er(n, density, seed, weighted, isolated=True, directed=False, sink_frac=0.0):
    rng = np.random.default_rng(seed)
    if directed:
        mask = rng.random((n, n)) < density
        np.fill_diagonal(mask, False)
        mask[rng.random(n) < sink_frac, :] = False
    else:
        mask = np.triu(rng.random((n, n)) < density, 1)
        mask = mask | mask.T
    w = rng.random((n, n)) * 0.999 + 0.001
    if not directed:
        w = np.triu(w, 1) + np.triu(w, 1).T
    mat = np.where(mask, w if weighted else 1.0, 0.0)
    if isolated:
        mat[n // 2, :] = 0.0
        mat[:, n // 2] = 0.0
    return mat


@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unit"])
def test_er3000_bounded_equals_exact_and_restatement(weighted):
    n, L, seed = 3000, 20, 17
    mat = _er(n, 0.25, 3, weighted)
    eng = WalkEngine.from_dense(mat, device=0)
    starts = rs.start_array(n, 1, seed)
    try:
        for p, q, gamma in [(0.5, 2.0, 0.0), (1.5, 0.3, 0.5), (0.3, 1.0, 0.0), (1.0, 0.7, 1.0)]:
            thr = rs.noise_thresholds(mat, gamma)
            eng.set_thresholds(thr)
            fast = _simulate(eng, p, q, starts, L, seed)
            assert eng.last_stats["redo_walks"] == 0
            exact = _simulate(eng, p, q, starts, L, seed, env={"PECANPY_AMD_DENSE_EXACT_TEST": "1"})
            assert eng.last_stats["ambiguous_steps"] == eng.last_stats["total_steps"]
            np.testing.assert_array_equal(fast, exact)
            want = rs.random_walks(mat, p, q, gamma, seed, starts, L, n_jobs=300, thr=thr)
            np.testing.assert_array_equal(fast[:300], want)
    finally:
        eng.close()


def test_directed_weighted_with_sinks_and_stream_halves():
    n, L, seed = 600, 16, 23
    mat = _er(n, 0.05, 4, True, directed=True, sink_frac=0.3)
    thr = rs.noise_thresholds(mat, 0.5)
    eng = WalkEngine.from_dense(mat, device=0)
    try:
        eng.set_thresholds(thr)
        starts = rs.start_array(n, 2, seed)
        whole = _simulate(eng, 0.7, 0.4, starts, L, seed)
        assert eng.last_stats["dead_end_walks"] > 0
        np.testing.assert_array_equal(whole, rs.random_walks(mat, 0.7, 0.4, 0.5, seed, starts, L, thr=thr))
        h = starts.size // 2 + 7   # (dead ends: the second half starts where the first half's draws actually end)
        a = _simulate(eng, 0.7, 0.4, starts[:h], L, seed)
        b = _simulate(eng, 0.7, 0.4, starts[h:], L, seed, stream_skip=eng.last_stats["total_steps"])
        np.testing.assert_array_equal(np.concatenate([a, b]), whole)
    finally:
        eng.close()


@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unit"])
def test_stream_halves_concatenate(weighted):
    """One draw per step: a job array splits anywhere (the on-the-fly classification of the mode, not the alias one)."""
    n, L, seed = 500, 24, 29
    mat = _er(n, 0.1, 6, weighted)
    thr = rs.noise_thresholds(mat, 0.0)
    eng = WalkEngine.from_dense(mat, device=0)
    try:
        eng.set_thresholds(thr)
        starts = rs.start_array(n, 3, seed)
        whole = _simulate(eng, 0.5, 2.0, starts, L, seed)
        h = starts.size // 3 + 5
        a = _simulate(eng, 0.5, 2.0, starts[:h], L, seed)
        b = _simulate(eng, 0.5, 2.0, starts[h:], L, seed, stream_skip=eng.count_stream_draws(starts[:h], L))
        np.testing.assert_array_equal(np.concatenate([a, b]), whole)
        np.testing.assert_array_equal(whole[:200], rs.random_walks(mat, 0.5, 2.0, 0.0, seed, starts, L, n_jobs=200, thr=thr))
    finally:
        eng.close()


def test_unsupported_handles():
    mat = _er(80, 0.2, 5, True, isolated=False)
    thr = rs.noise_thresholds(mat, 0.0)
    starts = np.arange(80, dtype=np.uint32)
    eng = WalkEngine.from_dense(mat, device=0)
    try:
        with pytest.raises(PwError, match="thresholds"):
            eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
        with pytest.raises(PwError, match="thresholds"):
            eng.step(MODE, 1.0, 2.0, False, 0, None, 0.5)
    finally:
        eng.close()
    neg = mat.copy()
    neg[0, np.nonzero(neg[0])[0][0]] = -0.5
    eng = WalkEngine.from_dense(neg, device=0)
    try:
        eng.set_thresholds(rs.noise_thresholds(neg, 0.0))
        with pytest.raises(PwError, match="positive"):
            eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
        with pytest.raises(PwError, match="positive"):
            eng.probs(MODE, 1.0, 2.0, False, 1, 0)
    finally:
        eng.close()
    bits = np.packbits((mat != 0), axis=1, bitorder="little")
    bits = np.pad(bits, ((0, 0), (0, (-bits.shape[1]) % 8))).view(np.uint64)
    eng = WalkEngine.from_dense_bits(bits, 80, device=0)
    try:
        eng.set_thresholds(thr)
        with pytest.raises(PwError, match="packed bits"):
            eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
    finally:
        eng.close()
    idx = np.nonzero(mat)
    indptr = np.concatenate([[0], np.cumsum((mat != 0).sum(1))]).astype(np.uint32)
    eng = WalkEngine.from_csr(indptr, idx[1].astype(np.uint32), mat[idx].astype(np.float32), device=0)
    try:
        eng.set_thresholds(thr)
        with pytest.raises(PwError, match="dense graph handle"):
            eng.simulate(MODE, 1.0, 2.0, False, starts, 5, seed=0)
        with pytest.raises(PwError, match="dense graph handle"):
            eng.step(MODE, 1.0, 2.0, False, 0, None, 0.5)
    finally:
        eng.close()
