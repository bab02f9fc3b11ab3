"""Every weighted walk path on weights whose dynamic range is that of the number format (``wide_weight_cases.py``), bit for bit
against the CPU oracle: the wave scan, the weighted lane form and its normaliser tables, ``pw_probs``, the alias builds and
walks, and the bounded dense kernel.  ``test_wide_weights_host.py`` shows on the CPU that these inputs do what they claim in the
oracle itself (binades crossed, elements absorbed, subnormal quotients, reads at ``choice == degree``, totals of +inf), so that
equality here is not equality of easy rows.

Every walk prints its counters (``pytest -s``): the share of steps a fast form left to the exact path is recorded in
MEASUREMENTS.md from there."""
import numpy as np
import pytest

import wide_weight_cases as wc
from oracle import pyoracle as orc
from pecanpy_amd.engine import WalkEngine

pytestmark = pytest.mark.gpu

NO_WLANES = (("PECANPY_AMD_NO_WLANES", "1"),)
WL_ENV = (("PECANPY_AMD_FORCE_TOT", "1"), ("PECANPY_AMD_CHAIN_TAIL", "0"))      # as table_history_cases.WL_ENV
WAYS = (("default", ()), ("wave", NO_WLANES), ("wlane", WL_ENV))


def _diff_report(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    j = int(np.flatnonzero(got[i] != want[i])[0])
    return (f"{bad.size}/{got.shape[0]} rows differ; first row {i} at column {j}: got {got[i, max(0, j - 2): j + 2].tolist()} "
            f"want {want[i, max(0, j - 2): j + 2].tolist()} (start {int(want[i, 0])}, length cell {int(got[i, -1])}/{int(want[i, -1])})")


def _in_lane_range(c):
    return all(1.0 / 1024 <= x <= 1024 for x in (c.p, c.q))


def _walk(eng, c, env, mp):
    with mp.context() as m:
        for k, v in env:
            m.setenv(k, v)
        got = eng.simulate("SparseOTF", c.p, c.q, c.ext is not None, wc.starts(c.graph), wc.L, seed=wc.SEED)
        return got, dict(eng.last_stats)


def _check_stats(st, c, want, ov, steps, what):
    """Steps, reads at ``choice == degree`` and dead ends (walks that moved and stopped before L steps) are those of the
    oracle's matrix."""
    assert (st["total_steps"], st["overflow_reads"], st["dead_end_walks"]) == (steps, ov, wc.dead_ends(want)), (what, st)


@pytest.mark.parametrize("c", wc.SPARSE_CASES, ids=wc.case_id)
def test_sparse_otf_equals_the_oracle_three_ways(c, monkeypatch):
    """The default path, the wave scan alone and the forced weighted lane form (normaliser tables built): the oracle's walk
    matrix and its step, overflow-read and dead-end counts."""
    indptr, indices, data = wc.graph(c.graph, c.family)
    want, ov, clamped, steps = wc.oracle_sparse(c)
    assert clamped == 0
    eng = WalkEngine.from_csr(indptr, indices, data)
    if c.ext is not None:
        eng.set_thresholds(wc.case_thr(c))
    for name, env in WAYS:
        got, st = _walk(eng, c, env, monkeypatch)
        print(wc.case_id(c), name, {k: st[k] for k in ("lane_kernel", "total_steps", "overflow_reads", "eager_steps", "redo_walks", "repair_rounds")})
        assert np.array_equal(got, want), (wc.case_id(c), name, _diff_report(got, want))
        _check_stats(st, c, want, ov, steps, (wc.case_id(c), name))
        if name == "wlane" and _in_lane_range(c):
            assert st["lane_kernel"] == 3, (wc.case_id(c), st)
    eng.close()


@pytest.mark.parametrize("family", ["loguniform", "stair_down", "stair_up"])
def test_verify_switch_leaves_the_weighted_form_alone(family, monkeypatch):
    """``PECANPY_AMD_VERIFY_TIGHT=1`` records the interval decisions of the unit-weight forms only: on a weighted graph the
    call must stay on the weighted lane form, record nothing (``verify_checked == 0``) and walk as without the switch.  (No
    device-side check of the weighted form's decisions exists; they are held to the oracle by the walks above.)"""
    c = wc.Case("rmat9", family, 0.5, 2.0, None)
    indptr, indices, data = wc.graph(c.graph, c.family)
    want = wc.oracle_sparse(c)[0]
    eng = WalkEngine.from_csr(indptr, indices, data)
    got, st = _walk(eng, c, WL_ENV + (("PECANPY_AMD_VERIFY_TIGHT", "1"),), monkeypatch)
    assert np.array_equal(got, want), _diff_report(got, want)
    assert st["lane_kernel"] == 3 and (st["verify_checked"], st["verify_mismatch"], st["verify_dropped"]) == (0, 0, 0), st
    eng.close()


@pytest.mark.parametrize("family", wc.FAMILIES)
@pytest.mark.parametrize("ext", [None, "g0", "hand"])
def test_probability_vectors_bitwise(family, ext):
    """``pw_probs`` against ``orc.sparse_probs`` as uint32 patterns (NaN patterns too) for 60 real (prev, cur) entries and the
    first step, as ``test_gpu_probe.py`` does on (0, 1] weights."""
    indptr, indices, data = wc.graph("rmat9", family)
    thr = None if ext is None else wc.thresholds("rmat9", family, ext)
    eng = WalkEngine.from_csr(indptr, indices, data)
    if thr is not None:
        eng.set_thresholds(thr)
    rng = np.random.default_rng(3)
    deg = np.diff(indptr.astype(np.int64))
    for p, q in wc.PQ[:2] + (() if wc.element_overflows(family, *wc.PQ[2]) else wc.PQ[2:]):
        for prev in rng.choice(np.nonzero(deg)[0], 60):
            cur = int(indices[indptr[prev] + rng.integers(0, deg[prev])])
            with np.errstate(all="ignore"):
                want = orc.sparse_probs(indptr, indices, data, p, q, cur, int(prev), thr=thr)
                want0 = orc.sparse_probs(indptr, indices, data, p, q, cur, None, thr=thr)
            got = eng.probs("SparseOTF", p, q, ext is not None, cur, int(prev))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (family, ext, p, q, cur, int(prev))
            first = eng.probs("SparseOTF", p, q, ext is not None, cur)
            assert np.array_equal(first.view(np.uint32), want0.view(np.uint32)), (family, ext, p, q, cur)
    eng.close()


def _tables_equal(got, want, what):
    for g, w, part in zip(got, want, ("alias_indptr", "alias_j", "alias_q")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, part, g.shape, w.shape)
        if part == "alias_q":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, part, f"{float((g != w).mean()):.4f} of the words differ")


@pytest.mark.parametrize("name", ["rmat9", "star"])
@pytest.mark.parametrize("family", ["moderate", "loguniform", "spike"])
@pytest.mark.parametrize("extend", [False, True])
def test_alias_tables_and_walks(name, family, extend):
    """``precomp_export`` against ``orc.precomp_tables`` / ``orc.first_order_tables`` bit for bit; PreComp, PreCompFirstOrder and
    FirstOrderUnweighted walks against the oracle."""
    indptr, indices, data = wc.graph(name, family)
    thr = wc.thresholds(name, family, "g0") if extend else None
    starts = wc.starts(name)
    eng = WalkEngine.from_csr(indptr, indices, data)
    if extend:
        eng.set_thresholds(thr)
    p, q = 0.5, 2.0
    tables = orc.precomp_tables(indptr, indices, data, p, q, thr=thr)
    want = orc.walks_precomp(indptr, indices, data, p, q, starts, wc.L, wc.SEED, thr=thr, tables=tables)
    got = eng.simulate("PreComp", p, q, extend, starts, wc.L, seed=wc.SEED)
    _tables_equal(eng.precomp_export(False), tables, (name, family, extend, "PreComp"))
    assert np.array_equal(got, want), ("PreComp", _diff_report(got, want))
    if not extend:
        want = orc.walks_first_order(indptr, indices, data, starts, wc.L, wc.SEED, precomp=True)
        got = eng.simulate("PreCompFirstOrder", 1, 1, False, starts, wc.L, seed=wc.SEED)
        aj, aq = orc.first_order_tables(indptr, data)
        _tables_equal(eng.precomp_export(True), (indptr.astype(np.uint64), aj, aq), (name, family, "PreCompFirstOrder"))
        assert np.array_equal(got, want), ("PreCompFirstOrder", _diff_report(got, want))
        want = orc.walks_first_order(indptr, indices, data, starts, wc.L, wc.SEED, precomp=False)
        got = eng.simulate("FirstOrderUnweighted", 1, 1, False, starts, wc.L, seed=wc.SEED)
        assert np.array_equal(got, want), ("FirstOrderUnweighted", _diff_report(got, want))
    eng.close()


def _dense_thr(mat, kind):
    n = mat.shape[0]
    if kind == "hand":
        return np.array([0.0, 2.0 ** -140, np.finfo(np.float32).max], dtype=np.float32)[np.arange(n) % 3].copy()
    thr = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            row = mat[i, mat[i] != 0]
            thr[i] = row.mean() if row.size else 0.0
    return np.nan_to_num(thr, nan=0.0)


@pytest.mark.parametrize("family", ["loguniform64", "spike64", "huge64"])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("ext", [None, "g0", "hand"])
def test_dense_bounded_complete_and_exact_equal_the_oracle(family, symmetric, ext, monkeypatch):
    """DenseOTF from the float64 matrix: the bounded kernel, the complete kernel (``PECANPY_AMD_DENSE_NO_WFAST``) and the
    in-kernel float64 chain on every fifth step (``PECANPY_AMD_DENSE_EXACT_TEST=5``) give the oracle's walks.  On ``huge64`` the
    float64 row total is +inf, the probabilities are zero and every draw r > 0 is a read at ``choice == degree``: the
    reference reads past a temporary there, the oracle and the kernels clamp it to the last neighbour and count it, and the
    counts are compared; the other families have no such read (asserted)."""
    mat = wc.dense(family, symmetric)
    n = mat.shape[0]
    thr = None if ext is None else _dense_thr(mat, ext)
    starts = orc.shuffled_starts(n, 2, wc.SEED)
    eng = WalkEngine.from_dense(np.array(mat))
    if thr is not None:
        eng.set_thresholds(thr)
    for p, q in wc.PQ[:2]:
        with np.errstate(all="ignore"):
            want, ost = orc.walks_dense_otf(mat, p, q, starts, wc.L, wc.SEED, thr=thr, return_stats=True)
        assert ost.overflow_reads == ost.clamped_reads and (ost.overflow_reads >= 3000 if family == "huge64" else ost.overflow_reads == 0), ost.overflow_reads
        runs = {}
        for what, env in (("bounded", ()), ("complete", (("PECANPY_AMD_DENSE_NO_WFAST", "1"),)),
                          ("exact", (("PECANPY_AMD_DENSE_EXACT_TEST", "5"),))):
            with monkeypatch.context() as m:
                for k, v in env:
                    m.setenv(k, v)
                runs[what] = eng.simulate("DenseOTF", p, q, ext is not None, starts, wc.L, seed=wc.SEED)
                st = dict(eng.last_stats)
            print(family, symmetric, ext, p, q, what, {k: st[k] for k in ("total_steps", "overflow_reads", "ambiguous_steps", "redo_walks")})
            assert np.array_equal(runs[what], want), (what, p, q, _diff_report(runs[what], want))
            assert (st["total_steps"], st["overflow_reads"], st["clamped_reads"]) == (ost.total_steps, ost.overflow_reads, ost.clamped_reads), (what, st)
    eng.close()


def test_one_handle_through_thresholds_and_parameters_and_back(monkeypatch):
    """One handle (it owns its graph, so the weights stay ``huge_pq``): thresholds uploaded, a walk, other thresholds, the two
    overflowing (p, q) pairs, and back to the first thresholds and pair.  Every call is the oracle's and the first walks
    return bit for bit."""
    indptr, indices, data = wc.graph("rmat9", "huge_pq")
    eng = WalkEngine.from_csr(indptr, indices, data)
    first = got = None
    for ext, p, q in (("g0", 0.5, 2.0), ("hand", 0.5, 2.0), ("hand", 1.0 / wc.P_EXT, wc.P_EXT), ("g0", wc.P_EXT, 1.0 / wc.P_EXT),
                      ("g0", 0.5, 2.0)):
        c = wc.Case("rmat9", "huge_pq", p, q, ext)
        eng.set_thresholds(wc.case_thr(c))
        got = _walk(eng, c, (), monkeypatch)[0]
        want = wc.oracle_sparse(c)[0]
        assert np.array_equal(got, want), (ext, p, q, _diff_report(got, want))
        if first is None:
            first = got
    assert np.array_equal(got, first)
    eng.close()


# ---- node2vec++ ----------------------------------------------------------------------------------------------------------------
# The reference's formula divides by 1 + (b - 1) with b = w / thr (experimental.py:88-92): for b < 2^-53 that is 0 and the
# value is inf or NaN.  On ``moderate``, ``loguniform`` and ``spike`` more than half of the steps have such a vector in the
# restated reference itself (test_wide_weights_host.py asserts it), and what a search over NaNs returns is not pinned; the
# staircases stay finite and are the cases here.
PP_ENVS = (("bounded", ()), ("complete", (("PECANPY_AMD_DENSE_NO_WFAST", "1"),)), ("exact", (("PECANPY_AMD_DENSE_EXACT_TEST", "5"),)))


def _pp_runs(eng, mode, p, q, starts, want, what, monkeypatch):
    for name, env in PP_ENVS:
        with monkeypatch.context() as m:
            for k, v in env:
                m.setenv(k, v)
            got = eng.simulate(mode, p, q, False, starts, wc.L, seed=wc.SEED)
            st = dict(eng.last_stats)
        print(what, name, {k: st[k] for k in ("total_steps", "ambiguous_steps", "redo_walks")})
        assert np.array_equal(got, want), (what, name, _diff_report(got, want))
        assert st["total_steps"] == int((want[:, -1].astype(np.int64) - 1).sum()), (what, name, st)


@pytest.mark.parametrize("family", wc.PP_FAMILIES64)
@pytest.mark.parametrize("symmetric", [True, False])
def test_dense_node2vec_plusplus_equals_the_restated_reference(family, symmetric, monkeypatch):
    """``experimental.Node2vecPlusPlus`` on the dense handle: bounded, complete and in-kernel exact chain against
    ``n2vpp_restated.random_walks``."""
    import n2vpp_restated as rs

    mat = np.array(wc.dense(family, symmetric))
    starts = rs.start_array(mat.shape[0], 2, wc.SEED)
    eng = WalkEngine.from_dense(mat)
    for p, q, gamma in wc.PP_PARAMS:
        thr = rs.noise_thresholds(mat, gamma)
        eng.set_thresholds(thr)
        want = rs.random_walks(mat, p, q, gamma, wc.SEED, starts, wc.L, thr=thr)
        _pp_runs(eng, "Node2vecPlusPlus", p, q, starts, want, (family, symmetric, p, q), monkeypatch)
    eng.close()


@pytest.mark.parametrize("name,family", wc.PP_SPARSE)
def test_sparse_node2vec_plusplus_equals_the_restated_reference(name, family, monkeypatch):
    """``SparseNode2vecPlusPlus`` on the CSR handle against ``n2vpp_sparse_restated.random_walks``."""
    import n2vpp_restated as rs
    import n2vpp_sparse_restated as srs

    indptr, indices, data = wc.graph(name, family)
    starts = rs.start_array(indptr.size - 1, wc.NUM_WALKS[name], wc.SEED)
    eng = WalkEngine.from_csr(indptr, indices, data)
    for p, q, gamma in wc.PP_PARAMS:
        thr = srs.noise_thresholds(indptr.astype(np.int64), data, gamma)
        eng.set_thresholds(thr)
        want = srs.random_walks(indptr, indices, data, p, q, gamma, wc.SEED, starts, wc.L, thr=thr)
        _pp_runs(eng, "SparseNode2vecPlusPlus", p, q, starts, want, (name, family, p, q), monkeypatch)
    eng.close()
