"""Wide-range weights on the CPU: the host hooks of the binade scan and of the weighted lane decision against NumPy's sequential
chain, and conditions on the ORACLE ALONE which show that the cases of ``test_gpu_wide_weights.py`` are what they claim (so
that equality with the oracle there cannot hold vacuously).  Reference-generated fixtures on the same families
(``golden/wide_*.npz``, written by ``golden/make_golden_wide.py``) pin the oracle itself through ``test_oracle_golden.py``.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import wide_weight_cases as wc
from oracle import pyoracle as orc
from pecanpy_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEGREES = [1, 2, 3, 63, 64, 65, 300, 2245, 20000]
KINDS = ("loguniform", "moderate", "spike", "stair_down", "stair_up", "huge")
LANE_AMBIGUOUS = 0xFFFFFFFD


def vector(kind, d, dtype, seed):
    """``d`` weights of a family as one row (the graph-free form of ``wide_weight_cases.csr_weights``; float64: the dense
    analogues -- exponents in [-1000, 900], a spike of 5e-324, ``huge`` near 2^1023)."""
    f64 = dtype == np.float64
    x = wc.mix(np.arange(d, dtype=np.int64), np.full(d, 7919 * seed + 1, dtype=np.int64), seed)
    bits = 40 if f64 else 23
    pos = np.arange(d)
    with np.errstate(under="ignore"):
        if kind == "loguniform":
            m, e = wc.mantissa_exponent(x, *((-1000, 901) if f64 else (-140, 101)), bits)
        elif kind == "moderate":
            m, e = wc.mantissa_exponent(x, -30, 31, bits)
        elif kind == "huge":
            m, e = wc.mantissa_exponent(x, *((1000, 1024) if f64 else (100, 127)), bits)
        elif kind == "spike":
            w = np.full(d, 5e-324 if f64 else 2.0 ** -149)
            w[int(x[0] % np.uint64(d))] = 1.0
            return w.astype(dtype)
        elif kind == "stair_down":
            m, e = np.ones(d), -(pos % 60)
        else:
            m, e = np.ones(d), -(59 - pos % 60)
        return np.ldexp(m, e).astype(dtype)


def _scan(x, r, use_target, chunk):
    lib = _lib.load()
    idx = C.c_uint32()
    f32 = x.dtype == np.float32
    s = C.c_float() if f32 else C.c_double()
    fn = lib.pw_selftest_seqscan_f32 if f32 else lib.pw_selftest_seqscan_f64
    _lib.check(fn(C.c_void_p(x.ctypes.data), x.size, float(r), int(use_target), chunk, C.byref(idx), C.byref(s)))
    return idx.value, x.dtype.type(s.value)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_binade_scan_equals_sequential_cumsum_on_wide_weights(kind, dtype):
    """The protocol of ``test_stream.py::test_binade_scan_equals_sequential_cumsum`` on the wide families: the scan's total is
    the sequential same-dtype sum bit for bit -- +inf where that overflows (before the fix in ``Binade::quantize`` the scan
    returned NaN there: 41 of 41 such float32 rows) -- and its search is ``np.searchsorted(np.cumsum(w / tot), r)`` for uniform
    draws, 0, the last CDF value and its successor, values on and one ulp either side of sampled partial sums, and 1 - 2^-53."""
    rng = np.random.default_rng(5)
    n_inf = 0
    for d in DEGREES:
        for trial in range(2):
            w = vector(kind, d, dtype, seed=3 * d + trial)
            with np.errstate(all="ignore"):
                cs = np.cumsum(w, dtype=dtype)
                pr = (w / cs[-1]).astype(dtype)
                cdf = np.cumsum(pr, dtype=dtype)
            n_inf += int(np.isinf(cs[-1]))
            for chunk in (1, 5, 64, 256):
                _, tot = _scan(w, 0.0, False, chunk)
                assert tot.tobytes() == cs[-1].tobytes(), (kind, d, chunk, tot, cs[-1])
            pick = cdf[rng.integers(0, d, min(d, 6))].astype(np.float64)
            targets = np.concatenate([rng.random(3), [0.0, float(cdf[-1]), float(np.nextafter(cdf[-1], dtype(2))), 1.0 - 2.0 ** -53],
                                      pick, np.nextafter(pick.astype(dtype), dtype(0)).astype(np.float64),
                                      np.nextafter(pick.astype(dtype), dtype(2)).astype(np.float64)])
            targets = targets[(targets >= 0) & (targets < 1)]
            want = np.searchsorted(cdf.astype(np.float64), targets, side="left")
            for i, r in enumerate(targets):
                got, _ = _scan(pr, r, True, (1, 5, 64, 256)[i % 4])
                assert got == int(want[i]), (kind, d, trial, r, got, int(want[i]))
    if kind == "huge":
        assert n_inf >= 4           # (the rows of 2245 and 20000 entries hold dozens of values >= 2^125 (2^1022): 8 of them overflow)


def _weighted_run(vals, base, cls, r):
    vals, base = np.ascontiguousarray(vals, np.float32), np.ascontiguousarray(base, np.float32)
    cls, r = np.ascontiguousarray(cls, np.uint8), np.ascontiguousarray(r, np.float64)
    chain, lane = np.zeros(r.size, np.uint32), np.zeros(r.size, np.uint32)
    _lib.check(_lib.load().pw_selftest_lane_weighted(
        vals.ctypes.data_as(C.c_void_p), base.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p), vals.size,
        r.ctypes.data_as(C.c_void_p), r.size, chain.ctypes.data_as(C.c_void_p), lane.ctypes.data_as(C.c_void_p)))
    return chain, lane


@pytest.mark.parametrize("kind", KINDS)
def test_weighted_lane_decision_never_disagrees_with_the_chain_on_wide_weights(kind, capsys):
    """``test_weighted_lane_decision_never_disagrees_with_the_float32_chain`` with the wide weight vectors: every target the
    bound SETTLES is the chain's position (the hook's chain is checked against NumPy's first); what it leaves open is
    printed, not asserted."""
    rs = np.random.RandomState(17)
    settled = total = 0
    for n in (1, 3, 17, 64, 300, 1000, 3000):
        for trial in range(4):
            w = vector(kind, n, np.float32, seed=n + trial)
            q = float(rs.choice([2.0, 0.5, 1.7, 0.3]))
            p = float(rs.choice([0.5, 2.0, 0.3]))
            cls = np.zeros(n, np.uint8)
            cls[rs.choice(n, int(rs.randint(0, max(1, n // 3))), replace=False)] = 1
            cand = np.flatnonzero(cls == 0)
            if cand.size and trial != 3:
                cls[rs.choice(cand)] = 2
            with np.errstate(all="ignore"):
                base = (w.astype(np.float64) / q).astype(np.float32)
                vals = base.copy()
                vals[cls == 1] = w[cls == 1]
                vals[cls == 2] = (w[cls == 2].astype(np.float64) / p).astype(np.float32)
                if not np.all(np.isfinite(vals)):
                    continue                       # (a single value of +inf: no case, wide_weight_cases.element_overflows)
                t = np.cumsum(vals, dtype=np.float32)[-1]
                c = np.cumsum((vals / t).astype(np.float32), dtype=np.float32).astype(np.float64)
            pick = rs.choice(n, min(n, 100), replace=False)
            r = np.concatenate([rs.random_sample(200), c[pick], np.nextafter(c[pick], 0), np.nextafter(c[pick], 2), [0.0, 0.9999999999]])
            r = np.clip(r, 0, 0.9999999999)
            chain, lane = _weighted_run(vals, base, cls, r)
            assert np.array_equal(chain, np.searchsorted(c, r, side="left").astype(np.uint32)), (kind, n, trial)
            decided = lane != LANE_AMBIGUOUS
            assert np.array_equal(lane[decided], chain[decided]), (kind, n, p, q, trial, np.flatnonzero(lane[decided] != chain[decided])[:5])
            settled += int(decided.sum())
            total += r.size
    with capsys.disabled():
        print(f"\n[wide weights] lane_decide_weighted on {kind}: {settled}/{total} targets settled ({settled / max(total, 1):.3f})")


# ---- the inputs are what they claim: conditions on the oracle and on NumPy's sequential float32 chain ---------------------------
def _step_values(c, cur, prev):
    """Unnormalised float32 values of the step prev -> cur, from the oracle's probabilities is not possible (they are divided):
    restated with NumPy for node2vec (the conditions below are checked on node2vec steps and on first steps)."""
    indptr, indices, data = wc.graph(c.graph, c.family)
    s0, s1 = int(indptr[cur]), int(indptr[cur + 1])
    w = data[s0:s1].astype(np.float64)
    if prev is not None:
        nb = indices[s0:s1]
        pn = indices[int(indptr[prev]): int(indptr[prev + 1])]
        out = ~np.isin(nb, pn) & (nb != prev)
        w = np.where(out, w / c.q, w)
        w = np.where(nb == prev, w / c.p, w)
    with np.errstate(over="ignore", under="ignore"):
        return w.astype(np.float32)


def _facts_of_case(c, rows=120):
    mat = wc.oracle_sparse(c)[0]
    best = dict(span=0, absorbed=0, subnormal=0, inf=0)
    for row in mat[:rows]:
        for j in range(1, min(int(row[-1]), 6)):
            cur, prev = int(row[j - 1]), (int(row[j - 2]) if j >= 2 and c.ext is None else None)
            tot, span, absorbed, subnormal = wc.row_facts(_step_values(c, cur, prev))
            best["span"] = max(best["span"], span)
            best["absorbed"] += absorbed
            best["subnormal"] += subnormal
            best["inf"] += int(np.isinf(tot))
    return best


@pytest.mark.parametrize("c", wc.SPARSE_CASES, ids=wc.case_id)
def test_sparse_cases_are_what_they_claim(c):
    """Per GPU case, on the oracle's walks and NumPy's sequential float32 arithmetic over walked rows: at least 5 000 sampled
    steps, no clamped read (the last non-empty row is tame), and the family's own property -- a CDF chain that spans >= 40
    binades (``loguniform``, ``stair_up``: its first positive partial sum and its last lie >= 40 exponents apart; a crossing
    element is one real addition in the scan however many binades it jumps), absorbed elements (``stair_down``, ``spike``),
    subnormal quotients (``spike``, ``loguniform``), a total of +inf and >= 50 reads at ``choice == degree`` (``huge``; ``huge_pq``
    at q = 2^-40) on the R-MAT.

    ``spike`` cannot produce reads at ``choice == degree``: every row holds at least one 1.0, the other quotients are at most
    2^-149 each, so the CDF ends within d * 2^-24 of 1 -- the oracle counts 0 such reads in every ``spike`` case, which is
    asserted here as what the family does; the read is exercised by ``huge`` instead (> 20 000 per R-MAT case)."""
    mat, ov, clamped, steps = wc.oracle_sparse(c)
    assert clamped == 0 and steps >= 5000, (clamped, steps)
    f = _facts_of_case(c)
    big = c.graph in ("rmat9", "rmat9d")
    if c.family in ("loguniform", "stair_up"):
        assert f["span"] >= (40 if c.graph != "ring" else 24), f         # (a ring row has 24 entries)
    if c.family in ("stair_down", "spike") and big:
        assert f["absorbed"] >= 1, f
    if c.family in ("spike", "loguniform"):
        assert f["subnormal"] >= 1, f
    if c.family == "spike":
        assert ov == 0
    if c.family == "huge" and c.graph == "rmat9":
        assert f["inf"] >= 1 and ov >= 50, (f, ov)
    if c.family == "huge_pq" and c.graph == "rmat9":
        assert (ov >= 50) == (c.q == wc.P_EXT), (ov, c)


def test_graphs_have_the_structure_the_paths_need():
    deg = lambda name: np.diff(wc.pattern(name)[0].astype(np.int64))      # noqa: E731
    assert deg("rmat9").max() > 256                       # the weighted lane form records its chain every 256 elements
    assert deg("star")[0] == 40 and deg("star").size == 41
    assert np.all(deg("rmat9d")[::13] == 0) and deg("rmat9d").max() > 64
    assert np.all(deg("ring") == 24)
    for fam in wc.FAMILIES64:
        for sym in (True, False):
            a = wc.dense(fam, sym)
            assert a.shape == (130, 130) and (a != 0).sum(axis=1).max() > 2 * 64 * 0.25 and bool(((a != 0) == (a != 0).T).all()) == sym
    for fam in wc.FAMILIES:
        _, _, data = wc.graph("rmat9", fam)
        assert data.dtype == np.float32 and np.all(np.isfinite(data)) and np.all(data > 0)
    thr = wc.thresholds("rmat9", "loguniform", "hand")
    data = wc.graph("rmat9", "loguniform")[2]
    assert thr[0] == 0 and 0 < thr[1] < np.finfo(np.float32).tiny and thr[2] >= data.max()


# ---- node2vec++: where the reference's own formula stays finite --------------------------------------------------------------
def _pp_nonfinite_dense(mat, p, q, gamma):
    import n2vpp_restated as rs

    nz = mat != 0
    thr = rs.noise_thresholds(mat, gamma)
    bad = tot = 0
    for cur in range(mat.shape[0]):
        for prev in np.nonzero(nz[cur])[0]:
            pr = rs.normalized_probs(mat, nz, p, q, cur, int(prev), thr)
            tot += 1
            bad += int(not np.all(np.isfinite(pr)))
    return bad, tot


@pytest.mark.parametrize("symmetric", [True, False])
def test_node2vec_plusplus_cases_are_those_the_reference_defines(symmetric):
    """experimental.py:88-92 divides by 1 + (b - 1), b = w / thr: 0 for b < 2^-53, so the value is inf or NaN.  On the dense
    staircases every step out of every entry has a finite vector (the GPU cases); on ``moderate64``, ``loguniform64`` and
    ``spike64`` a large share has not, in the restated reference itself -- those are no node2vec++ cases."""
    for fam in wc.PP_FAMILIES64:
        for p, q, gamma in wc.PP_PARAMS:
            assert _pp_nonfinite_dense(np.array(wc.dense(fam, symmetric)), p, q, gamma)[0] == 0, (fam, p, q)
    for fam in ("moderate64", "loguniform64", "spike64"):
        bad, tot = _pp_nonfinite_dense(np.array(wc.dense(fam, symmetric)), 0.5, 2.0, 0.0)
        assert bad > tot // 10, (fam, bad, tot)


@pytest.mark.parametrize("name,family", wc.PP_SPARSE)
def test_sparse_node2vec_plusplus_cases_stay_finite(name, family):
    """Every (prev, cur) entry of the graph, both parameter sets: the restated CSR reference gives a finite vector."""
    import n2vpp_sparse_restated as srs

    indptr, indices, data = wc.graph(name, family)
    ip = indptr.astype(np.int64)
    for p, q, gamma in wc.PP_PARAMS:
        thr = srs.noise_thresholds(ip, data, gamma)
        for prev in range(ip.size - 1):
            for cur in indices[ip[prev]: ip[prev + 1]][:: 1 if name != "rmat9" else 3]:
                if ip[cur] == ip[cur + 1]:
                    continue
                pr = srs.normalized_probs(ip, indices, data, p, q, int(cur), prev, thr)
                assert np.all(np.isfinite(pr)), (name, family, p, q, prev, int(cur))


# ---- the reference on these inputs ------------------------------------------------------------------------------------------
WIDE_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "wide_*.npz")))


def test_reference_fixtures_exist_and_record_the_reference_s_warnings():
    """``make_golden_wide.py`` ran the reference itself.  It raised on no case.  Under NumPy it warns of float32 overflow in the
    sequential row total on the ``huge`` case (Numba does not report it) and of the mean of an empty row in the thresholds of
    the node2vec+ case (isolated vertices: NaN thresholds that are never read, as in the older fixtures); both are recorded in
    the fixtures.  node2vec+ on ``loguniform`` is no fixture: the reference's own thresholds overflow to NaN on walked rows
    (``make_golden_wide.DROPPED``).  ``test_oracle_golden.py`` and the GPU golden tests pick the files up by name pattern."""
    names = [os.path.basename(f)[:-4] for f in WIDE_FIXTURES]
    assert len(names) == 6 and sum("_huge_" in n for n in names) == 1, names
    assert "wide_loguniform_SparseOTF_n2vplus_p0.3_q1.7" not in names
    for f in WIDE_FIXTURES:
        z = np.load(f)
        assert z["indptr"].size == 65 and z["walks"].shape == (128, 14)
        warned = [str(w) for w in z["ref_warnings"]]
        if "_huge_" in f:
            assert warned == ["RuntimeWarning: overflow encountered in scalar add"], warned
        elif bool(z["extend"]):
            assert warned and not any("overflow" in w or "multiply" in w for w in warned), warned
        else:
            assert warned == [], (f, warned)
