"""The call scripts of ``table_history_cases.py`` on the CPU oracle alone: what makes the GPU tests mean something.

A GPU step that is served a table left by the step before it returns that step's walks.  The GPU test sees this only if the
oracle's walks of the two steps differ, so every pair of consecutive steps that is meant to differ must do so in at least HALF of
the rows (and, for alias steps of one kind, in half of the ``alias_q`` words); steps that return to an earlier state must equal it.
The bar is fixed: a pair that falls under it gets other parameters."""
import numpy as np
import pytest

import table_history_cases as tc

HALF = 0.5


@pytest.mark.parametrize("name", sorted(tc.SCRIPTS))
def test_consecutive_steps_differ_in_the_oracle_and_returns_are_equal(name):
    kind, script = tc.SCRIPTS[name]
    shares = []
    for i, s in enumerate(script):
        walks = tc.oracle_walks(kind, s)
        assert walks.shape == (tc.step_starts(s).size, tc.L + 2)
        if i and s.differs:
            prev = script[i - 1]
            share = tc.rows_differing(walks, tc.oracle_walks(kind, prev))
            shares.append(round(share, 3))
            assert share >= HALF, (name, i, share)
        else:
            assert i == 0 or s.n != script[i - 1].n, (name, i)      # (only the first step and the small calls are exempt)
        if s.same_as is not None:
            assert s.same_as < i - 1                                 # a return, not a repeat
            assert np.array_equal(walks, tc.oracle_walks(kind, script[s.same_as])), (name, i)
    print(name, "rows differing between consecutive steps:", shares)
    assert len(shares) >= len(script) - 2


@pytest.mark.parametrize("name", ["alias", "py_alias"])
def test_alias_tables_of_consecutive_steps_differ_and_returns_are_equal(name):
    kind, script = tc.SCRIPTS[name]
    indptr = tc.graph(kind)[0]
    deg = np.diff(indptr.astype(np.int64))
    sizes, shares = [], []
    for i, s in enumerate(script):
        aip, aj, aq = tc.oracle_tables(kind, s)
        assert aj.size == aq.size == (deg.sum() if s.mode == "PreCompFirstOrder" else (deg * deg).sum())
        sizes.append(aq.size)
        if i:
            paq = tc.oracle_tables(kind, script[i - 1])[2]
            if paq.size == aq.size:
                share = tc.words_differing(aq, paq)
                shares.append(round(share, 3))
                assert share >= HALF, (name, i, share)
        if s.same_as is not None:
            want = tc.oracle_tables(kind, script[s.same_as])
            assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                       for a, b in zip((aip, aj, aq), want)), (name, i)
    print(name, "alias_q words differing between consecutive steps:", shares, "sizes", sizes)
    if name == "alias":   # the kind switch changes the size in both directions
        k = [s.mode for s in script].index("PreCompFirstOrder")
        assert sizes[k - 1] > sizes[k] < sizes[k + 1]
        assert len(shares) == len(script) - 3
    else:
        assert len(shares) == len(script) - 1


def test_scripts_say_what_the_gpu_tests_rely_on():
    """The sizes the switches of the library compare, from the graphs themselves."""
    w, u = tc.graph("weighted"), tc.graph("unit")
    assert np.array_equal(w[0], u[0]) and np.array_equal(w[1], u[1]) and np.all(u[2] == 1)
    n, nnz = w[0].size - 1, w[1].size
    assert n == 256 and tc.starts().size == 512
    # a whole call samples at least as many steps as the graph has entries (tables are worth building), a small one fewer --
    # also than the unit graph's lines (entries + one per vertex at most)
    assert tc.starts().size * tc.L >= nnz + n > nnz > tc.SMALL * tc.L
    for name, (kind, script) in tc.SCRIPTS.items():
        for s in script:
            assert s.n in (None, tc.SMALL)
            if s.n == tc.SMALL:
                assert "PECANPY_AMD_FORCE_TOT" not in dict(s.env) and s.built is False
                assert all((s.p, s.q) != (o.p, o.q) for o in script if o is not s), name   # no table was built for it
    t0, t1 = tc.thresholds("T0"), tc.thresholds("T1")
    assert t0.dtype == np.float32 and np.isfinite(t0).all() and np.isfinite(t1).all()
    assert (t0 != t1).mean() >= HALF
    # unit row totals are keyed by the float32 biases: the steps change one of them at a time
    f = lambda x: np.float32(1.0 / x)
    a, b, c = tc.UNIT[0], tc.UNIT[1], tc.UNIT[2]
    assert f(a.p) == f(b.p) and f(a.q) != f(b.q) and f(c.p) != f(b.p) and f(c.q) == f(a.q)
    # the lane form's range of biases
    out = [s for s in tc.WLANE if not (1 / 1024 <= s.p <= 1024 and 1 / 1024 <= s.q <= 1024)]
    assert len(out) == 1 and out[0].not_lane == 3 and all(s.lane == 3 for s in tc.WLANE if s is not out[0])
    k = tc.WLANE.index(out[0])
    assert tc.WLANE[k + 1].same_as == k - 1 and tc.WLANE[k + 1][:5] == tc.WLANE[k - 1][:5]


def test_twin_case_puts_the_halves_on_opposite_sides_of_the_size_test():
    indptr, indices, data = tc.twin_graph()
    nnz = indices.size
    assert indptr.size - 1 == 1 << 16 and nnz == 2 * tc.TWIN_EDGES == 1048578
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr.astype(np.int64)))
    assert not (rows == indices).any()                                    # no self loops: the weighted lane form applies
    order = np.lexsort((rows, indices))                                   # the transpose, row by row
    assert np.array_equal(indices[order], rows) and np.array_equal(data[order], data)    # undirected, symmetric weights
    half = tc.TWIN_JOBS // 2
    assert tc.twin_starts().size == tc.TWIN_JOBS >= 1 << 20
    assert half * tc.TWIN_L < nnz <= (tc.TWIN_JOBS - half) * tc.TWIN_L
