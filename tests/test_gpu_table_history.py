"""The tables a graph handle keeps between calls, held to the CPU oracle while their keys change and return.

Each test walks ONE handle through a script of ``table_history_cases.py``: thresholds replaced under tables that were built
from them, (p, q) and extend changed and changed back, the two alias kinds alternated, the modes interleaved.  Every step's
walks equal the oracle's exactly (the host test shows that consecutive steps differ in over 80 % of the rows there, so a table
served under the wrong key cannot pass), ``param_index_ms`` says which steps built tables, and where the script names it the
step also equals the same call on a fresh handle, integer statistics included.  One large case: the two halves of a twin call
that disagree about whether the normaliser table is worth building."""
import numpy as np
import pytest

import table_history_cases as tc
from pecanpy_amd import _lib
from pecanpy_amd.engine import WalkEngine

pytestmark = pytest.mark.gpu


def _diff(got, want):
    bad = (got != want).any(axis=1)
    return f"{int(bad.sum())}/{got.shape[0]} rows differ ({bad.mean():.3f})"


def _integers(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms")}


def _engine(kind):
    indptr, indices, data = tc.graph(kind)
    return WalkEngine.from_csr(indptr, indices, data if kind == "weighted" else None)


def _run_script(name, monkeypatch, after_step=None):
    """The script ``name`` on one handle: every step against the oracle, its statistics against the script's expectations,
    an immediate repeat of it (no table built, same walks) and, where named, the same call on a fresh handle."""
    kind, script = tc.SCRIPTS[name]
    eng = _engine(kind)
    uploaded = None
    for i, s in enumerate(script):
        if s.thr is not None and s.thr != uploaded:
            eng.set_thresholds(tc.thresholds(s.thr))
            uploaded = s.thr
        with monkeypatch.context() as mp:
            for k, v in s.env:
                mp.setenv(k, v)
            starts = tc.step_starts(s)
            got = eng.simulate(s.mode, s.p, s.q, s.extend, starts, tc.L, seed=tc.SEED)
            st = dict(eng.last_stats)
            want = tc.oracle_walks(kind, s)
            assert np.array_equal(got, want), (name, i, s, _diff(got, want))
            if s.built is True:
                assert st["param_index_ms"] > 0, (name, i, st)
            if s.built is False:
                assert st["param_index_ms"] == 0, (name, i, st)
            if s.lane is not None:
                assert st["lane_kernel"] == s.lane, (name, i, st)
            if s.not_lane is not None:
                assert st["lane_kernel"] != s.not_lane, (name, i, st)
            again = eng.simulate(s.mode, s.p, s.q, s.extend, starts, tc.L, seed=tc.SEED)
            assert np.array_equal(again, want), (name, i, "repeat", _diff(again, want))
            assert eng.last_stats["param_index_ms"] == 0, (name, i, "repeat", eng.last_stats)
            assert _integers(eng.last_stats) == _integers(st), (name, i, "repeat")
            if s.fresh:
                fresh = _engine(kind)
                if s.thr is not None:
                    fresh.set_thresholds(tc.thresholds(s.thr))
                alone = fresh.simulate(s.mode, s.p, s.q, s.extend, starts, tc.L, seed=tc.SEED)
                assert np.array_equal(alone, got), (name, i, "fresh handle")
                assert _integers(fresh.last_stats) == _integers(st), (name, i, fresh.last_stats, st)
                fresh.close()
        if after_step:
            after_step(eng, i, s)
    eng.close()


def _tables_equal(got, want, what):
    for g, w, part in zip(got, want, ("alias_indptr", "alias_j", "alias_q")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, part, g.shape, w.shape)
        if part == "alias_q":
            g, w = g.view(np.uint32), w.view(np.uint32)
            assert np.array_equal(g, w), (what, part, f"{float((g != w).mean()):.3f} of the words differ")
        else:
            assert np.array_equal(g, w), (what, part)


def test_alias_tables_follow_thresholds_parameters_and_kind():
    """PreComp on one handle: thresholds replaced under extend tables (before ``alias_thr_version``: the second step kept the
    tables of the first -- 84.4 % of the walk rows and 91.4 % of the ``alias_q`` words were those of gamma 0), extend off,
    another (p, q), the first-order kind (sum(deg) entries instead of sum(deg^2)) and back."""
    kind, script = tc.SCRIPTS["alias"]
    indptr = tc.graph(kind)[0]
    eng = _engine(kind)
    uploaded, sizes = None, []
    for i, s in enumerate(script):
        if s.thr != uploaded:
            eng.set_thresholds(tc.thresholds(s.thr))
            uploaded = s.thr
        got = eng.simulate(s.mode, s.p, s.q, s.extend, tc.starts(), tc.L, seed=tc.SEED)
        want = tc.oracle_walks(kind, s)
        assert np.array_equal(got, want), (i, s, _diff(got, want))
        first_order = s.mode == "PreCompFirstOrder"
        aip, aj, aq = eng.precomp_export(first_order)
        oip, oj, oq = tc.oracle_tables(kind, s)
        if first_order:     # (alias_indptr of this kind: the handle reports its own prefix of the degrees)
            assert np.array_equal(aip, indptr.astype(np.uint64))
        _tables_equal((aip, aj, aq), (oip, oj, oq), (i, s))
        sizes.append(aq.size)
    deg = np.diff(indptr.astype(np.int64))
    k = [s.mode for s in script].index("PreCompFirstOrder")
    assert sizes[k - 1] == sizes[k + 1] == (deg * deg).sum() and sizes[k] == deg.sum()
    # tables that the next call would build again are not handed out: an upload alone makes the export fail ...
    assert script[-1].extend and uploaded == "T0"
    eng.set_thresholds(tc.thresholds("T1"))
    with pytest.raises(_lib.PwError):
        eng.precomp_export(False)
    # ... and a build for the same (p, q, extend) replaces them
    eng.precomp_build(script[-1].p, script[-1].q, True, False)
    _tables_equal(eng.precomp_export(False), tc.oracle_tables(kind, script[1]), "rebuilt after an upload")
    # tables that read no thresholds stay: extend off, and the first-order kind
    eng.precomp_build(0.5, 2, False, False)
    eng.set_thresholds(tc.thresholds("T0"))
    _tables_equal(eng.precomp_export(False), tc.oracle_tables(kind, script[2]), "plain tables across an upload")
    eng.close()


def test_precomp_object_follows_gamma_and_parameters():
    """The same at the level of the mode class: ``gamma`` and ``(p, q)`` of a ``PreComp(extend=True)`` object change between
    calls; the mirrored ``alias_*`` arrays and the walks are the oracle's at every step (before ``alias_thr_version``: after
    ``gamma = 1`` both were still those of gamma 0)."""
    from pecanpy_amd import pecanpy as node2vec

    kind, script = tc.SCRIPTS["py_alias"]
    indptr, indices, data = tc.graph(kind)
    g = node2vec.PreComp.from_csr(indptr, indices, data, p=script[0].p, q=script[0].q, extend=True, gamma=0, random_state=tc.SEED)
    for i, s in enumerate(script):
        g.p, g.q, g.gamma = s.p, s.q, {"T0": 0, "T1": 1}[s.thr]
        with np.errstate(all="ignore"):       # (the mean of an empty row: NaN thresholds of isolated vertices, never read)
            g.preprocess_transition_probs()
            _tables_equal((g.alias_indptr, g.alias_j, g.alias_q), tc.oracle_tables(kind, s), (i, s))
            got = g.simulate_walks_array(2, tc.L)
        want = tc.oracle_walks(kind, s)
        assert np.array_equal(got, want), (i, s, _diff(got, want))
        assert np.array_equal(g.alias_dim, np.diff(indptr))


def test_normaliser_table_is_rebuilt_exactly_when_its_keys_change(monkeypatch):
    _run_script("normaliser", monkeypatch)


def test_weighted_lane_tables_follow_their_keys_and_survive_a_call_outside_the_form(monkeypatch):
    _run_script("wlane", monkeypatch)


def test_unit_row_totals_are_keyed_by_both_biases(monkeypatch):
    _run_script("unit", monkeypatch)


def test_modes_interleaved_on_one_weighted_handle(monkeypatch):
    def alias_tables(eng, i, s):
        if s.mode == "PreComp":
            _tables_equal(eng.precomp_export(False), tc.oracle_tables("weighted", s), (i, s))

    _run_script("interleaved", monkeypatch, alias_tables)


def test_twin_halves_that_disagree_about_the_normaliser_table(monkeypatch):
    """A twin call whose first half samples fewer steps than the graph has entries (it declines the normaliser table and
    walks the two-pass step) and whose second half samples as many (it builds the table, and the lane tables, in the graph
    data both contexts share): the walks of one context, and of the oracle; the tables left behind serve later calls under
    their own keys only."""
    import torch

    from oracle import pyoracle as orc

    indptr, indices, data = tc.twin_graph()
    nnz, starts, L, seed, p, q = indices.size, tc.twin_starts(), tc.TWIN_L, tc.TWIN_SEED, tc.TWIN_P, tc.TWIN_Q
    half = starts.size // 2
    assert starts.size >= 1 << 20 and half * L < nnz <= (starts.size - half) * L      # opposite sides of the size test
    d_starts = torch.from_numpy(starts.view(np.int32).copy()).cuda()      # (the shared array is read-only)
    eng, one = WalkEngine.from_csr(indptr, indices, data), WalkEngine.from_csr(indptr, indices, data)
    a = eng.simulate_device("SparseOTF", p, q, False, d_starts, L, seed=seed)
    sa = dict(eng.last_stats)
    monkeypatch.setenv("PECANPY_AMD_NO_TWIN", "1")
    b = one.simulate_device("SparseOTF", p, q, False, d_starts, L, seed=seed)
    sb = dict(one.last_stats)
    monkeypatch.delenv("PECANPY_AMD_NO_TWIN")
    print("twin halves:", sa, "one context:", sb)
    assert torch.equal(a, b), _diff(a.cpu().numpy(), b.cpu().numpy())
    assert sb["lane_kernel"] == 3 and sa["param_index_ms"] > 0 and sb["param_index_ms"] > 0, (sa, sb)
    assert (sa["total_steps"], sa["overflow_reads"], sa["dead_end_walks"]) == (sb["total_steps"], sb["overflow_reads"], sb["dead_end_walks"])
    a = a.cpu().numpy().view(np.uint32)
    want = orc.walks_sparse_otf(indptr, indices, data, p, q, starts[:1500], L, seed)
    assert np.array_equal(a[:1500], want), _diff(a[:1500], want)
    k = starts.size - 1500
    skip = int((a[:k, -1].astype(np.int64) - 1).sum())          # the draws of the rows before them
    want = orc.walks_sparse_otf(indptr, indices, data, p, q, starts[k:], L, seed, stream_skip=skip)
    assert np.array_equal(a[k:], want), _diff(a[k:], want)
    # later calls on the handle: a small one at another (p, q) (no table of its own: it must not read the one left behind),
    # then one at the first (p, q), served by the table the second half built
    for pp, qq in ((0.3, 1.7), (p, q)):
        got = eng.simulate("SparseOTF", pp, qq, False, starts[:512], L, seed=seed)
        assert 512 * L < nnz and eng.last_stats["param_index_ms"] == 0, eng.last_stats
        want = orc.walks_sparse_otf(indptr, indices, data, pp, qq, starts[:512], L, seed)
        assert np.array_equal(got, want), (pp, qq, _diff(got, want))
    eng.close()
    one.close()
