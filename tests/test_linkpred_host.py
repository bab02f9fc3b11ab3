"""The link-prediction definitions on the host (no GPU): the selftest hooks with ``on_device = 0`` -- the host build of
csrc/linkpred.hip.h -- against the NumPy statements of pecanpy_amd/linkpred.py on every case of tests/linkpred_cases.py:
scores bit for bit, ``(wins, ties)`` and ``(u, v, candidates_used)`` equal; every refusal with nothing written; the Python
layer without a device; the flags of ``--task score``."""
import numpy as np
import pytest

import linkpred_cases as lc
from pecanpy_amd import _lib, cli, embed, linkpred
from pecanpy_amd import pecanpy as node2vec


# ---- pair scores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", (False, True), ids=("self", "second-matrix"))
@pytest.mark.parametrize("shape", lc.PAIR_SHAPES, ids=lambda s: f"n{s[0]}-d{s[1]}")
def test_pair_scores_host_build_equals_the_statement(shape, second):
    n, dim = shape
    for m in lc.PAIR_MS:
        A, B, u, v = lc.pair_case(n, dim, m, second)
        for metric in lc.METRICS:
            rc, score = lc.score_selftest(A, B, u, v, metric, on_device=0)
            assert rc == 0, lc.last_error()
            assert lc.same_bits(score, lc.score_statement(n, dim, m, second, metric)), (m, metric)


def test_pair_cases_hold_what_they_promise():
    A, B, u, v = lc.pair_case(700, 128, 1000, False)
    assert u[0] == v[0] and u[1] == v[1] and (u[2], v[2]) == (u[3], v[3]) == (u[4], v[4])
    cos, dot = lc.score_statement(700, 128, 1000, False, "cosine"), lc.score_statement(700, 128, 1000, False, "dot")
    assert cos[2] == cos[3] == cos[4] and abs(cos[0] - 1.0) < 1e-15
    for i in (1, 5, 6, 7):   # a zero row on either side: +0.0 under both metrics
        assert cos[i] == 0.0 and dot[i] == 0.0 and not np.signbit(cos[i]) and not np.signbit(dot[i])
    # the order of the additions shows: the float64 sum in another order differs somewhere
    other = (A[u].astype(np.float64)[:, ::-1] * A[v].astype(np.float64)[:, ::-1]).cumsum(axis=1)[:, -1]
    assert (other != dot).any()


def test_pair_scores_refusals_write_nothing():
    A, B, u, v = lc.pair_case(65, 37, 65, True)   # B has 68 rows
    for which, pos, row, needle in (("u", 40, 65, b"u[40] = 65 is outside the 65 rows"), ("v", 9, 68, b"v[9] = 68 is outside the 68 rows")):
        bu, bv = u.copy(), v.copy()
        (bu if which == "u" else bv)[pos] = row
        (bu if which == "u" else bv)[pos + 5] = 4000000000
        rc, score = lc.score_selftest(A, B, bu, bv, "cosine", on_device=0)
        assert rc == _lib.ERR_INVALID and needle in lc.last_error(), lc.last_error()
        assert np.isnan(score).all()
        with pytest.raises(ValueError, match=needle.decode().replace("[", r"\[").replace("]", r"\]")):
            linkpred.score_pairs_host(A, bu, bv, other=B)
    bu, bv = u.copy(), v.copy()
    bu[7], bv[7] = 65, 68   # both at one position: u is named
    rc, score = lc.score_selftest(A, B, bu, bv, "dot", on_device=0)
    assert rc == _lib.ERR_INVALID and b"u[7] = 65" in lc.last_error() and np.isnan(score).all()
    rc, score = lc.score_selftest(A, np.ascontiguousarray(B[:, :36]), u, v, "dot", on_device=0)
    assert rc == _lib.ERR_INVALID and b"dim 37 and 36" in lc.last_error() and np.isnan(score).all()
    with pytest.raises(ValueError, match="dim 37 and 36"):
        linkpred.score_pairs_host(A, u, v, other=B[:, :36])
    rc, score = lc.score_selftest(A, B, u, v, "dot", on_device=0)
    assert rc == 0
    assert _lib.load().pw_selftest_score_pairs(0, 0, lc._ptr(A), 65, None, 0, 37, 37, lc._ptr(u), lc._ptr(v), 65, 2, lc._ptr(score)) == _lib.ERR_INVALID
    assert b"metric" in lc.last_error()
    with pytest.raises(ValueError, match="metric"):
        linkpred.score_pairs_host(A, u, v, metric="euclid")


# ---- AUC ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.auc_cases()))
def test_auc_host_build_equals_the_statement(name):
    pos, neg = lc.auc_cases()[name]
    rc, wins, ties = lc.auc_selftest(pos, neg, on_device=0)
    assert rc == 0, lc.last_error()
    value, want_wins, want_ties = lc.auc_statement(name)
    assert (wins, ties) == (want_wins, want_ties)
    assert isinstance(want_wins, int) and isinstance(want_ties, int) and 0.0 <= value <= 1.0


def test_auc_statement_is_the_plain_count():
    assert lc.auc_statement("hand-4x2") == lc.HAND_ANSWER
    for name in ("signed-zeros-65x63", "infinities-63x65", "subnormals-200x200", "all-equal-63x65", "normal-63x65"):
        pos, neg = lc.auc_cases()[name]
        wins, ties = int((pos[:, None] > neg[None, :]).sum()), int((pos[:, None] == neg[None, :]).sum())
        assert lc.auc_statement(name)[1:] == (wins, ties), name
    assert lc.auc_statement("all-equal-63x65") == (0.5, 0, 63 * 65)
    pos, neg = lc.auc_cases()["signed-zeros-65x63"]
    assert (np.signbit(pos) & (pos == 0)).any() and ((~np.signbit(neg)) & (neg == 0)).any()


def test_auc_refusals_write_nothing():
    pos, neg = (x.copy() for x in lc.auc_cases()["normal-63x65"])
    for name, arr, at in (("pos", pos, 17), ("neg", neg, 60)):
        arr[at] = np.nan
        arr[at + 2] = np.nan
        rc, wins, ties = lc.auc_selftest(pos, neg, on_device=0)
        assert rc == _lib.ERR_INVALID and f"{name}[{at}] is a NaN".encode() in lc.last_error(), lc.last_error()
        assert (wins, ties) == (0xDEAD, 0xDEAD)
        with pytest.raises(ValueError, match=rf"{name}\[{at}\] is a NaN"):
            linkpred.auc_host(pos, neg)
        arr[at] = arr[at + 2] = 0.0
    pos[3] = neg[1] = np.nan   # one in each: pos is named
    assert lc.auc_selftest(pos, neg, on_device=0)[0] == _lib.ERR_INVALID and b"pos[3]" in lc.last_error()
    assert lc.auc_selftest(pos[:0], neg, on_device=0)[0] == _lib.ERR_INVALID
    assert lc.auc_selftest(neg, pos[:0], on_device=0)[0] == _lib.ERR_INVALID
    with pytest.raises(ValueError, match="at least one"):
        linkpred.auc_host([], [1.0])
    out = (lc.C.c_uint64 * 2)(7, 7)
    one = np.zeros(1)
    assert _lib.load().pw_selftest_auc(0, 0, lc._ptr(one), 2 ** 31, lc._ptr(one), 2 ** 31, out) == _lib.ERR_INVALID   # m * n = 2^62
    assert b"2^62" in lc.last_error() and (out[0], out[1]) == (7, 7)


# ---- sampler -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.graphs()))
def test_sampler_host_build_equals_the_statement(name):
    graph = lc.graphs()[name]
    indptr, indices = graph
    edges = {(r, int(c)) for r in range(indptr.size - 1) for c in indices[indptr[r]:indptr[r + 1]]}
    for m in lc.SAMPLE_MS:
        rc, u, v, used = lc.sample_selftest(graph, 11, 0, m, on_device=0)
        assert rc == 0, lc.last_error()
        want_u, want_v, want_used = lc.sample_statement(name, 11, 0, m)
        assert np.array_equal(u, want_u) and np.array_equal(v, want_v) and used == want_used
        assert used >= m and (m > 0 or used == 0)
        assert all(a != b and (int(a), int(b)) not in edges for a, b in zip(u, v))   # no loop, no edge


@pytest.mark.parametrize("name", list(lc.graphs()))
def test_sampler_prefix_and_continuation(name):
    graph = lc.graphs()[name]
    for first in (0, 12345):
        _, u, v, used = lc.sample_selftest(graph, 3, first, 300, on_device=0)
        rc1, u1, v1, used1 = lc.sample_selftest(graph, 3, first, 100, on_device=0)
        rc2, u2, v2, used2 = lc.sample_selftest(graph, 3, first + used1, 200, on_device=0)
        assert rc1 == 0 and rc2 == 0
        assert np.array_equal(u[:100], u1) and np.array_equal(v[:100], v1)           # sample(m1 + m2) has sample(m1) as its prefix
        assert np.array_equal(u[100:], u2) and np.array_equal(v[100:], v2) and used1 + used2 == used   # ... and the second call continues
        su, sv, sused = linkpred.sample_non_edges_host(*graph, 200, 3, first + used1)
        assert np.array_equal(su, u2) and np.array_equal(sv, v2) and sused == used2


def test_sampler_refusals_write_nothing():
    rc, u, v, used = lc.sample_selftest(lc.COMPLETE_5, 1, 0, 4, on_device=0)
    assert rc == _lib.ERR_INVALID and b"no off-diagonal non-edge" in lc.last_error()
    assert (u == 0xDEADBEEF).all() and (v == 0xDEADBEEF).all() and used == 0xDEAD
    with pytest.raises(ValueError, match="no off-diagonal non-edge"):
        linkpred.sample_non_edges_host(*lc.COMPLETE_5, 4, 1)
    one = (np.zeros(2, dtype=np.uint32), np.zeros(0, dtype=np.uint32))   # one vertex: nothing off the diagonal
    assert lc.sample_selftest(one, 1, 0, 1, on_device=0)[0] == _lib.ERR_INVALID


def test_sampler_cap():
    """One acceptable pair among 256 and a stretch of the stream that does not draw it: the cap of 16 * 256 + 64 candidates ends
    the call, in the host build and in the statement alike; where the pair is drawn in time both give it."""
    graph = lc.cap_graph(lc.CAP_ARC)
    assert linkpred.candidate_cap(1, 16, 1) == 4160
    rc, u, v, used = lc.sample_selftest(graph, lc.CAP_SEED, lc.CAP_FIRST, 1, on_device=0)
    assert rc == _lib.ERR_INVALID and b"4160 candidates examined (the cap) gave 0 of the 1 non-edges" in lc.last_error(), lc.last_error()
    assert u[0] == 0xDEADBEEF and v[0] == 0xDEADBEEF and used == 0xDEAD
    with pytest.raises(ValueError, match=r"4160 candidates examined \(the cap\) gave 0 of the 1"):
        linkpred.sample_non_edges_host(*graph, 1, lc.CAP_SEED, lc.CAP_FIRST)
    rc, u, v, used = lc.sample_selftest(graph, lc.CAP_SEED, lc.CAP_FIRST - 1, 1, on_device=0)   # the candidate before is the pair
    assert rc == 0 and (int(u[0]), int(v[0])) == tuple(lc.CAP_ARC) and used == 1
    assert linkpred.sample_non_edges_host(*graph, 1, lc.CAP_SEED, lc.CAP_FIRST - 1)[2] == 1


# ---- the Python layer and the CLI --------------------------------------------------------------------------------------
@pytest.mark.skipif(_lib.load().pw_device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_device_entry_points_need_a_device_and_say_so():
    with pytest.raises(_lib.PwError, match="no HIP device"):
        linkpred.auc(np.ones(3), np.zeros(2))
    indptr, indices = lc.graphs()["karate"]
    g = node2vec.SparseOTF.from_csr(indptr, indices, None)
    with pytest.raises(_lib.PwError, match="no HIP device"):
        g.sample_non_edges(4, seed=1)
    with pytest.raises(_lib.PwError, match="no HIP device"):
        embed.KnnIndex(np.ones((6, 4), dtype=np.float32)).score_pairs([0], [1])


def test_dense_graphs_have_no_sampler():
    g = node2vec.DenseOTF.from_mat(np.ones((4, 4)) - np.eye(4), ["a", "b", "c", "d"])
    with pytest.raises(NotImplementedError, match="sparse"):
        g.sample_non_edges(2, seed=1)


def test_the_names_are_where_knn_index_is():
    for name in ("auc", "auc_host", "link_auc", "score_pairs_host", "sample_non_edges_host"):
        assert getattr(embed, name) is getattr(linkpred, name)
    assert callable(embed.KnnIndex.score_pairs) and callable(embed.SgnsSession.score_pairs) and callable(node2vec.Base.sample_non_edges)


def test_cli_flags_of_task_score(capsys):
    args = cli.parse_args(["--input", "a.emb", "--output", "b.tsv", "--task", "score", "--pairs", "p.tsv"])
    assert (args.task, args.pairs, args.neg_pairs, args.metric, args.delimiter) == ("score", "p.tsv", None, "cosine", "\t")
    args = cli.parse_args(["--input", "a.emb", "--output", "b.tsv", "--task", "score", "--pairs", "p", "--neg_pairs", "n", "--metric", "dot"])
    assert (args.neg_pairs, args.metric) == ("n", "dot")
    with pytest.raises(SystemExit):
        cli.parse_args(["--input", "a.emb", "--output", "b.tsv", "--task", "score"])
    assert "--task score needs --pairs" in capsys.readouterr().err
    args = cli.parse_args(["--input", "a", "--output", "b"])   # every other task as before
    assert (args.task, args.pairs, args.metric, args.topn) == ("pecanpy", None, "cosine", 10)


def test_task_score_names_the_line_of_an_unknown_id(tmp_path):
    src, pairs = tmp_path / "in.npz", tmp_path / "pairs.tsv"
    np.savez(src, IDs=["a", "b", "c"], data=np.eye(3, dtype=np.float32))
    pairs.write_text("a\tb\nb\tzebra\n")
    with pytest.raises(ValueError, match="pairs.tsv, line 2: unknown node ID 'zebra'"):
        cli.main(["--input", str(src), "--output", str(tmp_path / "out.tsv"), "--task", "score", "--pairs", str(pairs)])
    pairs.write_text("a\tb\tc\n")
    with pytest.raises(ValueError, match="line 1: expected two node IDs, found 3 fields"):
        cli.main(["--input", str(src), "--output", str(tmp_path / "out.tsv"), "--task", "score", "--pairs", str(pairs)])
