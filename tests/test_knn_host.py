"""The nearest-neighbour definition on the host (no GPU): ``pw_selftest_knn(on_device=0)`` -- the host build of
csrc/knn.hip.h -- and ``embed.knn_host`` -- its NumPy statement -- against the naive reference (tests/knn_ref.py), ``idx``
equal and ``score`` bit for bit on every case of tests/knn_cases.py; every invalid argument refused with nothing written;
the flags of ``--task neighbours``."""
import ctypes as C
import sys
import types
import warnings

import numpy as np
import pytest

import knn_cases as kc
from pecanpy_amd import _lib, cli, embed


@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("case", kc.CASES, ids=kc.IDS)
def test_host_build_equals_the_reference(case, metric):
    rc, idx, score = kc.selftest(case, metric, on_device=0)
    assert rc == 0
    kc.assert_same(idx, score, *kc.reference(case, metric))


@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("case", kc.CASES, ids=kc.IDS)
def test_numpy_statement_equals_the_reference(case, metric):
    idx, score = embed.knn_host(case.X, queries=case.queries, rows=case.rows, topn=case.topn, metric=metric, exclude_self=case.exclude_self)
    assert idx.dtype == np.int64 and score.dtype == np.float64
    kc.assert_same(idx, score, *kc.reference(case, metric))


def test_the_facts_the_definition_rests_on():
    """Copies of a row scaled by powers of two score the same bits against it under cosine (the scaling is exact) and rank
    by row number; no score is -0.0; an all-negative database still fills the list."""
    case = next(c for c in kc.CASES if c.name == "ties-n257-d37-top10")
    idx, score = kc.reference(case, "cosine")   # query 0 is row 1: rows 0, 64, 65 and 256 are its copies
    assert list(idx[0][:4]) == [0, 64, 65, 256] and (score[0][:4] == score[0][0]).all() and abs(score[0][0] - 1.0) < 1e-15
    assert score[0][4] < score[0][0]
    for c in kc.CASES:
        for metric in kc.METRICS:
            s = kc.reference(c, metric)[1]
            assert not (np.signbit(s) & (s == 0.0)).any(), c
    neg = next(c for c in kc.CASES if c.name == "every-score-negative")
    idx, score = kc.reference(neg, "dot")
    assert (score[:, :128] < 0).all() and (idx >= 0).all()


def _refused(case, metric, needle, on_device=0):
    rc, idx, score = kc.selftest(case, metric, on_device)
    assert rc == _lib.ERR_INVALID
    assert needle in _lib.load().pw_last_error(), _lib.load().pw_last_error()
    assert (idx == 0xDEADBEEF).all() and np.isnan(score).all()   # nothing written


def test_invalid_arguments_are_refused_with_nothing_written():
    X = np.random.default_rng(1).standard_normal((20, 5)).astype(np.float32)
    rows = np.array([3, 4], dtype=np.uint32)
    for value in (np.nan, np.inf, -np.inf):
        bad = X.copy()
        bad[17, 2] = value
        bad[19, 0] = value
        _refused(kc.Case("bad-row", bad, rows=rows), "cosine", b"row 17 ")
        with pytest.raises(ValueError, match="row 17 "):
            embed.knn_host(bad, rows=rows)
        Q = X[:4].copy()
        Q[2, 4] = value
        _refused(kc.Case("bad-query", X, queries=Q), "dot", b"query 2 ")
        with pytest.raises(ValueError, match="query 2 "):
            embed.knn_host(X, queries=Q)
    for topn in (0, 129):
        _refused(kc.Case("topn", X, rows=rows, topn=topn), "dot", b"topn")
        with pytest.raises(ValueError, match="topn"):
            embed.knn_host(X, rows=rows, topn=topn)
    _refused(kc.Case("range", X, rows=np.array([3, 20], dtype=np.uint32)), "dot", b"row number 20 at position 1")
    with pytest.raises(ValueError, match="row number 20"):
        embed.knn_host(X, rows=[3, 20])
    with pytest.raises(ValueError, match="row number -1"):
        embed.knn_host(X, rows=[-1])
    with pytest.raises(ValueError, match="exactly one"):
        embed.knn_host(X)
    with pytest.raises(ValueError, match="exactly one"):
        embed.knn_host(X, queries=X[:1], rows=[0])
    with pytest.raises(ValueError, match="metric"):
        embed.knn_host(X, rows=[0], metric="euclid")


def test_the_c_entry_refuses_topn_and_pointer_combinations():
    lib = _lib.load()
    X = np.ones((4, 3), dtype=np.float32)
    rows = np.zeros(1, dtype=np.uint32)
    idx, score = np.full((1, 200), 7, dtype=np.uint32), np.full((1, 200), 7.0)

    def call(queries, rows_, topn, metric=1, n=4, dim=3):
        return lib.pw_selftest_knn(0, 0, C.c_void_p(X.ctypes.data), n, dim, queries, rows_, 1, topn, metric, 1, None,
                                   C.c_void_p(idx.ctypes.data), C.c_void_p(score.ctypes.data))

    pr, pq = C.c_void_p(rows.ctypes.data), C.c_void_p(X.ctypes.data)
    assert call(None, pr, 0) == _lib.ERR_INVALID and b"topn = 0" in lib.pw_last_error()
    assert call(None, pr, 129) == _lib.ERR_INVALID and b"topn = 129" in lib.pw_last_error()
    assert call(pq, pr, 1) == _lib.ERR_INVALID and b"exactly one" in lib.pw_last_error()
    assert call(None, None, 1) == _lib.ERR_INVALID and b"exactly one" in lib.pw_last_error()
    assert call(None, pr, 1, metric=2) == _lib.ERR_INVALID
    assert call(None, pr, 1, dim=0) == _lib.ERR_INVALID and call(None, pr, 1, dim=4097) == _lib.ERR_INVALID
    assert call(None, pr, 1, n=0) == _lib.ERR_INVALID
    assert (idx == 7).all() and (score == 7.0).all()
    assert call(None, pr, 128) == 0 and list(idx[0][:4]) == [1, 2, 3, 0xFFFFFFFF] and score[0][3] == -np.inf
    assert lib.pw_selftest_knn(0, 0, pq, 4, 3, None, pr, 0, 1, 1, 1, None, None, None) == 0   # nq = 0: a valid call that does nothing


def test_knn_index_checks_its_matrix_before_any_device_work(monkeypatch):
    import torch

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_library)
    X = np.ones((6, 4), dtype=np.float32)
    for bad, needle in ((X.astype(np.float64), "float32"), (torch.ones(6, 4, dtype=torch.float16), "float32"), (X[:, ::2], "contiguous"),
                        (torch.ones(4, 6).t(), "contiguous"), (X.ravel(), r"float32\[n, dim\]"), (X[:0], r"float32\[n, dim\]"),
                        (np.ones((2, 4097), dtype=np.float32), "dim <= 4096"), (X.tolist(), "torch tensor or a NumPy array")):
        with pytest.raises(ValueError, match=needle):
            embed.KnnIndex(bad)
    with pytest.raises(ValueError, match="5 node names for 6 rows"):
        embed.KnnIndex(X, node_ids=list("abcde"))


@pytest.mark.skipif(_lib.load().pw_device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_knn_index_needs_a_device_and_says_so():
    with pytest.raises(_lib.PwError, match="no HIP device"):
        embed.KnnIndex(np.ones((6, 4), dtype=np.float32))


def test_cli_flags_of_task_neighbours():
    args = cli.parse_args(["--input", "a.emb", "--output", "b.tsv", "--task", "neighbours"])
    assert (args.task, args.topn, args.metric, args.queries) == ("neighbours", 10, "cosine", None)
    args = cli.parse_args(["--input", "a.emb", "--output", "b.tsv", "--task", "neighbours", "--topn", "3", "--metric", "dot", "--queries", "q.txt"])
    assert (args.topn, args.metric, args.queries) == (3, "dot", "q.txt")
    with pytest.raises(SystemExit):
        cli.parse_args(["--input", "a", "--output", "b", "--task", "neighbours", "--metric", "euclid"])
    assert cli.parse_args(["--input", "a", "--output", "b"]).task == "pecanpy"   # every other task as before


class _HostIndex:
    """``KnnIndex`` by ``knn_host``: what ``--task neighbours`` does around the device call, without a device."""

    def __init__(self, vectors, node_ids=None):
        self.X = vectors

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def query(self, rows=None, topn=10, metric="cosine"):
        import torch

        idx, score = embed.knn_host(self.X, rows=rows, topn=topn, metric=metric)
        return torch.from_numpy(idx), torch.from_numpy(score)


def test_task_neighbours_warns_about_graph_and_trainer_flags_and_writes_the_lines(tmp_path, monkeypatch):
    monkeypatch.setattr(embed, "KnnIndex", _HostIndex)
    names = ["a", "b", "c", "d"]
    X = np.array([[1, 0], [2, 0], [0, 1], [1, 1]], dtype=np.float32)
    src, out = tmp_path / "in.npz", tmp_path / "out.tsv"
    np.savez(src, IDs=names, data=X)
    base = ["--input", str(src), "--output", str(out), "--task", "neighbours", "--topn", "2"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cli.main(base + ["--p", "0.5", "--weighted"])             # graph flags: ignored as --task train ignores them
    assert out.read_text() == ("a\tb\t1.000000\na\td\t0.707107\nb\ta\t1.000000\nb\td\t0.707107\n"
                               "c\td\t0.707107\nc\ta\t0.000000\nd\ta\t0.707107\nd\tb\t0.707107\n")
    with pytest.warns(UserWarning, match="--task neighbours has none, so they are ignored"):
        cli.main(base + ["--fresh_walks"])
    with pytest.warns(UserWarning, match="--task neighbours has no graph, so they are ignored"):
        cli.main(base + ["--freeze_init"])
    q = tmp_path / "q.txt"
    q.write_text("d\nzebra\n")
    with pytest.raises(ValueError, match="unknown node ID 'zebra'"):
        cli.main(base + ["--queries", str(q)])
