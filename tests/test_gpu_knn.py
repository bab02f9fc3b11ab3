"""(GPU) Nearest neighbours of embedding vectors on the device (csrc/knn.hip.h: ``pw_knn``, ``embed.KnnIndex``) against the
naive reference (tests/knn_ref.py): ``idx`` equal and ``score`` bit for bit on every case of tests/knn_cases.py, with the
default tiles and with forced tiles that make every seam happen at small n; the norms; device pointers; the snapshot a
session's index is; ``against="context"``; ``--task neighbours``; and one shape with many persistent passes per workgroup."""
import os

import numpy as np
import pytest

import knn_cases as kc
import knn_ref

pytestmark = pytest.mark.gpu

# (rows_per_block, queries_per_tile, grid, col_chunk): one workgroup walking every tile and block with one query per
# wavefront and a chunk that divides neither 128 nor 37; three workgroups (row parts, or tile parts once there are three
# tiles); two row groups with single queries; the widest block with the narrowest chunk
FORCED = ((64, 1, 1, 12), (64, kc.QT, 3, 32), (128, 1, 3, 20), (256, kc.QT, 0, 8))


@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("case", kc.CASES, ids=kc.IDS)
def test_device_equals_the_reference(case, metric):
    rc, idx, score = kc.selftest(case, metric, on_device=1)
    assert rc == 0
    kc.assert_same(idx, score, *kc.reference(case, metric))


@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("case", kc.CASES, ids=kc.IDS)
def test_forced_tiles_equal_the_reference(case, metric):
    for tiles in FORCED:
        rc, idx, score = kc.selftest(case, metric, on_device=1, tiles=tiles)
        assert rc == 0, tiles
        kc.assert_same(idx, score, *kc.reference(case, metric))


def test_bad_tiles_and_bad_input_are_refused_on_the_device_path():
    from pecanpy_amd import _lib

    case = kc.CASES[0]
    for tiles in ((96, 0, 0, 0), (0, 9, 0, 0), (0, 0, 0, 6), (0, 0, 0, 36), (0, 0, 70000, 0)):
        rc, idx, score = kc.selftest(case, "dot", on_device=1, tiles=tiles)
        assert rc == _lib.ERR_INVALID and np.isnan(score).all()
    X = case.X.copy()
    X[0, 3] = np.inf
    bad = kc.Case("inf", np.concatenate([case.X, case.X, X]), rows=np.array([0], dtype=np.uint32))
    rc, idx, score = kc.selftest(bad, "cosine", on_device=1)
    assert rc == _lib.ERR_INVALID and b"row 2 " in _lib.load().pw_last_error() and np.isnan(score).all()
    Q = np.zeros((3, case.X.shape[1]), dtype=np.float32)
    Q[1, 0] = np.nan
    rc, idx, score = kc.selftest(kc.Case("nanq", case.X, queries=Q), "cosine", on_device=1)
    assert rc == _lib.ERR_INVALID and b"query 1 " in _lib.load().pw_last_error() and np.isnan(score).all()
    rc, idx, score = kc.selftest(kc.Case("range", case.X, rows=np.array([0, 1], dtype=np.uint32)), "dot", on_device=1)
    assert rc == _lib.ERR_INVALID and b"row number 1 at position 1" in _lib.load().pw_last_error() and np.isnan(score).all()


@pytest.mark.parametrize("n,dim", [(1, 1), (65, 37), (700, 128), (257, 515)])
def test_norms_equal_numpy_bitwise(n, dim):
    from pecanpy_amd.embed import KnnIndex

    X = np.random.default_rng(n + dim).standard_normal((n, dim)).astype(np.float32)
    with KnnIndex(X) as index:
        got = index.norms().cpu().numpy()
    assert np.array_equal(got.view(np.uint64), knn_ref.norms(X).view(np.uint64))


@pytest.mark.parametrize("case", [c for c in kc.CASES if c.name.startswith(("normal-n700", "ties-n257", "zero-rows"))], ids=repr)
def test_device_pointers_equal_host_pointers(case):
    import torch

    from pecanpy_amd.embed import KnnIndex

    with KnnIndex(torch.from_numpy(case.X).cuda()) as index:
        for metric in kc.METRICS:
            if case.rows is not None:
                idx, score = index.query(rows=torch.from_numpy(case.rows.astype(np.int64)).cuda(), topn=case.topn, metric=metric,
                                         exclude_self=case.exclude_self)
            else:
                idx, score = index.query(vectors=torch.from_numpy(case.queries).cuda(), topn=case.topn, metric=metric)
            assert idx.is_cuda and idx.dtype == torch.int64 and score.is_cuda and score.dtype == torch.float64
            rc, want_idx, want_score = kc.selftest(case, metric, on_device=1)
            assert rc == 0
            kc.assert_same(idx.cpu().numpy(), score.cpu().numpy(), want_idx, want_score)
            kc.assert_same(idx.cpu().numpy(), score.cpu().numpy(), *kc.reference(case, metric))
        st = index.last_stats
        assert st["grid"] >= 1 and st["rows_per_block"] in (64, 128, 256) and st["queries_per_tile"] == kc.QT and st["batches"] == 1


def test_most_similar_has_gensims_shape():
    from pecanpy_amd.embed import KnnIndex

    case = next(c for c in kc.CASES if c.name.startswith("ties-n65"))
    names = [f"v{i}" for i in range(case.X.shape[0])]
    want_idx, want_score = knn_ref.knn_ref(case.X, rows=[1, 5], topn=128)
    with KnnIndex(case.X, node_ids=names) as index:
        one = index.most_similar("v1", topn=128)
        both = index.most_similar(["v1", "v5"], topn=128)
        with pytest.raises(ValueError, match="unknown node ID 'nobody'"):
            index.most_similar("nobody")
    assert len(one) == 64 and one == both[0]                       # the padding is trimmed: 65 rows less the node itself
    assert [name for name, _ in both[1]] == [f"v{i}" for i in want_idx[1] if i >= 0]
    assert [s for _, s in one] == [float(s) for s in want_score[0][:64]]
    with KnnIndex(case.X) as index:                                # no names: row numbers
        assert [i for i, _ in index.most_similar(1, topn=3)] == [int(i) for i in want_idx[0][:3]]


@pytest.fixture(scope="module")
def karate_session_walks():
    from sgns_corpora import karate_walks, on_device

    mat, n = karate_walks(10, 30, seed=2)
    return on_device(mat), n


def test_a_sessions_index_is_a_snapshot(karate_session_walks):
    from pecanpy_amd.embed import SgnsSession

    d_walks, n = karate_session_walks
    rows = np.arange(n)
    with SgnsSession(d_walks, n, dim=16, window=5, epochs=2, seed=3, workers=1) as s:
        s.run(1)
        before = s.vectors().cpu().numpy()
        with s.knn_index() as index:
            first = index.query(rows=rows, topn=5)
            s.run(1)
            after = s.vectors().cpu().numpy()
            assert not np.array_equal(before, after)
            again = index.query(rows=rows, topn=5)
            now = s.most_similar(rows, topn=5)
    want_before = knn_ref.knn_ref(before, rows=rows, topn=5)
    want_after = knn_ref.knn_ref(after, rows=rows, topn=5)
    for got in (first, again):
        kc.assert_same(got[0].cpu().numpy(), got[1].cpu().numpy(), *want_before)
    kc.assert_same(now[0].cpu().numpy(), now[1].cpu().numpy(), *want_after)
    assert not np.array_equal(want_before[1], want_after[1])


def test_against_context_is_the_models_link_score(karate_session_walks):
    from pecanpy_amd.embed import SgnsSession

    d_walks, n = karate_session_walks
    rows = np.array([0, 33, 5, 0])
    with SgnsSession(d_walks, n, dim=16, window=5, epochs=1, seed=3, workers=1) as s:
        s.run(1)
        vec, ctx = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
        idx, score = s.most_similar(rows, topn=n, metric="dot", against="context")
        with pytest.raises(ValueError, match="against"):
            s.most_similar(rows, against="syn2")
    want = knn_ref.knn_ref(ctx, queries=vec[rows], topn=n, metric="dot")
    kc.assert_same(idx.cpu().numpy(), score.cpu().numpy(), *want)
    assert (idx.cpu().numpy() >= 0).all()                        # a vector query: nothing is left out


@pytest.mark.parametrize("ext", [".emb", ".npz"])
def test_cli_task_neighbours(tmp_path, ext):
    from pecanpy_amd import cli
    from pecanpy_amd.embed import save_word2vec_format

    rng = np.random.default_rng(11)
    names = [f"node{i}" for i in range(70)]
    X = kc._plant(rng.standard_normal((70, 12)).astype(np.float32), 70)
    src, out, qfile = tmp_path / ("in" + ext), tmp_path / "out.tsv", tmp_path / "q.txt"
    if ext == ".npz":
        np.savez(src, IDs=names, data=X)
    else:
        save_word2vec_format(src, names, X)
    _, stored = cli.read_init_emb(str(src))                      # (the text format keeps six decimals)

    def text(rows, topn, metric):
        idx, score = knn_ref.knn_ref(stored, rows=rows, topn=topn, metric=metric)
        return "".join("%s\t%s\t%.6f\n" % (names[r], names[i], s) for r, ri, rs in zip(rows, idx, score) for i, s in zip(ri, rs) if i >= 0)

    cli.main(["--input", str(src), "--output", str(out), "--task", "neighbours"])
    assert out.read_text() == text(list(range(70)), 10, "cosine")
    qfile.write_text("node64\nnode1\n\nnode64\n")
    cli.main(["--input", str(src), "--output", str(out), "--task", "neighbours", "--queries", str(qfile), "--topn", "128", "--metric", "dot"])
    assert out.read_text() == text([64, 1, 64], 128, "dot")
    qfile.write_text("node1\nnode70\n")
    with pytest.raises(ValueError, match="unknown node ID 'node70'"):
        cli.main(["--input", str(src), "--output", str(out), "--task", "neighbours", "--queries", str(qfile)])


def test_many_persistent_passes_per_workgroup():
    """n = 200 000: the one shape where a workgroup walks many row blocks per tile, against ``embed.knn_host``."""
    import torch

    from pecanpy_amd.embed import KnnIndex, knn_host

    rng = np.random.default_rng(5)
    X = rng.standard_normal((200000, 128)).astype(np.float32)
    Q = rng.standard_normal((64, 128)).astype(np.float32)
    Q[:8] = X[[0, 63, 64, 4095, 4096, 131071, 199999, 100000]]
    want_idx, want_score = knn_host(X, queries=Q, topn=10)
    with KnnIndex(torch.from_numpy(X).cuda()) as index:
        idx, score = index.query(vectors=Q, topn=10)
        st = index.last_stats
    assert st["grid"] * 2 < 200000 // st["rows_per_block"]       # every workgroup walks more than two row blocks
    kc.assert_same(idx.cpu().numpy(), score.cpu().numpy(), want_idx, want_score)
    assert (idx.cpu().numpy()[:8, 0] == [0, 63, 64, 4095, 4096, 131071, 199999, 100000]).all()
