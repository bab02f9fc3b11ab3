"""Link prediction on the GPU: the selftest hooks with ``on_device = 1`` -- upload, the kernels of csrc/linkpred.hip.h,
download -- against the NumPy statements of pecanpy_amd/linkpred.py on every case of tests/linkpred_cases.py, bit for bit and
integer for integer; the device-pointer entry points against the hooks; a session's link score against ``most_similar``; the
pipeline on the karate graph; ``--task score``."""
import numpy as np
import pytest

import linkpred_cases as lc
from pecanpy_amd import _lib, linkpred

pytestmark = pytest.mark.gpu


# ---- the case lists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", (False, True), ids=("self", "second-matrix"))
@pytest.mark.parametrize("shape", lc.PAIR_SHAPES, ids=lambda s: f"n{s[0]}-d{s[1]}")
def test_pair_scores_kernel_equals_the_statement(shape, second):
    n, dim = shape   # dim 37 and 515 end in a ragged chunk of 5 / 3 columns, m = 1, 63, 65, 1000 in a ragged tile of pairs
    for m in lc.PAIR_MS:
        A, B, u, v = lc.pair_case(n, dim, m, second)
        for metric in lc.METRICS:
            rc, score = lc.score_selftest(A, B, u, v, metric, on_device=1)
            assert rc == 0, lc.last_error()
            assert lc.same_bits(score, lc.score_statement(n, dim, m, second, metric)), (m, metric)


def test_pair_scores_many_tiles_per_wavefront():
    """More tiles than the grid holds wavefronts: every wavefront walks several (m = 300 000 at dim 8)."""
    rng = np.random.default_rng(9)
    A = lc._matrix(rng, 5000, 8)
    u, v = rng.integers(0, 5000, size=(2, 300000)).astype(np.uint32)
    rc, score = lc.score_selftest(A, None, u, v, "cosine", on_device=1)
    assert rc == 0, lc.last_error()
    assert lc.same_bits(score, linkpred.score_pairs_host(A, u, v))


def test_pair_scores_refusals_write_nothing():
    A, B, u, v = lc.pair_case(65, 37, 65, True)   # B has 68 rows
    for which, pos, row, needle in (("u", 40, 65, b"u[40] = 65 is outside the 65 rows"), ("v", 9, 68, b"v[9] = 68 is outside the 68 rows")):
        bu, bv = u.copy(), v.copy()
        (bu if which == "u" else bv)[pos] = row
        (bu if which == "u" else bv)[pos + 5] = 4000000000
        rc, score = lc.score_selftest(A, B, bu, bv, "cosine", on_device=1)
        assert rc == _lib.ERR_INVALID and needle in lc.last_error(), lc.last_error()
        assert np.isnan(score).all()
    rc, score = lc.score_selftest(A, np.ascontiguousarray(B[:, :36]), u, v, "dot", on_device=1)
    assert rc == _lib.ERR_INVALID and b"dim 37 and 36" in lc.last_error() and np.isnan(score).all()


@pytest.mark.parametrize("name", list(lc.auc_cases()))
def test_auc_kernels_equal_the_statement(name):
    pos, neg = lc.auc_cases()[name]
    rc, wins, ties = lc.auc_selftest(pos, neg, on_device=1)
    assert rc == 0, lc.last_error()
    assert (wins, ties) == lc.auc_statement(name)[1:]


def test_auc_refusals_write_nothing():
    pos, neg = (x.copy() for x in lc.auc_cases()["normal-5000x3000"])
    for name, arr, at in (("pos", pos, 4100), ("neg", neg, 2049)):
        arr[at] = np.nan
        arr[at + 2] = np.nan
        rc, wins, ties = lc.auc_selftest(pos, neg, on_device=1)
        assert rc == _lib.ERR_INVALID and f"{name}[{at}] is a NaN".encode() in lc.last_error(), lc.last_error()
        assert (wins, ties) == (0xDEAD, 0xDEAD)
        arr[at] = arr[at + 2] = 0.0
    pos[3] = neg[1] = np.nan
    assert lc.auc_selftest(pos, neg, on_device=1)[0] == _lib.ERR_INVALID and b"pos[3]" in lc.last_error()


@pytest.mark.parametrize("name", list(lc.graphs()))
def test_sampler_kernels_equal_the_statement(name):
    graph = lc.graphs()[name]
    for m in lc.SAMPLE_MS:
        want_u, want_v, want_used = lc.sample_statement(name, 11, 0, m)
        for batch in lc.SAMPLE_BATCHES:   # 64 and 100 cut the answer in many places; the default takes it in one
            rc, u, v, used = lc.sample_selftest(graph, 11, 0, m, on_device=1, batch=batch)
            assert rc == 0, lc.last_error()
            assert np.array_equal(u, want_u) and np.array_equal(v, want_v) and used == want_used, (m, batch)


def test_sampler_continues_on_the_device():
    graph = lc.graphs()["karate"]
    first = 700001   # (not a multiple of the stream's block of 312 candidates)
    _, u, v, used = lc.sample_selftest(graph, 3, first, 300, on_device=0)
    rc1, u1, v1, used1 = lc.sample_selftest(graph, 3, first, 100, on_device=1, batch=64)
    rc2, u2, v2, used2 = lc.sample_selftest(graph, 3, first + used1, 200, on_device=1)
    assert rc1 == 0 and rc2 == 0, lc.last_error()
    assert np.array_equal(u[:100], u1) and np.array_equal(v[:100], v1) and np.array_equal(u[100:], u2) and np.array_equal(v[100:], v2)
    assert used1 + used2 == used


def test_sampler_refusals_write_nothing():
    rc, u, v, used = lc.sample_selftest(lc.COMPLETE_5, 1, 0, 4, on_device=1)
    assert rc == _lib.ERR_INVALID and b"no off-diagonal non-edge" in lc.last_error()
    assert (u == 0xDEADBEEF).all() and (v == 0xDEADBEEF).all() and used == 0xDEAD
    graph = lc.cap_graph(lc.CAP_ARC)
    for batch in (64, 0):
        rc, u, v, used = lc.sample_selftest(graph, lc.CAP_SEED, lc.CAP_FIRST, 1, on_device=1, batch=batch)
        assert rc == _lib.ERR_INVALID and b"4160 candidates examined (the cap) gave 0 of the 1 non-edges" in lc.last_error(), lc.last_error()
        assert u[0] == 0xDEADBEEF and v[0] == 0xDEADBEEF and used == 0xDEAD
    rc, u, v, used = lc.sample_selftest(graph, lc.CAP_SEED, lc.CAP_FIRST - 1, 1, on_device=1)
    assert rc == 0 and (int(u[0]), int(v[0])) == tuple(lc.CAP_ARC) and used == 1


# ---- the device-pointer entry points -----------------------------------------------------------------------------------
def test_device_pointer_entry_points_equal_the_hooks():
    import torch

    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.embed import KnnIndex

    A, B, u, v = lc.pair_case(700, 128, 1000, True)
    with KnnIndex(A) as a, KnnIndex(torch.from_numpy(B).cuda()) as b:
        for metric in lc.METRICS:
            on_gpu = a.score_pairs(torch.from_numpy(u.astype(np.int64)).cuda(), torch.from_numpy(v.astype(np.int32)).cuda(), metric=metric, other=b)
            assert on_gpu.is_cuda and on_gpu.dtype == torch.float64
            assert lc.same_bits(on_gpu.cpu().numpy(), lc.score_selftest(A, B, u, v, metric, on_device=1)[1])
            own = a.score_pairs(u, u[::-1].copy(), metric=metric)   # NumPy row numbers, the index against itself
            assert lc.same_bits(own.cpu().numpy(), lc.score_selftest(A, None, u, u[::-1].copy(), metric, on_device=1)[1])
        assert a.score_pairs(u[:0], v[:0]).shape == (0,)
        with pytest.raises(ValueError, match=r"v\[2\] = 703 is outside the 703 rows"):
            a.score_pairs([0, 1, 2], [0, 1, 703], other=b)
        with pytest.raises(ValueError, match="dim 128 and 37"):
            with KnnIndex(lc.pair_case(65, 37, 1, False)[0]) as c:
                a.score_pairs([0], [0], other=c)

    pos, neg = lc.auc_cases()["seven-values-5000x3000"]
    value, wins, ties = linkpred.auc(torch.from_numpy(pos.copy()).cuda(), neg)   # one on the device, one on the host
    assert (value, wins, ties) == lc.auc_statement("seven-values-5000x3000") and (wins, ties) == lc.auc_selftest(pos, neg, 1)[1:]
    with pytest.raises(ValueError, match=r"neg\[1\] is a NaN"):
        linkpred.auc(pos, np.array([0.0, np.nan]))

    indptr, indices = lc.graphs()["karate"]
    g = node2vec.SparseOTF.from_csr(indptr, indices, None)
    g.device = 0
    d_u, d_v, used = g.sample_non_edges(1000, seed=11)
    want_u, want_v, want_used = lc.sample_statement("karate", 11, 0, 1000)
    assert d_u.is_cuda and d_u.dtype == torch.int64
    assert np.array_equal(d_u.cpu().numpy(), want_u) and np.array_equal(d_v.cpu().numpy(), want_v) and used == want_used
    more_u, more_v, more_used = g.sample_non_edges(64, seed=11, first_candidate=used)
    both = linkpred.sample_non_edges_host(indptr, indices, 1064, 11)
    assert np.array_equal(more_u.cpu().numpy(), both[0][1000:]) and np.array_equal(more_v.cpu().numpy(), both[1][1000:]) and used + more_used == both[2]


# ---- a session's scores and the pipeline -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def karate_session_walks():
    from sgns_corpora import karate_walks, on_device

    mat, n = karate_walks(10, 30, seed=2)
    return on_device(mat), n


def test_session_pair_scores_are_most_similars(karate_session_walks):
    from pecanpy_amd.embed import SgnsSession

    d_walks, n = karate_session_walks
    rows = np.array([0, 33, 5, 0])
    with SgnsSession(d_walks, n, dim=16, window=5, epochs=1, seed=3, workers=1) as s:
        s.run(1)
        for against, metric in (("context", "dot"), ("context", "cosine"), ("vectors", "cosine")):
            idx, score = s.most_similar(rows, topn=5, metric=metric, against=against)
            pairs = s.score_pairs(np.repeat(rows, 5), idx.reshape(-1), metric=metric, against=against)   # idx stays on the device
            assert lc.same_bits(pairs.cpu().numpy(), score.reshape(-1).cpu().numpy()), (against, metric)
        with pytest.raises(ValueError, match="against"):
            s.score_pairs(rows, rows, against="syn2")


def test_link_auc_on_the_karate_graph(karate_session_walks):
    """Train on the graph, its edges as positives, sampled non-edges as negatives: the integers of the host statement."""
    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.embed import KnnIndex, SgnsSession

    d_walks, n = karate_session_walks
    indptr, indices = lc.graphs()["karate"]
    g = node2vec.SparseOTF.from_csr(indptr, indices, None)
    g.device = 0
    eu = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    ev = indices.astype(np.int64)
    nu, nv, _ = g.sample_non_edges(len(eu), seed=5)
    with SgnsSession(d_walks, n, dim=16, window=5, epochs=2, seed=3, workers=1) as s:
        s.run(2)
        vec, ctx = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
        got = linkpred.link_auc(s, (eu, ev), (nu, nv))                                   # dot against the context vectors
        got_cos = linkpred.link_auc(s, np.stack([eu, ev], axis=1), (nu, nv), metric="cosine", against="vectors")
        with KnnIndex(vec) as index:
            got_index = linkpred.link_auc(index, (eu, ev), (nu, nv), metric="cosine")
    hu, hv = nu.cpu().numpy(), nv.cpu().numpy()
    want = linkpred.auc_host(linkpred.score_pairs_host(vec, eu, ev, "dot", other=ctx), linkpred.score_pairs_host(vec, hu, hv, "dot", other=ctx))
    want_cos = linkpred.auc_host(linkpred.score_pairs_host(vec, eu, ev, "cosine"), linkpred.score_pairs_host(vec, hu, hv, "cosine"))
    print("link_auc on karate:", got, got_cos)
    assert got == want and got_cos == want_cos and got_index == want_cos


# ---- the command line --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [".emb", ".npz"])
def test_cli_task_score(tmp_path, ext, capsys):
    from pecanpy_amd import cli
    from pecanpy_amd.embed import save_word2vec_format

    rng = np.random.default_rng(11)
    names = [f"node{i}" for i in range(70)]
    X = lc._matrix(rng, 70, 12)
    src, out, pairs, negs = tmp_path / ("in" + ext), tmp_path / "out.tsv", tmp_path / "pairs.tsv", tmp_path / "neg.tsv"
    if ext == ".npz":
        np.savez(src, IDs=names, data=X)
    else:
        save_word2vec_format(src, names, X)
    _, stored = cli.read_init_emb(str(src))                      # (the text format keeps six decimals)
    u, v = rng.integers(0, 70, size=(2, 130))
    nu, nv = rng.integers(0, 70, size=(2, 67))
    pairs.write_text("".join(f"{names[a]},{names[b]}\n" for a, b in zip(u, v)) + "\n")
    negs.write_text("".join(f"{names[a]},{names[b]}\n" for a, b in zip(nu, nv)))
    for metric in lc.METRICS:
        cli.main(["--input", str(src), "--output", str(out), "--task", "score", "--pairs", str(pairs), "--neg_pairs", str(negs), "--metric", metric,
                  "--delimiter", ","])
        want, want_neg = linkpred.score_pairs_host(stored, u, v, metric), linkpred.score_pairs_host(stored, nu, nv, metric)
        lines = [line.split(",") for line in out.read_text().splitlines()]
        assert [(a, b) for a, b, _ in lines] == [(names[a], names[b]) for a, b in zip(u, v)]
        assert lc.same_bits(np.array([float(s) for _, _, s in lines]), want)
        value, wins, ties = linkpred.auc_host(want, want_neg)
        printed = [line for line in capsys.readouterr().out.splitlines() if not line.startswith("Took ")]   # (the stage timer's line)
        assert printed[-1] == f"{value!r} {wins} {ties} 130 67"
