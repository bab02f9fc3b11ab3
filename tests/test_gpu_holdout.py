"""Edge hold-out on the GPU: the selftest hook with ``on_device = 1`` -- upload, the kernels of csrc/holdout.hip.h, download --
against the plain-loop statement ``linkpred.holdout_edges_host`` on every case of tests/holdout_cases.py at every word batch,
array for array; ``Base.holdout_edges``: the train graph, its walks, the held-out tensors in ``score_pairs``; ``--task split``
followed by ``--task score`` in a fresh process."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import holdout_cases as hc
from pecanpy_amd import _lib, linkpred

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fraction", hc.FRACTIONS, ids=("thr-0", "thr-half", "thr-max"))
@pytest.mark.parametrize("name", list(hc.graphs()))
def test_kernels_equal_the_statement(name, fraction):
    """Every (protect, first_word) with the default batch; batches of 64 and 100 words -- which cut the flags, the mates of a
    hub row and the stream's blocks of 624 words in many places -- for both protect settings at first_word 0, and at
    first_word 2^33 + 5 with protection."""
    graph = hc.graphs()[name]
    for protect in hc.PROTECTS:
        for first_word in hc.FIRST_WORDS:
            for batch in hc.BATCHES:
                if batch and first_word and not protect:
                    continue
                got = hc.selftest(graph, fraction, protect, first_word, on_device=1, batch=batch)
                assert got.rc == 0, hc.last_error()
                assert hc.equals_statement(got, name, fraction, protect, first_word), (protect, first_word, batch)


def test_a_csr_without_a_mate_is_refused_and_nothing_is_written():
    for batch in (0, 3):   # (3: the offending entry and an earlier, complete one fall into different batches)
        got = hc.selftest(hc.MISSING_MATE, Fraction(1, 2), True, 0, on_device=1, batch=batch)
        assert got.rc == _lib.ERR_INVALID and f"position {hc.MISSING_AT} has no mate".encode() in hc.last_error(), hc.last_error()
        assert got.untouched()
    as_directed = hc.selftest(hc.MISSING_MATE, Fraction(1, 2), True, 0, on_device=1, directed=True)
    train, held, _ = linkpred.holdout_edges_host(*hc.MISSING_MATE[:3], Fraction(1, 2), hc.SEED, directed=True)
    assert as_directed.rc == 0 and hc.same_arrays(as_directed.train, train) and hc.same_arrays(as_directed.held, held)


def _graph(cls, name, **kw):
    indptr, indices, data, _ = hc.graphs()[name]
    g = cls.from_csr(indptr, indices, data, random_state=4, **kw)
    g.device = 0
    return g


@pytest.mark.parametrize("mode", ("SparseOTF", "PreComp"))
def test_base_holdout_edges_gives_the_statements_graph_and_walks(mode):
    import torch

    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.embed import KnnIndex

    cls = getattr(node2vec, mode)
    g = _graph(cls, "er-700", p=0.5, q=2.0)
    g.preprocess_transition_probs()
    before = g.simulate_walks(1, 8)
    train, (u, v, w), used = g.holdout_edges(0.5, seed=hc.SEED)
    (t_indptr, t_indices, t_data), (hu, hv, hw), (units, protected) = hc.statement("er-700", Fraction(1, 2), True, 0)
    # the object: the caller's class and parameters, the statement's arrays, the handle in place
    assert type(train) is cls and (train.p, train.q, train.random_state, train.device) == (0.5, 2.0, 4, 0) and train.nodes == g.nodes
    assert hc.same_arrays((train.indptr, train.indices, train.data), (t_indptr, t_indices, t_data))
    assert train._engine is not None and train._get_engine() is train._engine   # nothing is uploaded again
    assert used == g.indices.size and g.last_holdout_stats["held"] == hu.size
    assert (g.last_holdout_stats["units"], g.last_holdout_stats["protected"]) == (units, protected)
    # the tensors: on the device, what score_pairs takes
    assert u.is_cuda and u.dtype == torch.int64 and v.dtype == torch.int64 and w.dtype == torch.float32
    assert np.array_equal(u.cpu().numpy(), hu) and np.array_equal(v.cpu().numpy(), hv) and hc.same_arrays((w.cpu().numpy(),), (hw,))
    vectors = np.random.default_rng(3).standard_normal((700, 16)).astype(np.float32)
    with KnnIndex(vectors) as index:
        scores = index.score_pairs(u, v, metric="dot")
    assert np.array_equal(scores.cpu().numpy(), linkpred.score_pairs_host(vectors, hu, hv, "dot"))
    # the train graph walks as from_csr of the statement's arrays does, walk for walk
    twin = cls.from_csr(t_indptr, t_indices, t_data, p=0.5, q=2.0, random_state=4)
    twin.device = 0
    train.preprocess_transition_probs()
    twin.preprocess_transition_probs()
    assert train.simulate_walks(2, 12) == twin.simulate_walks(2, 12)
    # the source graph is as it was
    assert g.simulate_walks(1, 8) == before and hc.same_arrays((g.indptr, g.indices), hc.graphs()["er-700"][:2])


def test_directed_unprotected_offsets_and_the_refusals_of_the_python_entry():
    from pecanpy_amd import pecanpy as node2vec

    g = _graph(node2vec.SparseOTF, "directed-700")
    first = hc.FIRST_WORDS[1]
    train, (u, v, w), _ = g.holdout_edges(Fraction(1, 2), seed=hc.SEED, directed=True, protect=False, first_word=first)
    (t_indptr, t_indices, t_data), (hu, hv, hw), _ = hc.statement("directed-700", Fraction(1, 2), False, first)
    assert hc.same_arrays((train.indptr, train.indices, train.data), (t_indptr, t_indices, t_data))
    assert np.array_equal(u.cpu().numpy(), hu) and np.array_equal(v.cpu().numpy(), hv) and hc.same_arrays((w.cpu().numpy(),), (hw,))
    with pytest.raises(ValueError, match="has no mate"):
        g.holdout_edges(0.5, seed=1)   # a directed graph split as an undirected one
    with pytest.raises(ValueError, match="fraction"):
        g.holdout_edges(1.0, seed=1, directed=True)
    dense = node2vec.DenseOTF.from_mat(np.array([[0, 1.0], [1.0, 0]]), ["a", "b"])
    with pytest.raises(NotImplementedError):
        dense.holdout_edges(0.5, seed=1)


def test_cli_split_then_score_in_a_fresh_process(tmp_path):
    """``--task split`` on the karate graph, vectors for its nodes, ``--task score``: the AUC line counts the held-out pairs."""
    indptr, indices, _, _ = hc.graphs()["karate"]
    n = indptr.size - 1
    names = [f"n{i}" for i in range(n)]
    src, train_npz, pairs, negs, emb, out = (tmp_path / x for x in ("karate.npz", "train.npz", "held.tsv", "neg.tsv", "vectors.npz", "scores.tsv"))
    np.savez(src, IDs=names, data=np.ones(indices.size, dtype=np.float32), indptr=indptr, indices=indices)
    np.savez(emb, IDs=names, data=np.random.default_rng(8).standard_normal((n, 8)).astype(np.float32))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "pecanpy_amd.cli"]
    split = subprocess.run(base + ["--input", str(src), "--output", str(train_npz), "--task", "split", "--pairs", str(pairs), "--neg_pairs", str(negs),
                                   "--random_state", str(hc.SEED), "--delimiter", ","], env=env, capture_output=True, text=True, timeout=300)
    assert split.returncode == 0, split.stderr
    (t_indptr, t_indices, t_data), (hu, hv, _), _ = hc.statement("karate", Fraction(1, 2), True, 0)
    with np.load(train_npz) as z:
        assert z["IDs"].tolist() == names and hc.same_arrays((z["indptr"], z["indices"], z["data"]), (t_indptr, t_indices, t_data))
    assert pairs.read_text() == "".join(f"n{a},n{b}\n" for a, b in zip(hu.tolist(), hv.tolist())) and hu.size > 10
    nu, nv, _ = linkpred.sample_non_edges_host(indptr, indices, hu.size, hc.SEED)   # non-edges of the ORIGINAL graph
    assert negs.read_text() == "".join(f"n{a},n{b}\n" for a, b in zip(nu.tolist(), nv.tolist()))
    score = subprocess.run(base + ["--input", str(emb), "--output", str(out), "--task", "score", "--pairs", str(pairs), "--neg_pairs", str(negs),
                                   "--metric", "dot", "--delimiter", ","], env=env, capture_output=True, text=True, timeout=300)
    assert score.returncode == 0, score.stderr
    line = [x for x in score.stdout.splitlines() if not x.startswith("Took ")][-1].split()
    assert len(line) == 5 and int(line[3]) == hu.size and int(line[4]) == hu.size and 0.0 <= float(line[0]) <= 1.0
    assert len(out.read_text().splitlines()) == hu.size
