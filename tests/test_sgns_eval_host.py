"""(CPU) Scoring without training and the change of corpus, before a GPU sees them: the restatement the GPU tests compare with
(tests/sgns_eval_ref.py) scores exactly what its own trainer evaluates and writes nothing, its ``set_walks`` is the constructor's
path; ``SgnsSession.evaluate`` / ``set_walks`` validate their arguments before any device work; the C ABI declares and exports the
two entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sgns_eval_ref as ref
import sgns_session_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(dim=8, window=sc.WINDOW, epochs=2, negative=5, seed=sc.SEED)


def corpus_b():
    """Another corpus of ``sc.corpus()``'s shape and vocabulary, with other frequencies."""
    rng = np.random.default_rng(21)
    mat = np.zeros((sc.N_WALKS, sc.L + 2), dtype=np.uint32)
    mat[:, :sc.L + 1] = np.minimum(rng.geometric(0.3, size=(sc.N_WALKS, sc.L + 1)) - 1, 18)
    mat[:, sc.L + 1] = sc.L + 1
    mat[5, sc.L + 1] = 4
    return mat


def session(walks, **over):
    kw = dict(KW, sample=sc.SAMPLE)
    kw.update(over)
    s = ref.Session(walks, sc.N_NODES, **kw)
    s.syn1[:] = ref.random_context_vectors(sc.N_NODES, kw["dim"])
    return s


@pytest.mark.parametrize("sample", sc.SAMPLES)
@pytest.mark.parametrize("negative", [0, 5, 7])
def test_evaluate_scores_what_a_trainer_that_cannot_move_evaluates(sample, negative):
    """``alpha = min_alpha = 0``: every gradient is zero, the vectors stay, and the trainer's loss of epoch 0 is the loss of
    the vectors as they are -- what ``evaluate(epoch=0)`` returns, to the bit, with the counts."""
    s = session(sc.corpus(), sample=sample, negative=negative, alpha=0.0, min_alpha=0.0)
    syn0, syn1 = s.syn0.copy(), s.syn1.copy()
    before = s.evaluate(epoch=0)
    assert s.evaluate() == before                                   # (epoch=None: state["epoch"], which is 0)
    trained = s.run(1)[0]
    assert np.array_equal(s.syn0, syn0) and np.array_equal(s.syn1, syn1)
    assert before == trained and before["loss"] > 0 and before["evaluations"] > 0
    assert s.evaluate() == s.run(1)[0] != before                    # epoch 1: other hashes


def test_evaluate_writes_nothing():
    s = session(sc.corpus())
    s.run(1)
    syn0, syn1, state = s.syn0.copy(), s.syn1.copy(), dict(s.state)
    own, other = s.evaluate(), s.evaluate(corpus_b()[:7], epoch=3)
    assert np.array_equal(s.syn0, syn0) and np.array_equal(s.syn1, syn1) and s.state == state
    assert own != other and s.evaluate() == own
    # the item base follows the shape of the matrix that is scored
    assert other == session_on_rows(s, corpus_b()[:7]).evaluate(epoch=3)
    assert s.evaluate(sc.corpus(), epoch=1) == own


def session_on_rows(like, walks):
    """A session on ``walks`` carrying ``like``'s vectors and tables: what scoring a foreign matrix must equal."""
    s = session(walks)
    s.syn0, s.syn1, s.table, s.keep = like.syn0, like.syn1, like.table, like.keep
    return s


def test_set_walks_of_the_own_matrix_changes_nothing():
    a, b = session(sc.corpus()), session(sc.corpus())
    a.set_walks(sc.corpus())
    ra, rb = a.run(1), b.run(1)
    a.set_walks(sc.corpus(), recount=True)
    ra += a.run(1)
    rb += b.run(1)
    assert ra == rb and np.array_equal(a.syn0, b.syn0) and np.array_equal(a.syn1, b.syn1) and a.state == b.state


def test_set_walks_with_recount_is_a_fresh_session():
    a, b = session(sc.corpus()), session(corpus_b())
    assert not np.array_equal(a.table, b.table) and not np.array_equal(a.keep, b.keep)
    a.set_walks(corpus_b(), recount=True)
    assert np.array_equal(a.table, b.table) and np.array_equal(a.keep, b.keep)
    assert a.run(2) == b.run(2) and np.array_equal(a.syn0, b.syn0) and np.array_equal(a.syn1, b.syn1)
    # without the recount the tables stay those of the first corpus, and the run differs
    c = session(sc.corpus())
    kept = c.table.copy()
    c.set_walks(corpus_b())
    assert np.array_equal(c.table, kept) and c.rows == b.rows and c.run(2) != session(corpus_b()).run(2)
    with pytest.raises(ValueError):
        c.set_walks(corpus_b()[:5])


# ---- the Python surface, before any device work --------------------------------------------------------------------------------
def _mock_session():
    """A session object with a handle that must never reach the library: every call below fails in Python first."""
    import torch

    from pecanpy_amd.embed import SgnsSession

    s = SgnsSession.__new__(SgnsSession)
    s._handle = object()
    s.d_walks = torch.from_numpy(sc.corpus().view(np.int32).copy())
    s.num_nodes, s.params, s.last_stats = sc.N_NODES, dict(dim=8), None
    return s


def test_evaluate_and_set_walks_check_their_arguments_first():
    import torch

    s = _mock_session()
    host = torch.from_numpy(sc.corpus().view(np.int32).copy())
    try:
        for bad in (sc.corpus(), host, host.to(torch.int64), host.t()):
            with pytest.raises(ValueError, match="contiguous int32 CUDA tensor"):
                s.evaluate(bad)
            with pytest.raises(ValueError, match="contiguous int32 CUDA tensor"):
                s.set_walks(bad)
            with pytest.raises(ValueError, match="contiguous int32 CUDA tensor"):
                s.set_walks(bad, recount=True)
        with pytest.raises(ValueError, match="epoch"):
            s.evaluate(epoch=-1)
        assert s.d_walks.data_ptr() != host.data_ptr()              # a refused matrix is not kept
    finally:
        s._handle = None                                            # (nothing to free)


def test_a_closed_session_scores_and_swaps_nothing():
    s = _mock_session()
    s._handle = None
    for use in (s.evaluate, lambda: s.evaluate(epoch=0), lambda: s.set_walks(s.d_walks)):
        with pytest.raises(ValueError, match="closed"):
            use()


def test_embed_session_with_the_new_arguments_needs_a_device_matrix_too(monkeypatch):
    from pecanpy_amd import pecanpy as node2vec

    g = node2vec.SparseOTF(1, 1, 1, random_state=3)
    monkeypatch.setattr(g, "_device_walks", lambda num_walks, walk_length: None)
    for kw in (dict(fresh_walks=True), dict(holdout_walks=1), dict(fresh_walks=True, holdout_walks=2)):
        with pytest.raises(NotImplementedError, match="device"):
            g.embed_session(8, 2, 5, 3, 1, **kw)
    assert g.random_state == 3                                      # (the call seed of a corpus is put back)
    with pytest.raises(ValueError, match="holdout_walks"):
        g.embed_session(8, 2, 5, 3, 1, holdout_walks=-1)


def test_the_cli_has_the_two_flags():
    from pecanpy_amd import cli

    args = cli.parse_args(["--input", "g.edg", "--output", "g.emb"])
    assert args.fresh_walks is False and args.holdout_walks == 0
    args = cli.parse_args(["--input", "g.edg", "--output", "g.emb", "--fresh_walks", "--holdout_walks", "2"])
    assert args.fresh_walks is True and args.holdout_walks == 2


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_entries_and_the_library_exports_them():
    from pecanpy_amd import _lib

    text = open(os.path.join(REPO, "include", "pecanpy_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("pw_sgns_evaluate", "pw_sgns_set_walks"):
        assert re.search(r"\bint " + name + r"\s*\(pw_sgns \*s, const uint32_t \*d_walks, uint64_t n_walks, uint32_t walk_length,", code), name
        assert name in _lib.SYMBOLS and name in doc, name
    assert re.search(r"PW_SGNS_RECOUNT\s*=\s*1\b", code) and _lib.PW_SGNS_RECOUNT == 1
    assert len(_lib.SYMBOLS["pw_sgns_evaluate"][1]) == 6 and len(_lib.SYMBOLS["pw_sgns_set_walks"][1]) == 5
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "pw_sgns_evaluate") and hasattr(lib, "pw_sgns_set_walks")


def test_the_two_entries_reject_null_handles_without_a_device():
    from pecanpy_amd import _lib

    lib = _lib.load()
    cell = _lib.PwSgnsEpoch()
    assert lib.pw_sgns_evaluate(None, None, 0, 0, 0, C.byref(cell)) != 0 and b"null pointer" in lib.pw_last_error()
    assert lib.pw_sgns_set_walks(None, None, 1, 9, 0) != 0 and b"null pointer" in lib.pw_last_error()
