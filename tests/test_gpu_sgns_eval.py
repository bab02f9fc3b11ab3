"""(GPU) Scoring walks without training and a session's change of corpus (``SgnsSession.evaluate`` / ``set_walks`` over
``pw_sgns_evaluate`` / ``pw_sgns_set_walks``, csrc/sgns.hip.h: ``sgns_eval_kernel``), up to ``Base.embed_session(fresh_walks=...,
holdout_walks=...)`` and the two command-line flags.

The read-only pass writes no vector, so nothing races: its record is held EXACTLY -- to itself at every ``workers``, and to the
pinned one-wavefront trainer, whose epoch loss at ``alpha = min_alpha = 0`` is the loss of the vectors as they are.  Against the
float64 restatement (tests/sgns_eval_ref.py) the counts are exact and the loss is held to the session tests' tolerance
(tests/test_gpu_sgns_session.py: ``LOSS_TOL``, imported, not chosen here).

Corpus A: walks on karate, 2 per node, L = 10; B: the same with another seed; B3: 3 per node (another ``n_walks``)."""
import functools
import struct

import numpy as np
import pytest

import sgns_eval_ref as ref
import sgns_session_cases as sc
from sgns_corpora import karate_walks, on_device
from test_gpu_sgns_session import LOSS_TOL

pytestmark = pytest.mark.gpu

N = 34
L = 10
COUNTS = ("evaluations", "kept_occurrences", "trained_pairs")
KW = dict(dim=65, window=5, epochs=3, negative=5, sample=0.02, seed=7)


@functools.lru_cache(maxsize=None)
def corpus(name):
    num_walks, seed = dict(A=(2, 1), B=(2, 2), B3=(3, 3))[name]
    mat, n = karate_walks(num_walks, L, seed=seed)
    assert n == N and mat.shape == (num_walks * N, L + 2)
    mat = np.ascontiguousarray(mat, dtype=np.uint32)
    mat.setflags(write=False)
    return mat


@functools.lru_cache(maxsize=None)
def matrices(dim, n=N):
    """Seeded random ``(syn0, syn1)`` of trained size: dot products of order one."""
    rng = np.random.default_rng(1000 + dim)
    return tuple((rng.standard_normal((n, dim)) * 0.5).astype(np.float32) for _ in range(2))


@pytest.fixture(scope="module")
def dev():
    return {name: on_device(corpus(name)) for name in ("A", "B", "B3")}


def open_session(d_walks, n=N, load=True, **over):
    from pecanpy_amd.embed import SgnsSession

    kw = dict(KW, workers=1)
    kw.update(over)
    s = SgnsSession(d_walks, n, **kw)
    if load:
        syn0, syn1 = matrices(kw["dim"], n)
        s.load(vectors=syn0, context_vectors=syn1)
    return s


def restated(dtype=np.float64, walks="A", n=N, **over):
    kw = dict(KW)
    kw.update(over)
    s = ref.Session(corpus(walks) if isinstance(walks, str) else walks, n, dtype=dtype, **kw)
    syn0, syn1 = matrices(kw["dim"], n)
    s.syn0[:], s.syn1[:] = syn0, syn1
    return s


@functools.lru_cache(maxsize=None)
def reference():
    """The float64 and the float32 restatement on the loaded matrices: A at epoch 0 and B3 at epoch 2, scored from a session on A."""
    out = {}
    for dtype in (np.float64, np.float32):
        s = restated(dtype)
        out[np.dtype(dtype).name] = dict(A=s.evaluate(epoch=0), B3=s.evaluate(corpus("B3"), epoch=2))
    return out


def bits(record):
    return struct.pack("<d", record["loss"]), tuple(record[k] for k in COUNTS)


def snapshot(s):
    return s.vectors(), s.context_vectors(), s.state


def unchanged(s, snap):
    import torch

    return torch.equal(s.vectors(), snap[0]) and torch.equal(s.context_vectors(), snap[1]) and s.state == snap[2]


def exact_at_every_worker_count(d_walks, n, **over):
    """Check 1: the same record from sessions of 1, the default number of and 3 wavefronts, twice from one, nothing written."""
    records = []
    for workers in (1, 0, 3):
        with open_session(d_walks, n, workers=workers, **over) as s:
            snap = snapshot(s)
            first, second = s.evaluate(), s.evaluate()
            assert bits(first) == bits(second) and set(first) == {"loss", *COUNTS}
            assert unchanged(s, snap)
            records.append(first)
    print(records[0])
    assert bits(records[0]) == bits(records[1]) == bits(records[2])
    assert records[0]["loss"] > 0 and np.isfinite(records[0]["loss"]) and records[0]["evaluations"] > 0
    return records[0]


def test_exact_across_wavefront_counts(dev):
    exact_at_every_worker_count(dev["A"], N)


@pytest.mark.parametrize("negative", [0, 5])
@pytest.mark.parametrize("sample", [0.0, 1e-3], ids=["all", "thinned"])
@pytest.mark.parametrize("dim", [1, 64, 65, 512])
def test_tied_to_the_pinned_trainer(dev, dim, sample, negative):
    """``alpha = min_alpha = 0``: the trainer's vectors cannot move, so the loss of its epoch 0 -- every term taken just before
    an update of zero -- is the loss ``evaluate(epoch=0)`` reports beforehand, bit for bit, with all counts."""
    with open_session(dev["A"], dim=dim, sample=sample, negative=negative, alpha=0.0, min_alpha=0.0, compute_loss=True) as s:
        snap = snapshot(s)
        before = s.evaluate(epoch=0)
        trained = s.run(1)[0]
        assert unchanged(s, (snap[0], snap[1], dict(snap[2], epoch=1, sched_pos=1)))
        print(before, trained)
        assert bits(before) == bits(trained)
        assert before["kept_occurrences"] < int(corpus("A")[:, -1].sum()) if sample else before["kept_occurrences"] == int(corpus("A")[:, -1].sum())
        assert before["evaluations"] > 0 and before["loss"] > 0


def test_counts_and_loss_against_the_restatement(dev):
    """Checks 3 and 4: the counts exactly, on A and on B3 (another ``n_walks``) scored by a session created on A; the loss within
    ``LOSS_TOL`` of the float64 restatement's.  The float32 restatement's own distance is printed beside it."""
    want, want32 = reference()["float64"], reference()["float32"]
    with open_session(dev["A"], workers=0) as s:
        got = dict(A=s.evaluate(epoch=0), B3=s.evaluate(dev["B3"], epoch=2))
    for name in ("A", "B3"):
        g, w = got[name], want[name]
        rel, rel32 = abs(g["loss"] - w["loss"]) / w["loss"], abs(want32[name]["loss"] - w["loss"]) / w["loss"]
        print(f"{name}: loss {g['loss']!r}, want {w['loss']!r}, relative distance {rel:.3e} (float32 restatement {rel32:.3e}), "
              f"tol {LOSS_TOL:.3e}, ratio {rel / LOSS_TOL:.3f}")
        assert tuple(g[k] for k in COUNTS) == tuple(w[k] for k in COUNTS)
    assert got["A"]["evaluations"] != got["B3"]["evaluations"]
    for name in ("A", "B3"):
        assert abs(got[name]["loss"] - want[name]["loss"]) <= LOSS_TOL * want[name]["loss"], (name, got[name], want[name])


def test_set_walks_with_recount_is_a_fresh_session(dev):
    import torch

    with open_session(dev["A"], load=False, compute_loss=True) as swapped, open_session(dev["B"], load=False, compute_loss=True) as fresh:
        swapped.set_walks(dev["B"], recount=True)
        assert swapped.d_walks is dev["B"]
        assert swapped.run(2) == fresh.run(2)
        assert torch.equal(swapped.vectors(), fresh.vectors()) and torch.equal(swapped.context_vectors(), fresh.context_vectors())


def test_set_walks_of_the_own_matrix_changes_nothing(dev):
    import torch

    with open_session(dev["A"], load=False, compute_loss=True) as swapped, open_session(dev["A"], load=False, compute_loss=True) as plain:
        swapped.set_walks(dev["A"])
        ra, rb = swapped.run(1), plain.run(1)
        swapped.set_walks(dev["A"].clone())
        assert ra + swapped.run(1) == rb + plain.run(1)
        assert torch.equal(swapped.vectors(), plain.vectors()) and torch.equal(swapped.context_vectors(), plain.context_vectors())


def test_set_walks_between_epochs_against_the_restatement(dev):
    """A, then B with the tables of A (``recount=False``): the counts of both epochs exactly, both matrices within the
    one-wavefront bound of the float64 restatement doing the same."""
    want = ref.Session(corpus("A"), N, **KW)
    records = want.run(1)
    want.set_walks(corpus("B"))
    records += want.run(1)
    with open_session(dev["A"], load=False, compute_loss=True) as s:
        got = s.run(1)
        s.set_walks(dev["B"])
        got += s.run(1)
        syn0, syn1 = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
    for g, w in zip(got, records):
        print(f"loss {g['loss']!r}, restatement {w['loss']!r}")
    assert [tuple(g[k] for k in COUNTS) for g in got] == [tuple(w[k] for k in COUNTS) for w in records]
    for g, w in ((syn0, want.syn0), (syn1, want.syn1)):
        err, bound = np.abs(g - w).max(), sc.bound(w)
        print(f"max|got - want| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert np.isfinite(g).all() and err <= bound, (err, bound)
    # the tables did stay: a session created on B counts otherwise in its second epoch
    with open_session(dev["B"], load=False) as other:
        assert other.evaluate(epoch=1)["kept_occurrences"] != got[1]["kept_occurrences"]


def test_refusals_change_nothing(dev):
    import torch

    from pecanpy_amd._lib import PwError

    bad_id, bad_len = corpus("B").copy(), corpus("B").copy()
    bad_id[40, 3] = N
    bad_len[17, -1] = L + 2
    with open_session(dev["A"]) as s:
        before, snap = s.evaluate(), snapshot(s)
        for bad in (dev["B3"], on_device(bad_id), on_device(bad_len), dev["B"][:, :-1].contiguous(), dev["B"].cpu()):
            for recount in (False, True):
                with pytest.raises((PwError, ValueError)):
                    s.set_walks(bad, recount=recount)
            assert s.d_walks is dev["A"]
        with pytest.raises(PwError, match="walk 40: node id >= n_nodes"):
            s.evaluate(on_device(bad_id))
        with pytest.raises(PwError, match="walk 17: node id >= n_nodes or length cell > walk_length \\+ 1"):
            s.evaluate(on_device(bad_len))
        with pytest.raises(PwError, match="walk_length must be below 8192"):
            s.evaluate(torch.zeros((1, 8192 + 2), dtype=torch.int32, device="cuda"))
        assert bits(s.evaluate()) == bits(before) and unchanged(s, snap)
        # and the session still trains on A: the first epoch of a session that was never asked
        with open_session(dev["A"]) as plain:
            assert s.run(1) == plain.run(1) and torch.equal(s.vectors(), plain.vectors())


@functools.lru_cache(maxsize=None)
def long_corpus():
    rng = np.random.default_rng(9)
    mat = np.zeros((3, 2048 + 2), dtype=np.uint32)
    mat[:, :2049] = rng.integers(0, 5, size=(3, 2049))
    mat[:, 2049] = (2049, 1500, 2049)
    return mat


def test_long_walks_one_wavefront_per_workgroup():
    """L = 2048: four wavefronts' survivors no longer fit the LDS of a workgroup.  Checks 1 and 3."""
    over = dict(dim=4, window=2, negative=2, sample=0.01)          # (five words of about 1100 occurrences: about a quarter is kept)
    got = exact_at_every_worker_count(on_device(long_corpus()), 5, **over)
    want = restated(walks=long_corpus(), n=5, **over).evaluate(epoch=0)
    print(want)
    assert tuple(got[k] for k in COUNTS) == tuple(want[k] for k in COUNTS)
    assert want["kept_occurrences"] < int(long_corpus()[:, -1].sum())


# ---- graph level and the command line --------------------------------------------------------------------------------------------
GRAPH_KW = dict(dim=16, num_walks=2, walk_length=L, window_size=5, epochs=3, workers=1)


def write_edg(path):
    import os

    from sgns_corpora import GOLDEN

    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    indptr, indices, ids = k["indptr"], k["indices"], k["ids"]
    with open(path, "w") as f:
        for u in range(N):
            for v in indices[indptr[u]:indptr[u + 1]]:
                if u < v:
                    f.write(f"{ids[u]}\t{ids[v]}\n")
    return str(path)


def graph(edg, random_state):
    """The graph object the command line builds from the edge list."""
    from pecanpy_amd import pecanpy as node2vec

    g = node2vec.SparseOTF(1, 0.5, 1, False, False, 0, random_state)
    g.read_edg_device(edg, False, False, "\t")
    return g


@pytest.fixture(scope="module")
def edg(tmp_path_factory):
    return write_edg(tmp_path_factory.mktemp("karate") / "karate.edg")


def hand_driven(edg, fresh, holdout):
    """Three epochs of a plain session, its corpus swapped by hand for that of the graphs seeded 4 and 5, the seed-2 matrix
    scored by hand after every epoch."""
    from pecanpy_amd.embed import SgnsSession

    kw = {k: v for k, v in GRAPH_KW.items() if k not in ("num_walks", "walk_length", "window_size")}
    walks = [graph(edg, r)._device_walks(GRAPH_KW["num_walks"], L) for r in (3, 4, 5)]
    held = graph(edg, 2)._device_walks(1, L)
    records = []
    s = SgnsSession(walks[0], N, window=GRAPH_KW["window_size"], seed=3, compute_loss=True, **kw)
    for e in range(3):
        if fresh and e:
            s.set_walks(walks[e])
        r = s.run(1)[0]
        if holdout:
            h = s.evaluate(held, epoch=0)
            r["holdout_loss"], r["holdout_evaluations"] = h["loss"], h["evaluations"]
        records.append(r)
    return s, records


def test_graph_level_fresh_and_held_out_walks(edg):
    import torch

    from pecanpy_amd.embed import SgnsSession
    from pecanpy_amd.pecanpy import GraphSgnsSession

    g = graph(edg, 3)
    with g.embed_session(compute_loss=True, **GRAPH_KW) as plain:
        assert type(plain) is SgnsSession
    with g.embed_session(compute_loss=True, fresh_walks=True, **GRAPH_KW) as s:
        got = s.run(3)
        want_s, want = hand_driven(edg, True, False)
        with want_s:
            assert isinstance(s, GraphSgnsSession) and got == want
            assert torch.equal(s.vectors(), want_s.vectors()) and torch.equal(s.context_vectors(), want_s.context_vectors())
    with g.embed_session(compute_loss=True, holdout_walks=1, **GRAPH_KW) as s:
        got = s.run(1) + s.run(2)
        want_s, want = hand_driven(edg, False, True)
        with want_s:
            print([(r["holdout_loss"], r["holdout_evaluations"]) for r in got])
            assert len({r["holdout_evaluations"] for r in got}) == 1 and got[0]["holdout_evaluations"] > 0
            assert [bits(dict(r, loss=r["holdout_loss"])) for r in got] == [bits(dict(r, loss=r["holdout_loss"])) for r in want]
            assert got == want and torch.equal(s.vectors(), want_s.vectors())
            assert len({r["holdout_loss"] for r in got}) == 3        # the vectors moved between the three scorings
        with pytest.raises(ValueError, match="0 of 3 epochs left"):
            s.run(1)
    assert g.random_state == 3


def test_cli_fresh_and_held_out_walks(edg, tmp_path, capsys):
    """``--fresh_walks --holdout_walks 1 --epoch_loss --workers 1 --random_state 3``: three epoch lines with a held-out mean,
    and the vectors of the session ``embed_session(fresh_walks=True, holdout_walks=1)`` of the same graph."""
    from pecanpy_amd import cli

    out = str(tmp_path / "karate.npz")
    capsys.readouterr()
    cli.main(["--input", edg, "--output", out, "--mode", "SparseOTF", "--p", "1", "--q", "0.5", "--dimensions", str(GRAPH_KW["dim"]),
              "--num-walks", "2", "--walk-length", str(L), "--window-size", "5", "--epochs", "3", "--workers", "1", "--random_state", "3",
              "--epoch_loss", "--fresh_walks", "--holdout_walks", "1"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch ")]
    g = graph(edg, 3)
    with g.embed_session(compute_loss=True, fresh_walks=True, holdout_walks=1, **GRAPH_KW) as s:
        records = s.run(3)
        vectors = s.vectors().cpu().numpy()
    assert len(lines) == 3 and [ln.split(":")[0] for ln in lines] == ["epoch 1", "epoch 2", "epoch 3"]
    for ln, r in zip(lines, records):
        print(ln)
        mean = float(ln.split("held-out mean ")[1].split(" ")[0])
        assert mean == pytest.approx(r["holdout_loss"] / r["holdout_evaluations"], abs=1e-6) and mean > 0
        assert int(ln.split()[-2]) == r["holdout_evaluations"]
        assert float(ln.split("loss ")[1].split(",")[0]) == pytest.approx(r["loss"], abs=1e-6)
    z = np.load(out)
    assert [str(x) for x in z["IDs"]] == [str(x) for x in g.nodes]
    assert np.array_equal(z["data"], vectors)


def test_cli_flags_keep_the_gensim_route_and_warn(edg, tmp_path, capsys, monkeypatch):
    """With gensim importable the command does what it does without the flags, and says so."""
    import sys
    import types
    import warnings

    from pecanpy_amd import cli

    calls = []

    class Word2Vec:
        def __init__(self, walks, **kw):
            calls.append(kw)
            names = sorted({x for w in walks for x in w})
            self.wv = types.SimpleNamespace(index_to_key=names, vectors=np.zeros((len(names), kw["vector_size"]), np.float32))

    gensim = types.ModuleType("gensim")
    gensim.models = types.ModuleType("gensim.models")
    gensim.models.Word2Vec = Word2Vec
    monkeypatch.setitem(sys.modules, "gensim", gensim)
    monkeypatch.setitem(sys.modules, "gensim.models", gensim.models)
    out = tmp_path / "karate.npz"
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        cli.main(["--input", edg, "--output", str(out), "--mode", "SparseOTF", "--p", "1", "--q", "0.5", "--dimensions", "4",
                  "--num-walks", "2", "--walk-length", "5", "--random_state", "1", "--fresh_walks", "--holdout_walks", "1"])
    assert any("--fresh_walks and --holdout_walks" in str(w.message) and "gensim" in str(w.message) for w in caught)
    assert len(calls) == 1 and "epoch 1:" not in capsys.readouterr().out
    assert np.load(out)["data"].shape == (N, 4)
