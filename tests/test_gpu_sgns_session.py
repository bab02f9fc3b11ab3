"""(GPU) The skip-gram trainer as a session (``pecanpy_amd.embed.SgnsSession`` over ``pw_sgns``): slices of a schedule compose,
a checkpoint continues a run, the loss flag leaves the update alone, the loss and both matrices are the restatement's
(tests/sgns_session_ref.py), the parallel form and a new schedule, the errors, and ``pecanpy --epoch_loss``.

Everything "equal" is ``torch.equal`` / ``==`` at ``workers=1``: every random choice is a hash of (seed, epoch, walk, position),
the learning rate a function of the schedule position, and the epoch loss a sum in an order fixed by the number of walks.
The corpus and the parameter sets: tests/sgns_session_cases.py."""
import os
import sys
import types
import warnings

import numpy as np
import pytest

import sgns_session_cases as sc

pytestmark = pytest.mark.gpu

# The loss tolerance.  g = the largest relative distance between the epoch losses of the float32 and the float64 restatement
# over the 16 cases, four epochs each (tests/test_sgns_session_host.py recomputes it; MEASUREMENTS.md, "Skip-gram sessions"):
# 1.06e-8, at dim64-neg7-all.  The bound is 4 g: the factor covers the kernel's lane-order float32 sums, which the NumPy
# restatement does not model.
LOSS_GAP = 1.0582545362895505e-08
LOSS_TOL = 4 * LOSS_GAP   # 4.233e-08
# The restatement's own fall of the mean loss per evaluation, first epoch to last, on the two-clique corpus (float64: 0.431790 ->
# 0.345845; its float32 run differs by 4e-9): a racing run must show half of it.
CLIQUE_FALL = 0.08594474598232865
CLIQUE_REQUIRED = CLIQUE_FALL / 2

COUNTS = ("kept_occurrences", "trained_pairs", "evaluations")


@pytest.fixture(scope="module")
def d_walks():
    from sgns_corpora import on_device

    return on_device(sc.corpus())


def open_session(d_walks, param, **over):
    from pecanpy_amd.embed import SgnsSession

    kw = dict(sc.kw_of(param), workers=1, compute_loss=True)
    kw.update(over)
    return SgnsSession(d_walks, sc.N_NODES, **kw)


def losses(records):
    return [r["loss"] for r in records]


def counts(records):
    return [tuple(r[k] for k in COUNTS) for r in records]


def close_to(got, want):
    err, bound = np.abs(got - want).max(), sc.bound(want)
    print(f"max|got - want| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("param", sc.PARAMS, ids=sc.IDS)
def test_slices_compose(d_walks, param):
    import torch

    from pecanpy_amd.embed import train_sgns_device

    with open_session(d_walks, param) as a, open_session(d_walks, param) as b:
        ra = a.run(1) + a.run(1) + a.run(1)
        rb = b.run(3)
        assert a.state == b.state and a.state["epoch"] == a.state["sched_pos"] == a.state["sched_total"] == 3
        one_shot = train_sgns_device(d_walks, sc.N_NODES, workers=1, **sc.kw_of(param))
        assert torch.equal(a.vectors(), b.vectors()) and torch.equal(a.vectors(), one_shot)
        assert torch.equal(a.context_vectors(), b.context_vectors())
        assert counts(ra) == counts(rb)
        assert losses(ra) == losses(rb) and all(type(x) is float and x > 0 for x in losses(ra))
        st = train_sgns_device.last_stats
        assert (st["kept_occurrences"], st["trained_pairs"]) == tuple(sum(r[k] for r in rb) for k in COUNTS[:2])
        assert b.last_stats["wavefronts"] == 1


@pytest.mark.parametrize("param", sc.PARAMS, ids=sc.IDS)
def test_a_checkpoint_continues_the_run(d_walks, param, tmp_path):
    import torch

    from pecanpy_amd.embed import SgnsSession

    path = str(tmp_path / "session.ckpt")
    with open_session(d_walks, param) as whole:
        want = whole.run(3)
        with open_session(d_walks, param) as first:
            assert first.run(1) == want[:1]
            first.save(path)
        assert os.path.exists(path) and not os.path.exists(path + ".npz")
        with SgnsSession.restore(path, d_walks) as second:
            assert second.params == whole.params and second.state["epoch"] == 1 and second.state["sched_pos"] == 1
            got = second.run(2)
            assert losses(got) == losses(want[1:]) and counts(got) == counts(want[1:])
            assert torch.equal(second.vectors(), whole.vectors())
            assert torch.equal(second.context_vectors(), whole.context_vectors())
            assert second.state == whole.state


@pytest.mark.parametrize("param", sc.PARAMS, ids=sc.IDS)
def test_the_loss_flag_does_not_touch_the_update(d_walks, param):
    import torch

    with open_session(d_walks, param) as on, open_session(d_walks, param, compute_loss=False) as off:
        r_on, r_off = on.run(3), off.run(3)
        assert torch.equal(on.vectors(), off.vectors()) and torch.equal(on.context_vectors(), off.context_vectors())
        assert [c[:2] for c in counts(r_on)] == [c[:2] for c in counts(r_off)]
        assert all(r["loss"] == 0.0 and r["evaluations"] == 0 for r in r_off)


@pytest.mark.parametrize("param", sc.PARAMS, ids=sc.IDS)
def test_loss_and_matrices_against_the_restatement(d_walks, param):
    """Tests 4 and 7 of the session: the epoch losses within ``LOSS_TOL`` of the float64 restatement's, the counts exactly, both
    matrices within the one-wavefront bound; ``syn1`` rows of nodes that were never a target are exactly zero."""
    want = sc.reference(param)["schedule"]
    with open_session(d_walks, param) as s:
        got = s.run(3)
        syn0, syn1 = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
    for g, w in zip(got, want["records"]):
        rel = abs(g["loss"] - w["loss"]) / w["loss"]
        print(f"loss {g['loss']!r}, want {w['loss']!r}, relative distance {rel:.3e}, tol {LOSS_TOL:.3e}, ratio {rel / LOSS_TOL:.3f}")
    assert counts(got) == counts(want["records"])
    close_to(syn0, want["syn0"])
    close_to(syn1, want["syn1"])
    never = np.setdiff1d(np.arange(sc.N_NODES), sc.used_ids())
    assert never.size >= 3 and not syn1[never].any() and syn1[sc.used_ids()].any(axis=1).all()
    for g, w in zip(got, want["records"]):
        assert abs(g["loss"] - w["loss"]) <= LOSS_TOL * w["loss"], (g["loss"], w["loss"])


@pytest.mark.parametrize("case_id", ["two-workgroups", "three-ballot-words"])
def test_the_parallel_form_without_a_tolerance(case_id):
    """A component per wavefront and ``negative=0``: no two wavefronts share a row, the per-walk loss values are those of
    ``workers=1``, and the reduction depends on nothing else -- equal matrices and equal epoch losses."""
    import torch

    from pecanpy_amd.embed import SgnsSession
    from sgns_corpora import WAVE_CASES, case_corpus, case_kw, on_device

    case = next(c for c in WAVE_CASES if c["id"] == case_id)
    mat, n = case_corpus(case)
    d = on_device(mat)
    kw = case_kw(case)
    with SgnsSession(d, n, workers=case["workers"], compute_loss=True, **kw) as par, \
            SgnsSession(d, n, workers=1, compute_loss=True, **kw) as one:
        rp, r1 = par.run(case["epochs"]), one.run(case["epochs"])
        assert par.last_stats["wavefronts"] == case["wavefronts"] >= 8 and one.last_stats["wavefronts"] == 1   # two workgroups of four
        assert torch.equal(par.vectors(), one.vectors()) and torch.equal(par.context_vectors(), one.context_vectors())
        assert losses(rp) == losses(r1) and counts(rp) == counts(r1)
        assert all(x > 0 for x in losses(rp))


@pytest.mark.parametrize("param", sc.PARAMS, ids=sc.IDS)
def test_a_new_schedule_on_the_trained_vectors(d_walks, param):
    want = sc.reference(param)["rescheduled"]
    with open_session(d_walks, param) as s:
        s.run(3)
        with pytest.raises(ValueError, match="0 of 3 epochs left"):
            s.run(1)
        s.reschedule(**sc.RESCHEDULE)
        got = s.run(1)
        st = s.state
        syn0, syn1 = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
    assert st["epoch"] == 4 and st["sched_pos"] == st["sched_total"] == 1
    assert st["alpha"] == st["min_alpha"] == float(np.float32(0.01))
    assert counts(got) == counts(want["records"])                  # the hashes of epoch 3
    close_to(syn0, want["syn0"])
    close_to(syn1, want["syn1"])
    w = want["records"][0]["loss"]
    assert abs(got[0]["loss"] - w) <= LOSS_TOL * w, (got[0]["loss"], w)


def test_a_racing_runs_loss_falls():
    from pecanpy_amd.embed import SgnsSession
    from sgns_corpora import on_device

    with SgnsSession(on_device(sc.clique_corpus()), sc.CLIQUE_NODES, workers=0, compute_loss=True, **sc.CLIQUE_KW) as s:
        records = s.run(4)
        waves = s.last_stats["wavefronts"]
    mean = [r["loss"] / r["evaluations"] for r in records]
    print(f"{waves} wavefronts, mean loss per epoch {mean}, fall {mean[0] - mean[-1]:.6f}, required {CLIQUE_REQUIRED:.6f}")
    assert waves > 1
    assert mean[0] - mean[-1] >= CLIQUE_REQUIRED


def test_errors(d_walks):
    import torch

    param = sc.PARAMS[0]
    dim = param[0]
    s = open_session(d_walks, param)
    with pytest.raises(ValueError, match="3 of 3 epochs left, 4 asked for"):
        s.run(4)
    assert s.state["epoch"] == 0                                   # (checked before any launch)
    before = s.vectors()
    good = torch.zeros((sc.N_NODES, dim), dtype=torch.float32)
    for bad in (torch.zeros((sc.N_NODES, dim + 1)), torch.zeros((sc.N_NODES + 1, dim)), np.zeros((sc.N_NODES, dim), np.float64),
                good.to(torch.float16).cuda(), torch.zeros((sc.N_NODES, dim), device="meta")):
        for name in ("vectors", "context_vectors"):
            with pytest.raises(ValueError, match=name):
                s.load(**{name: bad})
    with pytest.raises(ValueError, match="context_vectors"):      # nothing is written when one of the two is wrong
        s.load(vectors=good, context_vectors=good[:, :-1])
    assert torch.equal(s.vectors(), before)
    s.load(vectors=good.numpy(), context_vectors=good.cuda() + 1)  # a host array and a device tensor
    assert torch.equal(s.vectors(), good.cuda()) and torch.equal(s.context_vectors(), good.cuda() + 1)
    s.close()
    s.close()
    for use in (lambda: s.run(1), s.vectors, s.context_vectors, lambda: s.state, lambda: s.load(vectors=good),
                lambda: s.reschedule(1), lambda: s.save("unused")):
        with pytest.raises(ValueError, match="closed"):
            use()
    from pecanpy_amd import _lib
    from pecanpy_amd.embed import SgnsSession

    with pytest.raises(_lib.PwError, match="node id >= n_nodes"):  # the one-shot trainer's check, the same text
        SgnsSession(d_walks, 5, dim=8)


def _write_corpus(path):
    mat = sc.corpus()
    with open(path, "w") as f:
        for row in mat:
            f.write(" ".join(f"n{x}" for x in row[:row[-1]]) + "\n")


def test_cli_epoch_loss_on_a_corpus_file(tmp_path, capsys):
    """``--task train --epoch_loss --workers 1``: one line per epoch, and the file that the route of the command without the
    flag -- ``train_sgns_file`` and the device writer -- writes with ``workers=1``.  (The command without the flag does what
    it always did: it does not forward ``--workers``, so its trainer is the racing one and its bytes are not a function of
    the seed; it is run here for what it must still do -- write a file of the same shape and print no loss.)"""
    from pecanpy_amd import cli
    from pecanpy_amd.embed import save_word2vec_format_device, train_sgns_file

    walks = str(tmp_path / "walks.txt")
    _write_corpus(walks)
    out = {k: str(tmp_path / f"{k}.emb") for k in ("flag", "plain", "api")}
    common = ["--input", walks, "--task", "train", "--dimensions", "8", "--window-size", "3", "--epochs", "3", "--workers", "1",
              "--random_state", "7"]
    capsys.readouterr()
    cli.main(common + ["--output", out["flag"], "--epoch_loss"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch ")]
    cli.main(common + ["--output", out["plain"]])
    assert not [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch ")]
    names, d_vectors = train_sgns_file(walks, dim=8, window=3, epochs=3, seed=7, workers=1)
    save_word2vec_format_device(out["api"], names, d_vectors)
    assert len(lines) == 3 and [ln.split(":")[0] for ln in lines] == ["epoch 1", "epoch 2", "epoch 3"]
    for ln in lines:
        loss, mean, evaluations = float(ln.split("loss ")[1].split(",")[0]), float(ln.split("mean ")[1].split(" ")[0]), int(ln.split()[-2])
        assert loss > 0 and evaluations > 0 and mean == pytest.approx(loss / evaluations, abs=1e-6)
    data = {k: open(v, "rb").read() for k, v in out.items()}
    assert data["flag"].startswith(b"15 8\n")
    assert data["flag"] == data["api"]
    assert data["plain"].startswith(b"15 8\n") and len(data["plain"].split(b"\n")) == len(data["flag"].split(b"\n"))
    assert [ln.split(b" ")[0] for ln in data["plain"].split(b"\n")] == [ln.split(b" ")[0] for ln in data["flag"].split(b"\n")]


def test_cli_epoch_loss_keeps_the_gensim_route_and_warns(tmp_path, capsys, monkeypatch):
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
    edg = tmp_path / "ring.edg"
    edg.write_text("".join(f"{i}\t{(i + 1) % 6}\n" for i in range(6)))
    argv = ["--input", str(edg), "--output", str(tmp_path / "ring.npz"), "--dimensions", "4", "--num-walks", "2", "--walk-length", "5",
            "--mode", "FirstOrderUnweighted", "--random_state", "1", "--epoch_loss"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        cli.main(argv)
    assert any("--epoch_loss" in str(w.message) and "gensim" in str(w.message) for w in caught)
    assert len(calls) == 1 and calls[0]["sg"] == 1
    assert "epoch 1:" not in capsys.readouterr().out
    assert np.load(tmp_path / "ring.npz")["data"].shape == (6, 4)
