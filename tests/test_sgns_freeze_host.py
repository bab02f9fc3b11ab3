"""(CPU) Frozen rows and start subsets before a GPU sees them: the lock restatement (tests/sgns_freeze_ref.py) is the session
restatement when nothing is locked and keeps locked rows bit for bit, its cases reach the branches they are for, the loss
tolerance of tests/test_gpu_sgns_freeze.py is what the restatement gives; the job array of ``start_nodes``; every error that is
raised before device work; the command line's flags; the checkpoint of a session without locks; the C ABI."""
import ctypes as C
import os
import re
import sys
import types
import warnings

import numpy as np
import pytest

import sgns_freeze_ref as fr
import sgns_session_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", [sc.PARAMS[3], sc.PARAMS[12]], ids=[sc.IDS[3], sc.IDS[12]])
def test_without_locks_the_restatement_is_the_session_restatement(param):
    want = sc.reference(param)
    s = fr.Session(sc.corpus(), sc.N_NODES, **sc.kw_of(param))
    records = s.run(sc.EPOCHS)
    assert np.array_equal(s.syn0, want["schedule"]["syn0"]) and np.array_equal(s.syn1, want["schedule"]["syn1"])
    assert records == want["schedule"]["records"] and s.state == want["schedule"]["state"]
    s.reschedule(**sc.RESCHEDULE)
    assert s.run(1) == want["rescheduled"]["records"] and np.array_equal(s.syn0, want["rescheduled"]["syn0"])
    assert not any(s.coverage.values())


@pytest.mark.parametrize("param", sc.PARAMS, ids=sc.IDS)
def test_locked_rows_keep_their_bits_and_the_cases_reach_their_branches(param):
    r = fr.reference(param)
    l0, l1 = list(fr.LOCK0), list(fr.LOCK1)
    assert np.array_equal(r["syn0"][l0], r["before0"][l0]) and np.array_equal(r["syn1"][l1], r["before1"][l1])
    free0 = np.setdiff1d(sc.used_ids(), l0)
    free1 = np.setdiff1d(sc.used_ids(), l1)
    assert (r["syn0"][free0] != r["before0"][free0]).any(axis=1).all() and (r["syn1"][free1] != r["before1"][free1]).any(axis=1).all()
    # what is evaluated does not depend on the locks: the counts are the unlocked session's
    plain = sc.reference(param)["schedule"]["records"]
    assert [(x["evaluations"], x["kept_occurrences"], x["trained_pairs"]) for x in r["records"]] == \
        [(x["evaluations"], x["kept_occurrences"], x["trained_pairs"]) for x in plain]
    cov = r["coverage"]
    print(cov)
    assert cov["locked_target_twice_in_group"] >= 1
    assert cov["locked_ctx_free_target"] >= 1 and cov["free_ctx_locked_target"] >= 1
    # ids 17 and 19 occur in no walk; 0-2 are the most frequent ids of the corpus
    assert {17, 19}.isdisjoint(sc.used_ids().tolist())
    mat = sc.corpus()
    valid = np.arange(sc.L + 1)[None, :] < mat[:, -1:].astype(np.int64)
    freq = np.bincount(mat[:, :sc.L + 1][valid], minlength=sc.N_NODES)
    assert set(np.argsort(-freq, kind="stable")[:3].tolist()) == {0, 1, 2}


def test_the_loss_tolerance_is_four_times_the_float32_gap_of_the_locked_run():
    import test_gpu_sgns_freeze as gpu

    g = max(fr.loss_gap(p) for p in sc.PARAMS)
    print(f"g = {g:.3e}, recorded {gpu.LOSS_GAP:.3e}, tol {gpu.LOSS_TOL:.3e}")
    assert gpu.LOSS_TOL == 4 * gpu.LOSS_GAP
    assert gpu.LOSS_GAP / 2 <= g <= gpu.LOSS_GAP * 2      # (NumPy builds differ in the last bit of dot and exp)


# ---- start subsets ---------------------------------------------------------------------------------------------------------------
def ring(n=9, random_state=4):
    from pecanpy_amd import pecanpy as node2vec

    indptr = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    indices = np.array([[(i - 1) % n, (i + 1) % n] for i in range(n)], dtype=np.uint32).ravel()
    return node2vec.SparseOTF.from_csr(indptr, indices, np.ones(2 * n, np.float32), node_ids=[f"v{i}" for i in range(n)],
                                       p=1, q=1, random_state=random_state)


def test_the_job_array_of_a_start_subset_is_the_reference_construction():
    g = ring()
    subset = ["v7", "v0", "v3"]
    idx = g._indices_of(subset, "start_nodes")
    assert idx.dtype == np.uint32 and idx.tolist() == [7, 0, 3]
    want = np.concatenate([np.array([7, 0, 3], dtype=np.uint32)] * 4)
    np.random.seed(4)
    np.random.shuffle(want)
    got = g._start_array(4, start_idx=idx)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(g._starts_for(4, subset), want)
    # None: today's array
    from oracle import pyoracle as orc

    assert np.array_equal(g._starts_for(4, None), orc.shuffled_starts(9, 4, 4))
    assert np.array_equal(g._start_array(4), orc.shuffled_starts(9, 4, 4))
    assert np.array_equal(g._start_array(4, 11), orc.shuffled_starts(9, 4, 11))


@pytest.mark.parametrize("bad, text", [(["v1", "nobody"], "not in the graph"), ([], "empty"), (["v1", "v2", "v1"], "more than once")])
def test_start_nodes_are_checked_before_any_device_work(bad, text, monkeypatch):
    g = ring()
    monkeypatch.setattr(g, "_get_engine", lambda: pytest.fail("device work"))
    monkeypatch.setattr(g, "_call_seed", lambda: pytest.fail("the seed was drawn"))
    for call in (lambda: g.simulate_walks_array(2, 5, start_nodes=bad), lambda: g.simulate_walks(2, 5, start_nodes=bad),
                 lambda: g.simulate_walks_corpus(2, 5, start_nodes=bad), lambda: g.walks_to_file("unused", 2, 5, start_nodes=bad),
                 lambda: g._device_walks(2, 5, start_nodes=bad), lambda: g._session_walks(2, 5, start_nodes=bad)):
        with pytest.raises(ValueError, match=text):
            call()


# ---- extend_session --------------------------------------------------------------------------------------------------------------
def test_extend_session_errors_before_device_work(monkeypatch):
    g = ring()
    monkeypatch.setattr(g, "_get_engine", lambda: pytest.fail("device work"))
    vec = np.zeros((2, 8), np.float32)
    for ids, v, kw, text in ((["v1", "x"], vec, {}, "not in the graph"), (["v1", "v1"], vec, {}, "more than once"),
                             ([f"v{i}" for i in range(9)], np.zeros((9, 8), np.float32), {}, "no new vertex"),
                             (["v1", "v2"], vec.astype(np.float64), {}, "float32"), (["v1", "v2"], vec[:1], {}, "float32"),
                             (["v1", "v2"], vec, dict(context_vectors=np.zeros((2, 7), np.float32)), "dim of vectors"),
                             (["v1", "v2"], vec, dict(starts="some"), "starts"), (["v1", "v2"], vec, dict(holdout_walks=-1), "holdout_walks")):
        with pytest.raises(ValueError, match=text):
            g.extend_session(ids, v, **kw)
    with pytest.raises(TypeError):
        g.extend_session(["v1", "v2"], vec, dim=8)                              # (dim is taken from vectors)


def test_extend_session_has_no_device_matrix_under_the_multi_gpu_routes(monkeypatch):
    g = ring()
    asked = []
    monkeypatch.setattr(g, "_device_walks", lambda num_walks, walk_length, start_nodes=None: asked.append(start_nodes))
    for call in (g.extend_session, g.extend_embedding):
        with pytest.raises(NotImplementedError, match="device"):
            call(["v1", "v2"], np.zeros((2, 8), np.float32), num_walks=2, walk_length=5)
    assert asked == [[f"v{i}" for i in (0, 3, 4, 5, 6, 7, 8)]] * 2             # the new vertices, in the graph's order
    asked.clear()
    with pytest.raises(NotImplementedError, match="device"):
        g.extend_session(["v1", "v2"], np.zeros((2, 8), np.float32), starts="all")
    assert asked == [None]


# ---- SgnsSession with the library mocked ----------------------------------------------------------------------------------------
class FakeLib:
    """The entries ``save`` and ``freeze`` reach, on a session that holds no handle of the real library."""

    def __init__(self, locked=(0, 0)):
        self.locked, self.calls = locked, []

    def pw_sgns_lock_info(self, handle, out):
        out[0], out[1], out[2] = self.locked[0], self.locked[1], 0
        return 0

    def pw_sgns_get_state(self, handle, st):
        st._obj.epoch, st._obj.sched_pos, st._obj.sched_total, st._obj.alpha, st._obj.min_alpha = 1, 1, 3, 0.025, 1e-4
        return 0

    def pw_sgns_set_locks(self, *a):
        self.calls.append(a)
        return 0


def fake_session(monkeypatch, lib):
    import torch

    from pecanpy_amd import _lib, embed

    monkeypatch.setattr(_lib, "load", lambda: lib)
    s = object.__new__(embed.SgnsSession)
    s._handle, s.num_nodes, s.last_stats = C.c_void_p(1), sc.N_NODES, None
    s.params = dict(dim=8, window=3, epochs=3, negative=5, alpha=0.025, min_alpha=1e-4, sample=0.0, seed=7, workers=1, compute_loss=True)
    s.d_walks = torch.from_numpy(sc.corpus().view(np.int32).copy())            # (a host tensor stands in for the device matrix)
    monkeypatch.setattr(embed.SgnsSession, "_matrix", lambda self, which: torch.zeros((sc.N_NODES, 8)))
    monkeypatch.setattr(embed.SgnsSession, "close", lambda self: None)
    return s


def test_the_checkpoint_of_a_session_without_locks_has_no_new_keys(monkeypatch, tmp_path):
    import torch

    from pecanpy_amd import embed

    saved = {}
    monkeypatch.setattr(np, "savez", lambda f, **arrays: saved.update(arrays))
    s = fake_session(monkeypatch, FakeLib())
    s.save(str(tmp_path / "plain.ckpt"))
    assert sorted(saved) == sorted(["vectors", "context_vectors", "corpus_shape"] + ["state_" + k for k in ("epoch", "sched_pos", "sched_total",
                                   "alpha", "min_alpha")] + ["param_" + k for k in s.params])
    saved.clear()
    s = fake_session(monkeypatch, FakeLib(locked=(2, 0)))
    m0 = torch.zeros(sc.N_NODES, dtype=torch.bool)
    m0[[1, 5]] = True
    monkeypatch.setattr(embed.SgnsSession, "frozen", property(lambda self: (m0, torch.zeros_like(m0))))
    s.save(str(tmp_path / "locked.ckpt"))
    assert saved["frozen_vectors"].dtype == bool and np.flatnonzero(saved["frozen_vectors"]).tolist() == [1, 5]
    assert saved["frozen_context"].dtype == bool and not saved["frozen_context"].any()


def test_freeze_checks_its_rows_before_the_library_is_called(monkeypatch):
    import torch

    lib = FakeLib()
    s = fake_session(monkeypatch, lib)
    n = sc.N_NODES
    for bad, text in ((np.zeros(n + 1, dtype=bool), "num_nodes = 20"), (torch.zeros(n - 1, dtype=torch.bool), "num_nodes = 20"),
                      ([0, n], "outside 0..19"), (np.array([n], dtype=np.uint64), "outside 0..19"), (torch.tensor([-1]), "outside 0..19"),
                      (np.array([0.5]), "float"), (torch.zeros(n, dtype=torch.float16), "float"), (["a"], "bool mask or integer"),
                      (torch.zeros(n, dtype=torch.bool, device="meta"), "must be on the host or on")):
        for call in (lambda: s.freeze(bad), lambda: s.freeze([1], context=bad)):
            with pytest.raises(ValueError, match=text):
                call()
    # a tensor on another GPU: a session whose matrix says cuda:1 and a mask that says cuda:0
    class OnCuda0(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))

    s.d_walks = types.SimpleNamespace(device=torch.device("cuda", 1))
    with pytest.raises(ValueError, match="cuda:1, not on cuda:0"):
        s.freeze(torch.zeros(n, dtype=torch.bool).as_subclass(OnCuda0))
    assert lib.calls == []
    s._handle = None
    for use in (lambda: s.freeze([0]), s.unfreeze, lambda: s.frozen):
        with pytest.raises(ValueError, match="closed"):
            use()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from pecanpy_amd import cli

    base = ["--input", "g.edg", "--output", "g.emb"]
    a = cli.parse_args(base)
    assert a.init_emb is None and a.freeze_init is False and a.walks_from == "new"
    a = cli.parse_args(base + ["--init_emb", "old.npz", "--freeze_init", "--walks_from", "all"])
    assert a.init_emb == "old.npz" and a.freeze_init is True and a.walks_from == "all"
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--walks_from", "some"])
    assert {"--init_emb", "--freeze_init", "--walks_from"} <= {flag for flag, _ in cli._OPTIONS}


def test_cli_reads_both_forms_of_an_embedding_file_and_drops_unknown_ids(tmp_path):
    from pecanpy_amd import cli
    from pecanpy_amd.embed import save_word2vec_format

    rng = np.random.default_rng(1)
    ids, vec = ["v2", "ghost", "v5"], (rng.random((3, 4), dtype=np.float32) - 0.5)
    np.savez(tmp_path / "old.npz", IDs=ids, data=vec)
    save_word2vec_format(tmp_path / "old.emb", ids, vec)
    got_ids, got = cli.read_init_emb(str(tmp_path / "old.npz"))
    assert got_ids == ids and got.dtype == np.float32 and np.array_equal(got, vec)
    got_ids, got = cli.read_init_emb(str(tmp_path / "old.emb"))
    assert got_ids == ids and got.dtype == np.float32
    assert np.array_equal(got, np.array([[float("%.6f" % x) for x in row] for row in vec.tolist()], dtype=np.float32))
    (tmp_path / "short.emb").write_text("3 4\nv1 0 0 0 0\n")
    with pytest.raises(ValueError, match="announces 3 rows"):
        cli.read_init_emb(str(tmp_path / "short.emb"))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        known, data = cli._known_vectors(ring(), ids, vec)
    assert known == ["v2", "v5"] and np.array_equal(data, vec[[0, 2]])
    assert [str(w.message) for w in caught] == ["--init_emb: 1 of 3 IDs are not in the graph and are dropped"]


def test_cli_init_flags_warn_and_are_ignored_on_the_other_routes(tmp_path, monkeypatch):
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
    monkeypatch.setattr(cli, "read_graph", lambda args: types.SimpleNamespace(preprocess_transition_probs=lambda: None))
    monkeypatch.setattr(cli, "simulate_walks", lambda args, g: [["a", "b"], ["b", "c"]])
    monkeypatch.setattr(cli, "read_init_emb", lambda path: pytest.fail("the file of an ignored flag was read"))
    argv = ["--input", "unused.edg", "--output", str(tmp_path / "out.npz"), "--dimensions", "4", "--init_emb", "old.npz", "--freeze_init"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        cli.main(argv)
    assert any("--init_emb" in str(w.message) and "gensim" in str(w.message) for w in caught)
    assert len(calls) == 1 and np.load(tmp_path / "out.npz")["data"].shape == (3, 4)
    # --task train has no graph
    from pecanpy_amd import embed

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop("stop here")

    monkeypatch.setattr(embed, "train_sgns_file", stop)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(Stop):
            cli.main(["--input", "walks.txt", "--output", str(tmp_path / "t.emb"), "--task", "train", "--init_emb", "old.npz"])
    assert any("--init_emb" in str(w.message) and "--task train" in str(w.message) for w in caught)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_lock_entries_and_the_library_exports_them():
    from pecanpy_amd import _lib

    text = open(os.path.join(REPO, "include", "pecanpy_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("pw_sgns_set_locks", "pw_sgns_get_locks", "pw_sgns_lock_info"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS, name
    assert "COPIED" in text and "pw_sgns_vectors_set, which replaces a matrix wholesale" in text
    lib = _lib.load()
    out = (C.c_uint64 * 3)()
    for rc in (lib.pw_sgns_set_locks(None, None, None), lib.pw_sgns_get_locks(None, None, None), lib.pw_sgns_lock_info(None, out)):
        assert rc != 0 and b"null pointer" in lib.pw_last_error()


def test_the_unlocked_kernel_instances_keep_the_kernels_four_arguments(tmp_path):
    """The LOCK = false instances are instantiated with the signature the kernel always had; the LOCK instances add the two
    lock arguments; neither uses scratch nor spills a vector register."""
    import shutil
    import subprocess

    from pecanpy_amd import embed

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(os.path.dirname(os.path.abspath(embed.__file__)), "csrc")
    src = tmp_path / "sgns_lock.hip"
    four = "(pw::SgnsArgs, const uint32_t *, const uint32_t *, const float *"
    src.write_text('#include "sgns.hip.h"\n'
                   f"template __global__ void pw::sgns_walk_kernel<2, true, false>{four});\n"
                   f"template __global__ void pw::sgns_walk_kernel<2, false, true>{four}, const uint32_t *, const uint32_t *);\n"
                   f"template __global__ void pw::sgns_walk_kernel<3, true, true>{four}, const uint32_t *, const uint32_t *);\n")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{csrc}",
                          "-c", str(src), "-o", str(tmp_path / "sgns_lock.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:] if "sgns_walk_kernel" in b.split("\n")[0]]
    assert len(blocks) == 3
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0
