"""(GPU) Frozen rows in a skip-gram session (``SgnsSession.freeze`` over ``pw_sgns_set_locks``; csrc/sgns.hip.h, the LOCK
instances of ``sgns_walk_kernel``), walks from chosen start vertices (``start_nodes``) and the two together:
``Base.extend_session`` / ``extend_embedding`` and ``pecanpy --init_emb``.

Everything "equal" is bitwise (``torch.equal`` on the values or on their int32 views) at ``workers=1``.  The corpus, the parameter
sets and the lock sets: tests/sgns_session_cases.py, tests/sgns_freeze_ref.py."""
import os
import warnings

import numpy as np
import pytest

import sgns_freeze_ref as fr
import sgns_session_cases as sc

pytestmark = pytest.mark.gpu

# The loss tolerance, derived as tests/test_gpu_sgns_session.py derives LOSS_TOL: g = the largest relative distance between the
# epoch losses of the float32 and the float64 LOCK restatement over the 16 cases, three epochs each
# (tests/test_sgns_freeze_host.py recomputes it): 2.51e-10, at dim8-neg7-all.  The bound is 4 g.
LOSS_GAP = 2.5100307454582957e-10
LOSS_TOL = 4 * LOSS_GAP   # 1.004e-09

COUNTS = ("kept_occurrences", "trained_pairs", "evaluations")
LOCK0, LOCK1 = list(fr.LOCK0), list(fr.LOCK1)


@pytest.fixture(scope="module")
def d_walks():
    from sgns_corpora import on_device

    return on_device(sc.corpus())


def open_session(d_walks, param, **over):
    from pecanpy_amd.embed import SgnsSession

    kw = dict(sc.kw_of(param), workers=1, compute_loss=True)
    kw.update(over)
    return SgnsSession(d_walks, sc.N_NODES, **kw)


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def counts(records):
    return [tuple(r[k] for k in COUNTS) for r in records]


def close_to(got, want):
    err, bound = np.abs(got - want).max(), sc.bound(want)
    print(f"max|got - want| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= bound, (err, bound)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute_loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("workers", [1, 0], ids=["one-wavefront", "racing"])
@pytest.mark.parametrize("param", [sc.PARAMS[0], sc.PARAMS[7], sc.PARAMS[10], sc.PARAMS[13]], ids=[sc.IDS[i] for i in (0, 7, 10, 13)])
def test_frozen_rows_keep_their_bits(d_walks, param, workers, compute_loss):
    import torch

    with open_session(d_walks, param, workers=workers, compute_loss=compute_loss) as s:
        s.load(context_vectors=torch.full((sc.N_NODES, param[0]), 0.01))       # (a frozen syn1 row that is not zero)
        before0, before1 = s.vectors(), s.context_vectors()
        s.freeze(LOCK0, context=LOCK1)
        s.run(sc.EPOCHS)
        after0, after1 = s.vectors(), s.context_vectors()
        assert s.last_stats["lock_instances"] is True
    assert torch.equal(bits(after0[LOCK0]), bits(before0[LOCK0]))
    assert torch.equal(bits(after1[LOCK1]), bits(before1[LOCK1]))
    used = torch.from_numpy(sc.used_ids().astype(np.int64)).cuda()
    free0 = used[~torch.isin(used, torch.tensor(LOCK0).cuda())]
    free1 = used[~torch.isin(used, torch.tensor(LOCK1).cuda())]
    assert (after0[free0] != before0[free0]).any(dim=1).any() and (after1[free1] != before1[free1]).any(dim=1).any()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", sc.PARAMS, ids=sc.IDS)
def test_against_the_lock_restatement(d_walks, param):
    """Both matrices within the one-wavefront bound of the float64 lock restatement, the counts exactly, every epoch's loss
    within ``LOSS_TOL``; the locked rows are exactly what they were."""
    want = fr.reference(param)
    with open_session(d_walks, param) as s:
        s.freeze(LOCK0, context=LOCK1)
        got = s.run(sc.EPOCHS)
        syn0, syn1 = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
    for g, w in zip(got, want["records"]):
        rel = abs(g["loss"] - w["loss"]) / w["loss"]
        print(f"loss {g['loss']!r}, want {w['loss']!r}, relative distance {rel:.3e}, tol {LOSS_TOL:.3e}, ratio {rel / LOSS_TOL:.3f}")
    assert counts(got) == counts(want["records"])
    close_to(syn0, want["syn0"])
    close_to(syn1, want["syn1"])
    assert np.array_equal(syn0[LOCK0], want["before0"][LOCK0].astype(np.float32)) and not syn1[LOCK1].any()
    for g, w in zip(got, want["records"]):
        assert abs(g["loss"] - w["loss"]) <= LOSS_TOL * w["loss"], (g["loss"], w["loss"])


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workers", [1, 0], ids=["one-wavefront", "racing"])
@pytest.mark.parametrize("param", [sc.PARAMS[1], sc.PARAMS[6], sc.PARAMS[11], sc.PARAMS[12]], ids=[sc.IDS[i] for i in (1, 6, 11, 12)])
def test_everything_frozen_is_the_read_only_kernel(d_walks, param, workers):
    """Both matrices frozen completely: an epoch of ``run`` evaluates what ``evaluate`` evaluates, in its order -- the same
    record, the loss bit for bit -- and writes nothing."""
    import torch

    with open_session(d_walks, param, workers=workers) as warm, open_session(d_walks, param, workers=workers) as s:
        warm.run(1)                                                             # (vectors with a trained syn1, not zeros)
        s.load(vectors=warm.vectors(), context_vectors=warm.context_vectors())
        s.freeze(torch.ones(sc.N_NODES, dtype=torch.bool))
        before0, before1 = s.vectors(), s.context_vectors()
        for e in range(2):
            scored = s.evaluate(epoch=e)
            trained = s.run(1)[0]
            assert trained == scored and trained["loss"] > 0 and trained["evaluations"] > 0
            assert s.state["epoch"] == s.state["sched_pos"] == e + 1
        assert torch.equal(bits(s.vectors()), bits(before0)) and torch.equal(bits(s.context_vectors()), bits(before1))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", [sc.PARAMS[3], sc.PARAMS[8]], ids=[sc.IDS[3], sc.IDS[8]])
def test_nothing_frozen_is_the_kernel_without_locks(d_walks, param):
    import torch

    with open_session(d_walks, param) as plain, open_session(d_walks, param) as thawed, open_session(d_walks, param) as empty:
        thawed.freeze(LOCK0, context=LOCK1)
        thawed.unfreeze()
        empty.freeze(np.zeros(sc.N_NODES, dtype=bool))
        want = plain.run(sc.EPOCHS)
        assert plain.last_stats["lock_instances"] is False
        for s in (thawed, empty):
            assert not s.frozen[0].any() and not s.frozen[1].any() and s._lock_info()[:2] == (0, 0)
            assert s.run(sc.EPOCHS) == want
            assert s.last_stats["lock_instances"] is False
            assert {k: v for k, v in s.last_stats.items() if k in ("kept_occurrences", "trained_pairs", "wavefronts")} == \
                {k: v for k, v in plain.last_stats.items() if k in ("kept_occurrences", "trained_pairs", "wavefronts")}
            assert torch.equal(s.vectors(), plain.vectors()) and torch.equal(s.context_vectors(), plain.context_vectors())


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["round-up-to-a-workgroup", "two-workgroups", "three-ballot-words", "many-walks-per-wavefront"])
def test_the_parallel_form_without_a_tolerance(case_id):
    """A component per wavefront and ``negative=0``: no two wavefronts share a row, so with a lock set that hits every component
    the vectors equal those of ``workers=1`` bit for bit."""
    import torch

    from pecanpy_amd.embed import SgnsSession
    from sgns_corpora import WAVE_CASES, case_corpus, case_kw, on_device

    case = next(c for c in WAVE_CASES if c["id"] == case_id)
    mat, n = case_corpus(case)
    d = on_device(mat)
    kw = case_kw(case)
    lock0 = np.arange(0, n, 6)                                                  # the most frequent id of every component
    lock1 = np.arange(1, n, 3)                                                  # two ids of every component
    with SgnsSession(d, n, workers=case["workers"], compute_loss=True, **kw) as par, \
            SgnsSession(d, n, workers=1, compute_loss=True, **kw) as one:
        for s in (par, one):
            s.freeze(lock0, context=lock1)
        before0 = one.vectors()
        rp, r1 = par.run(case["epochs"]), one.run(case["epochs"])
        assert par.last_stats["wavefronts"] == case["wavefronts"] > 1 and one.last_stats["wavefronts"] == 1
        assert par.last_stats["lock_instances"] and one.last_stats["lock_instances"]
        assert torch.equal(par.vectors(), one.vectors()) and torch.equal(par.context_vectors(), one.context_vectors())
        assert rp == r1
        assert torch.equal(bits(par.vectors()[lock0]), bits(before0[lock0])) and not par.context_vectors()[lock1].any()
        assert (par.vectors() != before0).any()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
def masks_are(s, lock0, lock1):
    import torch

    m0, m1 = s.frozen
    return m0.dtype == m1.dtype == torch.bool and m0.is_cuda and \
        m0.nonzero().flatten().tolist() == sorted(lock0) and m1.nonzero().flatten().tolist() == sorted(lock1)


def test_locks_persist(d_walks, tmp_path):
    import torch

    from pecanpy_amd.embed import SgnsSession

    param = sc.PARAMS[5]
    other = torch.flip(d_walks, dims=[0]).contiguous()
    path = str(tmp_path / "session.ckpt")
    with open_session(d_walks, param) as whole, open_session(d_walks, param) as s:
        whole.freeze(LOCK0, context=LOCK1)
        want = whole.run(sc.EPOCHS)
        s.freeze(torch.tensor(LOCK0), context=torch.tensor(LOCK1).cuda())
        assert masks_are(s, LOCK0, LOCK1)
        assert s.run(1) == want[:1] and masks_are(s, LOCK0, LOCK1)
        s.save(path)
        with np.load(path) as z:
            assert z["frozen_vectors"].dtype == bool and np.flatnonzero(z["frozen_vectors"]).tolist() == sorted(LOCK0)
            assert np.flatnonzero(z["frozen_context"]).tolist() == sorted(LOCK1)
        with SgnsSession.restore(path, d_walks) as second:
            assert masks_are(second, LOCK0, LOCK1)
            assert second.run(2) == want[1:]
            assert torch.equal(second.vectors(), whole.vectors()) and torch.equal(second.context_vectors(), whole.context_vectors())
        s.evaluate()
        s.evaluate(other, epoch=0)
        assert masks_are(s, LOCK0, LOCK1)
        for recount in (False, True):
            s.set_walks(other if not recount else d_walks, recount=recount)
            assert masks_are(s, LOCK0, LOCK1)
        s.load(vectors=s.vectors(), context_vectors=s.context_vectors())
        assert masks_are(s, LOCK0, LOCK1)
        s.run(2)
        s.reschedule(1)
        assert masks_are(s, LOCK0, LOCK1)
        before0, before1 = s.vectors(), s.context_vectors()
        s.run(1)
        assert s.last_stats["lock_instances"] is True
        assert torch.equal(bits(s.vectors()[LOCK0]), bits(before0[LOCK0])) and torch.equal(bits(s.context_vectors()[LOCK1]), bits(before1[LOCK1]))
        s.freeze([3], context=False)                                            # replaces, and leaves syn1 free
        assert masks_are(s, [3], [])
        s.freeze(LOCK0)                                                         # context=True: the same rows
        assert masks_are(s, LOCK0, LOCK0)


def test_a_checkpoint_without_lock_keys_restores_with_nothing_frozen(d_walks, tmp_path):
    import torch

    from pecanpy_amd.embed import SgnsSession

    param = sc.PARAMS[0]
    path = str(tmp_path / "session.ckpt")
    with open_session(d_walks, param) as s:
        s.run(1)
        s.save(path)
        with np.load(path) as z:
            assert not [k for k in z.files if "frozen" in k]                    # the file a session without locks always wrote
        rest = s.run(2)
        with SgnsSession.restore(path, d_walks) as second:
            assert not second.frozen[0].any() and not second.frozen[1].any()
            assert second.run(2) == rest and second.last_stats["lock_instances"] is False
            assert torch.equal(second.vectors(), s.vectors())


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
def _karate():
    from sgns_corpora import GOLDEN

    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    return k["indptr"], k["indices"], k["data"], [str(i) for i in k["ids"]]


SUBSET_POS = [33, 0, 7, 12, 21, 4]    # positions in ``nodes``, not in ascending order: the order given is the order used


def _mode_graph(mode, seed):
    from pecanpy_amd import pecanpy as node2vec

    indptr, indices, data, ids = _karate()
    first_order = mode in ("FirstOrderUnweighted", "PreCompFirstOrder")
    kw = dict(p=1 if first_order else 0.5, q=1 if first_order else 2, random_state=seed)
    if mode == "DenseOTF":
        dense = np.zeros((34, 34))
        dense[np.repeat(np.arange(34), np.diff(indptr.astype(np.int64))), indices] = data
        return node2vec.DenseOTF.from_mat(dense, ids, **kw)
    return getattr(node2vec, mode).from_csr(indptr, indices, data, node_ids=ids, **kw)


def _oracle_walks(mode, starts, L, seed):
    from oracle import pyoracle as orc

    indptr, indices, data, _ = _karate()
    if mode == "SparseOTF":
        return orc.walks_sparse_otf(indptr, indices, data, 0.5, 2, starts, L, seed)
    if mode == "DenseOTF":
        dense = np.zeros((34, 34))
        dense[np.repeat(np.arange(34), np.diff(indptr.astype(np.int64))), indices] = data
        return orc.walks_dense_otf(dense, 0.5, 2, starts, L, seed)
    if mode == "PreComp":
        return orc.walks_precomp(indptr, indices, data, 0.5, 2, starts, L, seed)
    return orc.walks_first_order(indptr, indices, data, starts, L, seed, precomp=mode == "PreCompFirstOrder")


@pytest.mark.parametrize("mode", ["SparseOTF", "DenseOTF", "PreComp", "FirstOrderUnweighted", "PreCompFirstOrder"])
def test_walks_from_a_start_subset_equal_the_oracle(mode):
    num_walks, L, seed = 3, 12, 5
    g = _mode_graph(mode, seed)
    subset = [g.nodes[i] for i in SUBSET_POS]
    got = g.simulate_walks_array(num_walks, L, start_nodes=subset)
    starts = np.concatenate([np.array(SUBSET_POS, dtype=np.uint32)] * num_walks)
    np.random.RandomState(seed).shuffle(starts)
    assert np.array_equal(got[:, 0], starts)
    assert sorted(got[:, 0].tolist()) == sorted(SUBSET_POS * num_walks)
    assert np.array_equal(got, _oracle_walks(mode, starts, L, seed))
    # None: the matrix of every vertex, as always
    from oracle import pyoracle as orc

    whole = _mode_graph(mode, seed).simulate_walks_array(num_walks, L, start_nodes=None)
    assert np.array_equal(whole, _mode_graph(mode, seed).simulate_walks_array(num_walks, L))
    assert np.array_equal(whole, _oracle_walks(mode, orc.shuffled_starts(34, num_walks, seed), L, seed))
    # the device matrix and the other entries take the same subset
    d = _mode_graph(mode, seed)._device_walks(num_walks, L, start_nodes=subset)
    if d is not None:
        assert np.array_equal(d.cpu().numpy().view(np.uint32), got)
    assert _mode_graph(mode, seed).simulate_walks(num_walks, L, start_nodes=subset)[0][0] == g.nodes[int(starts[0])]


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
EXT_KW = dict(num_walks=4, walk_length=10, window_size=4, epochs=3, workers=1)
DIM = 16


def _karate_sparse(seed=3):
    return _mode_graph("SparseOTF", seed)


def _known(g):
    rng = np.random.default_rng(28)
    pos = np.sort(rng.permutation(34)[:28])
    ids = [g.nodes[i] for i in pos]
    vec = (rng.random((28, DIM), dtype=np.float32) - 0.5) / DIM
    ctx = (rng.random((28, DIM), dtype=np.float32) - 0.5) / DIM
    return pos, ids, vec, ctx


@pytest.mark.parametrize("with_context", [False, True], ids=["vectors", "vectors+context"])
def test_extend_session_on_karate(with_context):
    import torch

    g = _karate_sparse()
    pos, ids, vec, ctx = _known(g)
    new = np.setdiff1d(np.arange(34), pos)
    assert new.size == 6
    with g.extend_session(ids, vec, context_vectors=torch.from_numpy(ctx).cuda() if with_context else None, **EXT_KW) as s:
        m0, m1 = s.frozen
        assert m0.nonzero().flatten().tolist() == pos.tolist()
        assert m1.nonzero().flatten().tolist() == (pos.tolist() if with_context else [])
        start0, start1 = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
        assert np.array_equal(start0[pos], vec) and np.array_equal(start1[pos], ctx if with_context else np.zeros_like(ctx))
        assert not start1[new].any()
        walks = s.d_walks.cpu().numpy().view(np.uint32)
        assert walks.shape[0] == 6 * EXT_KW["num_walks"] and set(walks[:, 0].tolist()) == set(new.tolist())
        s.run(3)
        syn0, syn1 = s.vectors().cpu().numpy(), s.context_vectors().cpu().numpy()
    assert np.array_equal(syn0[pos].view(np.int32), vec.view(np.int32))
    if with_context:
        assert np.array_equal(syn1[pos].view(np.int32), ctx.view(np.int32))
    else:
        assert (syn1[pos] != 0).any(axis=1).any()
    assert (syn0[new] != start0[new]).any(axis=1).all()
    # the whole schedule at once is the session run by hand
    got = _karate_sparse().extend_embedding(ids, vec, context_vectors=ctx if with_context else None, **EXT_KW)
    assert got.dtype == np.float32 and np.array_equal(got, syn0)


def test_extend_session_starts_all_and_unfrozen():
    g = _karate_sparse()
    pos, ids, vec, _ = _known(g)
    with g.extend_session(ids, vec, starts="all", **EXT_KW) as s:
        walks = s.d_walks.cpu().numpy().view(np.uint32)
        assert walks.shape[0] == 34 * EXT_KW["num_walks"] and set(walks[:, 0].tolist()) == set(range(34))
    with _karate_sparse().extend_session(ids, vec, freeze=False, **EXT_KW) as s:
        assert not s.frozen[0].any() and not s.frozen[1].any()
        s.run(3)
        assert s.last_stats["lock_instances"] is False
        assert (s.vectors().cpu().numpy()[pos] != vec).any(axis=1).any()
    with _karate_sparse().extend_session(ids, vec, fresh_walks=True, holdout_walks=1, **EXT_KW) as s:
        new = set(np.setdiff1d(np.arange(34), pos).tolist())
        assert set(s.d_holdout.cpu().numpy().view(np.uint32)[:, 0].tolist()) == new
        records = s.run(2)
        assert "holdout_loss" in records[1]
        assert set(s.d_walks.cpu().numpy().view(np.uint32)[:, 0].tolist()) == new      # the fresh corpus of epoch 1


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edg(tmp_path_factory):
    indptr, indices, _, ids = _karate()
    path = tmp_path_factory.mktemp("karate") / "karate.edg"
    with open(path, "w") as f:
        for u in range(34):
            for v in indices[indptr[u]:indptr[u + 1]]:
                if u < v:
                    f.write(f"{ids[u]}\t{ids[v]}\n")
    return str(path)


def test_cli_init_emb(edg, tmp_path):
    from pecanpy_amd import cli
    from pecanpy_amd.embed import save_word2vec_format

    g = _karate_sparse()
    _, ids, vec, _ = _known(g)
    ids, vec = ids + ["not-a-node", "nor-this"], np.concatenate([vec, np.ones((2, DIM), np.float32)])
    npz, txt = str(tmp_path / "old.npz"), str(tmp_path / "old.emb")
    np.savez(npz, IDs=ids, data=vec)
    save_word2vec_format(txt, ids, vec)
    rounded = np.array([[float("%.6f" % x) for x in row] for row in vec.tolist()], dtype=np.float32)
    common = ["--input", edg, "--mode", "SparseOTF", "--p", "0.5", "--q", "2", "--random_state", "3", "--num-walks", "4",
              "--walk-length", "10", "--window-size", "4", "--epochs", "2", "--dimensions", "99", "--workers", "1"]
    out = {}
    for name, init, want, extra in (("npz", npz, vec, ["--freeze_init"]), ("txt", txt, rounded, ["--freeze_init"]),
                                    ("free", npz, vec, []), ("all", npz, vec, ["--freeze_init", "--walks_from", "all"])):
        path = str(tmp_path / f"{name}.npz")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            cli.main(common + ["--output", path, "--init_emb", init] + extra)
        assert [str(w.message) for w in caught if "--init_emb" in str(w.message)] == \
            ["--init_emb: 2 of 30 IDs are not in the graph and are dropped"]
        with np.load(path) as z:
            out[name] = (z["IDs"].tolist(), z["data"])
        got_ids, data = out[name]
        assert len(got_ids) == 34 and data.shape == (34, DIM) and data.dtype == np.float32    # every vertex, the file's dim
        rows = [got_ids.index(i) for i in ids[:28]]
        if extra:
            assert np.array_equal(data[rows].view(np.int32), want[:28].view(np.int32))
        else:
            assert (data[rows] != want[:28]).any(axis=1).any()
        new = [i for i in range(34) if i not in rows]
        assert len(new) == 6 and np.isfinite(data).all() and (data[new] != 0).any(axis=1).all()
    assert out["npz"][0] == out["txt"][0] and sorted(out["npz"][0]) == sorted(g.nodes)
    # the API with the same arguments on the graph the command line reads gives the same vectors (workers=1: deterministic)
    from pecanpy_amd import pecanpy as node2vec

    g2 = node2vec.SparseOTF(0.5, 2, 1, False, False, 0, 3)
    g2.read_edg_device(edg, False, False, "\t")
    api = g2.extend_embedding(ids[:28], vec[:28], num_walks=4, walk_length=10, window_size=4, epochs=2, workers=1)
    order = [g2.nodes.index(i) for i in out["npz"][0]]
    assert np.array_equal(out["npz"][1], api[order])


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------
def test_errors_that_need_the_device(d_walks):
    import ctypes as C

    import torch

    from pecanpy_amd import _lib

    param = sc.PARAMS[0]
    s = open_session(d_walks, param)
    s.freeze(LOCK0)
    for bad, text in ((np.zeros(sc.N_NODES + 1, dtype=bool), "num_nodes = 20"), ([0, sc.N_NODES], "outside 0..19"), ([-1], "outside 0..19"),
                      (np.array([0.0, 1.0]), "float"), (torch.zeros(sc.N_NODES), "float"), (torch.zeros((2, 2), dtype=torch.int64), "one dimension"),
                      (torch.zeros(sc.N_NODES, dtype=torch.bool, device="meta"), "must be on")):
        with pytest.raises(ValueError, match=text):
            s.freeze(bad)
        with pytest.raises(ValueError, match=text):
            s.freeze([1], context=bad)
        assert masks_are(s, LOCK0, LOCK0)                                       # (an error changes nothing)
    s.close()
    for use in (lambda: s.freeze([0]), s.unfreeze, lambda: s.frozen):
        with pytest.raises(ValueError, match="closed"):
            use()
    lib = _lib.load()
    mask = torch.zeros(sc.N_NODES, dtype=torch.uint8, device="cuda")
    out = (C.c_uint64 * 3)()
    for rc in (lib.pw_sgns_set_locks(None, C.c_void_p(mask.data_ptr()), None), lib.pw_sgns_get_locks(None, C.c_void_p(mask.data_ptr()), None),
               lib.pw_sgns_lock_info(None, out)):
        assert rc != 0 and b"null pointer" in lib.pw_last_error()
