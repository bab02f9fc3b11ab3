"""(CPU) The skip-gram session before a GPU sees it: the NumPy restatement the GPU tests compare with (tests/sgns_session_ref.py)
is the float64 reference of the one-shot trainer (tests/sgns_f64.py) plus the loss and the state, its slices compose, and the
figures the GPU tests take from it -- the loss tolerance, the fall of the loss on the two-clique corpus -- are what
tests/test_gpu_sgns_session.py records; ``SgnsSession`` validates its arguments and ``restore`` its corpus before any device
work; the C ABI declares and exports the session's entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sgns_f64
import sgns_session_cases as sc
import sgns_session_ref as ref
import sgns_shape_cases as shapes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["pw_sgns_create_device", "pw_sgns_run", "pw_sgns_get_state", "pw_sgns_set_state", "pw_sgns_vectors_get",
                "pw_sgns_vectors_set", "pw_sgns_destroy"]


@pytest.mark.parametrize("case_id", shapes.IDS)
def test_the_restatement_is_the_float64_reference_plus_the_loss(case_id):
    """Bit for bit on every case of tests/sgns_shape_cases.py, with the reference's counts; the loss is finite, positive and
    counts the reference's evaluations."""
    r = shapes.reference(case_id)
    s, records = ref.train(r["mat"], r["n"], **r["kw"])
    assert np.array_equal(s.syn0, r["want64"])
    d = r["diag"]
    assert sum(x["kept_occurrences"] for x in records) == d["kept"]
    assert sum(x["trained_pairs"] for x in records) == d["pairs"]
    assert sum(x["evaluations"] for x in records) == d["evaluations"]
    assert len(records) == r["kw"]["epochs"] and all(np.isfinite(x["loss"]) and x["loss"] > 0 for x in records)


def test_softplus_is_finite_and_exact_where_the_sigmoid_is_clipped():
    assert ref.softplus(0.0) == np.log(2.0)
    assert ref.softplus(800.0) == 800.0 and ref.softplus(-800.0) == 0.0            # (no overflow on either side)
    assert ref.softplus(7.0) == pytest.approx(7.0 + np.log1p(np.exp(-7.0)), rel=1e-15)
    assert ref.softplus(-7.0) == pytest.approx(np.log1p(np.exp(-7.0)), rel=1e-15)
    assert ref.softplus(-7.0) > 0.0                                                # (a saturated evaluation still contributes)


@pytest.mark.parametrize("param", [sc.PARAMS[3], sc.PARAMS[12]], ids=[sc.IDS[3], sc.IDS[12]])
def test_the_restatements_slices_compose(param):
    """run(1) three times, run(1) + run(2) and run(3) once: the same matrices, records and state."""
    whole = sc.reference(param)["schedule"]
    for slices in ([1, 1, 1], [1, 2]):
        s, records = ref.train(sc.corpus(), sc.N_NODES, slices=slices, **sc.kw_of(param))
        assert np.array_equal(s.syn0, whole["syn0"]) and np.array_equal(s.syn1, whole["syn1"])
        assert records == whole["records"]
        assert s.state == whole["state"]
    with pytest.raises(ValueError):
        s.run(1)


def test_the_cases_reach_what_they_are_for():
    mat = sc.corpus()
    assert mat.shape == (sc.N_WALKS, sc.L + 2) and mat[3, -1] == 1 and 1 < mat[7, -1] < sc.L + 1
    assert set(range(17, 20)).isdisjoint(sc.used_ids().tolist())
    for param in sc.PARAMS:
        r = sc.reference(param)
        records = r["schedule"]["records"] + r["rescheduled"]["records"]
        occurrences = int(mat[:, -1].sum())
        if param[2]:
            assert all(x["kept_occurrences"] < 0.9 * occurrences for x in records)     # the sample value thins this corpus
        else:
            assert all(x["kept_occurrences"] == occurrences for x in records)
        # ids that occur nowhere are never a target: syn1 stays zero there, and it moves elsewhere
        assert not r["schedule"]["syn1"][17:].any() and r["schedule"]["syn1"][sc.used_ids()].any(axis=1).all()
        assert r["rescheduled"]["state"]["epoch"] == sc.EPOCHS + 1


def test_the_loss_tolerance_is_four_times_the_float32_gap():
    """``g``: the largest relative distance between the epoch losses of the float32 and the float64 restatement over the
    cases; the GPU test uses ``4 g`` as recorded there.  NumPy's ``dot`` and ``exp`` differ between builds in the last bit, so
    the recorded figure is held to a factor of two, not to its digits."""
    import test_gpu_sgns_session as gpu

    g = max(sc.loss_gap(p) for p in sc.PARAMS)
    print(f"g = {g:.3e}, recorded {gpu.LOSS_GAP:.3e}, tol {gpu.LOSS_TOL:.3e}")
    assert gpu.LOSS_TOL == 4 * gpu.LOSS_GAP
    assert gpu.LOSS_GAP / 2 <= g <= gpu.LOSS_GAP * 2
    # the float32 restatement's vectors are inside the one-wavefront bound the kernel is held to
    for p in sc.PARAMS:
        for part in ("schedule", "rescheduled"):
            want = sc.reference(p)[part]
            got = sc.reference(p, "float32")[part]
            for m in ("syn0", "syn1"):
                assert np.abs(got[m] - want[m]).max() <= sc.bound(want[m])


def test_the_restatements_loss_falls_on_the_two_cliques():
    """What the racing GPU run is asked for is half of the restatement's own fall, and that fall is far above the float32 /
    float64 gap of the restatement."""
    import test_gpu_sgns_session as gpu

    mean = {}
    for dtype in (np.float64, np.float32):
        _, records = ref.train(sc.clique_corpus(), sc.CLIQUE_NODES, dtype=dtype, **sc.CLIQUE_KW)
        mean[dtype] = [x["loss"] / x["evaluations"] for x in records]
    fall = mean[np.float64][0] - mean[np.float64][-1]
    gap = max(abs(a - b) for a, b in zip(mean[np.float64], mean[np.float32]))
    print(f"mean loss per epoch {mean[np.float64]}, fall {fall:.6f}, float32 gap {gap:.2e}")
    assert fall == pytest.approx(gpu.CLIQUE_FALL, rel=1e-6)
    assert gpu.CLIQUE_REQUIRED == gpu.CLIQUE_FALL / 2
    assert fall > 1000 * gap


# ---- the Python surface, before any device work --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, text", [
    (dict(num_nodes=0), "num_nodes"),
    (dict(dim=0), "dim"),
    (dict(dim=513), "dim"),
    (dict(window=0), "window"),
    (dict(epochs=0), "epochs"),
    (dict(negative=-1), "negative"),
    (dict(workers=-1), "workers"),
    (dict(sample=-0.5), "sample"),
    (dict(alpha=float("nan")), "alpha"),
])
def test_session_arguments_are_checked_first(kw, text):
    from pecanpy_amd.embed import SgnsSession

    kw = dict(dict(num_nodes=20), **kw)
    with pytest.raises(ValueError, match=text):
        SgnsSession(None, **kw)


def test_session_wants_a_device_matrix():
    import torch

    from pecanpy_amd.embed import SgnsSession

    host = torch.from_numpy(sc.corpus().view(np.int32).copy())
    for bad in (sc.corpus(), host, host.to(torch.int64)):
        with pytest.raises(ValueError, match="contiguous int32 CUDA tensor"):
            SgnsSession(bad, sc.N_NODES)


def _checkpoint(path, corpus_shape):
    dim = 8
    arrays = dict(vectors=np.zeros((sc.N_NODES, dim), np.float32), context_vectors=np.zeros((sc.N_NODES, dim), np.float32),
                  corpus_shape=np.array(corpus_shape, dtype=np.int64), state_epoch=np.array(1), state_sched_pos=np.array(1),
                  state_sched_total=np.array(3), state_alpha=np.array(0.025), state_min_alpha=np.array(1e-4))
    params = dict(dim=dim, window=3, epochs=3, negative=5, alpha=0.025, min_alpha=1e-4, sample=0.0, seed=7, workers=1, compute_loss=True)
    arrays.update({"param_" + k: np.array(v) for k, v in params.items()})
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def test_restore_refuses_a_corpus_of_another_shape(tmp_path):
    import torch

    from pecanpy_amd.embed import SgnsSession

    path = str(tmp_path / "session.npz")
    _checkpoint(path, (sc.N_WALKS + 1, sc.L, sc.N_NODES))
    host = torch.from_numpy(sc.corpus().view(np.int32).copy())
    with pytest.raises(ValueError, match="13 walks of length 9"):
        SgnsSession.restore(path, host)
    _checkpoint(path, (sc.N_WALKS, sc.L + 1, sc.N_NODES))
    with pytest.raises(ValueError, match="12 walks of length 10"):
        SgnsSession.restore(path, host)
    # the right shape gets as far as the constructor, which wants the matrix on a device
    _checkpoint(path, (sc.N_WALKS, sc.L, sc.N_NODES))
    with pytest.raises(ValueError, match="CUDA tensor"):
        SgnsSession.restore(path, host)


def test_embed_session_has_no_device_matrix_under_the_multi_gpu_routes(monkeypatch):
    from pecanpy_amd import pecanpy as node2vec

    g = node2vec.SparseOTF(1, 1, 1)
    monkeypatch.setattr(g, "_device_walks", lambda num_walks, walk_length: None)
    with pytest.raises(NotImplementedError, match="device"):
        g.embed_session(8, 2, 5, 3, 1)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_session_and_the_library_exports_it():
    from pecanpy_amd import _lib

    text = open(os.path.join(REPO, "include", "pecanpy_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"PW_SGNS_LOSS\s*=\s*1\b", code)
    assert "BORROWED" in text                                           # the header says whose the walk matrix is
    for struct, fields in (("pw_sgns_epoch", ["loss", "kept_occurrences", "trained_pairs", "evaluations"]),
                           ("pw_sgns_state", ["epoch", "sched_pos", "sched_total", "alpha", "min_alpha"])):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", code, flags=re.S).group(1)
        assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == fields
    assert [n for n, _ in _lib.PwSgnsEpoch._fields_] == ["loss", "kept_occurrences", "trained_pairs", "evaluations"]
    assert C.sizeof(_lib.PwSgnsEpoch) == 32 and C.sizeof(_lib.PwSgnsState) == 32
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name


def test_the_session_entries_reject_null_handles_without_a_device():
    from pecanpy_amd import _lib

    lib = _lib.load()
    st = _lib.PwSgnsState()
    assert lib.pw_sgns_get_state(None, C.byref(st)) != 0 and b"null pointer" in lib.pw_last_error()
    assert lib.pw_sgns_run(None, 1, None, None) != 0
    assert lib.pw_sgns_vectors_get(None, 0, None) != 0
    lib.pw_sgns_destroy(None)
    handle = C.c_void_p()
    assert lib.pw_sgns_create_device(0, None, 1, 9, 20, 8, 3, 5, 1, 0.025, 1e-4, 0.0, 7, 1, 0, C.byref(handle)) != 0
    assert b"null pointer / empty corpus" in lib.pw_last_error() and not handle.value
