"""The device embedding route: ``pw_sgns_train_device`` / ``train_sgns_device`` (the walk-resident kernel of csrc/sgns.hip.h on
a walk matrix in device memory), ``Base.embed_array`` and the command line on top of it.  The yardsticks are those of
tests/test_gpu_sgns.py: the sequential restatement ``oracle.pyoracle.sgns_train`` within ``2e-5 * max|want| + 1e-6`` for one
wavefront, similarity structure for hogwild."""
import os
import warnings

import numpy as np
import pytest

from oracle import pyoracle as orc
from pecanpy_amd import cli
from pecanpy_amd import pecanpy as node2vec
from pecanpy_amd.embed import train_sgns, train_sgns_device
from pecanpy_amd.engine import PwError

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MR_HI = {"1", "2", "3", "4", "5", "6", "7", "8", "11", "12", "13", "14", "17", "18", "20", "22"}   # Zachary's first faction
SETS = [(16, 5, 3, 1e-3), (100, 10, 2, 1e-3), (8, 3, 4, 0.0), (128, 4, 1, 0.05)]   # dim, window, epochs, sample


def karate_walks(num_walks=20, L=40, seed=1, p=1.0, q=0.5):
    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    starts = orc.shuffled_starts(34, num_walks, seed)
    return orc.walks_sparse_otf(k["indptr"], k["indices"], k["data"], p, q, starts, L, seed), 34


def on_device(walks):
    import torch

    return torch.from_numpy(np.ascontiguousarray(walks, dtype=np.uint32).view(np.int32)).cuda()


def close_to_oracle(got, want):
    err, bound = np.abs(got - want).max(), 2e-5 * np.abs(want).max() + 1e-6
    print(f"max|got - want| = {err:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dim,window,epochs,sample", SETS)
def test_device_entry_equals_host_entry(dim, window, epochs, sample):
    walks, n = karate_walks(num_walks=6, L=30, seed=2)
    kw = dict(dim=dim, window=window, epochs=epochs, sample=sample, seed=7, workers=1)
    host = train_sgns(walks, n, **kw)
    d_walks = on_device(walks)
    dev = train_sgns_device(d_walks, n, **kw)
    assert dev.is_cuda and tuple(dev.shape) == (n, dim)
    assert np.array_equal(dev.cpu().numpy(), host)                       # same kernel, same inputs
    st = train_sgns_device.last_stats
    assert st["wavefronts"] == 1 and st["trained_pairs"] > 0 and 0 < st["kept_occurrences"] <= epochs * int(walks[:, -1].sum())
    assert np.array_equal(train_sgns_device(d_walks, n, **kw).cpu().numpy(), host)   # repeatable
    assert np.array_equal(d_walks.cpu().numpy().view(np.uint32), walks)   # the matrix is read, never written


@pytest.mark.parametrize("dim,window,epochs,sample", SETS)
def test_walk_resident_kernel_equals_the_sequential_restatement(dim, window, epochs, sample):
    walks, n = karate_walks(num_walks=6, L=30, seed=2)
    want, _ = orc.sgns_train(walks, n, dim=dim, window=window, epochs=epochs, sample=sample, seed=7)
    got = train_sgns_device(on_device(walks), n, dim=dim, window=window, epochs=epochs, sample=sample, seed=7, workers=1)
    close_to_oracle(got.cpu().numpy(), want)


def test_walk_resident_kernel_on_rmat_walks():
    """A larger vocabulary with isolated vertices (never in a walk: no slot of the noise table) and dead-end rows."""
    from pecanpy_amd.synth import rmat_csr

    indptr, indices, data = rmat_csr(9, seed=4)
    n = indptr.size - 1
    starts = orc.shuffled_starts(n, 2, 5)
    walks = orc.walks_sparse_otf(indptr, indices, data, 0.5, 2, starts, 20, 5)
    want, _ = orc.sgns_train(walks, n, dim=32, window=5, epochs=2, seed=11)
    got = train_sgns_device(on_device(walks), n, dim=32, window=5, epochs=2, seed=11, workers=1)
    close_to_oracle(got.cpu().numpy(), want)


@pytest.mark.parametrize("L,dim,window,negative,sample", [
    (100, 24, 6, 0, 1e-3),     # more than one ballot word of occurrences per walk; the centre is the only target
    (30, 512, 5, 5, 1e-3),     # eight components per lane
    (30, 1, 5, 5, 1e-3),       # one lane holds the whole vector
    (30, 70, 4, 8, 0.02),      # more targets than one group of row requests; a partly filled second component
])
def test_walk_resident_kernel_at_the_edges_of_its_shapes(L, dim, window, negative, sample):
    walks, n = karate_walks(num_walks=4, L=L, seed=3)
    assert L + 1 <= 64 or (walks[:, -1] > 64).any()
    want, _ = orc.sgns_train(walks, n, dim=dim, window=window, epochs=2, negative=negative, sample=sample, seed=9)
    got = train_sgns_device(on_device(walks), n, dim=dim, window=window, epochs=2, negative=negative, sample=sample, seed=9,
                            workers=1)
    close_to_oracle(got.cpu().numpy(), want)


@pytest.mark.parametrize("dim", [64, 65, 192, 200, 320, 384, 448, 449])
def test_every_instance_of_the_kernel_equals_the_restatement(dim):
    """One instance per count of components per lane (1 .. 8); only the last component of a lane is guarded, so both a
    full and a partly filled last component are run."""
    walks, n = karate_walks(num_walks=2, L=20, seed=5)
    want, _ = orc.sgns_train(walks, n, dim=dim, window=4, epochs=1, seed=21)
    got = train_sgns_device(on_device(walks), n, dim=dim, window=4, epochs=1, seed=21, workers=1)
    close_to_oracle(got.cpu().numpy(), want)


def test_repeated_targets_see_the_row_just_written():
    """Three nodes: nearly every pair draws a target twice or draws the centre.  The rows of a pair are requested together,
    so a repeated target must be read again after its first update."""
    indptr = np.array([0, 2, 4, 6], dtype=np.uint32)
    indices = np.array([1, 2, 0, 2, 0, 1], dtype=np.uint32)
    data = np.ones(6, dtype=np.float32)
    starts = orc.shuffled_starts(3, 30, 4)
    walks = orc.walks_sparse_otf(indptr, indices, data, 1.0, 1.0, starts, 25, 4)
    want, _ = orc.sgns_train(walks, 3, dim=20, window=4, epochs=2, negative=5, sample=0.0, seed=13)
    got = train_sgns_device(on_device(walks), 3, dim=20, window=4, epochs=2, negative=5, sample=0.0, seed=13, workers=1)
    close_to_oracle(got.cpu().numpy(), want)


@pytest.mark.parametrize("cls", ["SparseOTF", "DenseOTF"])
def test_embed_array_keeps_the_walks_on_the_device(cls):
    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    if cls == "SparseOTF":
        g = node2vec.SparseOTF.from_csr(k["indptr"], k["indices"], k["data"], node_ids=list(k["ids"]), p=1, q=0.5, random_state=2)
    else:
        dense = np.zeros((34, 34), dtype=np.float64)
        for i in range(34):
            dense[i, k["indices"][k["indptr"][i]:k["indptr"][i + 1]]] = k["data"][k["indptr"][i]:k["indptr"][i + 1]]
        g = node2vec.DenseOTF.from_mat(dense, list(k["ids"]), p=1, q=0.5, random_state=2)
    got = g.embed_array(dim=12, num_walks=6, walk_length=25, window_size=4, epochs=2, workers=1)
    st = g.last_embed_stats
    assert st["walk_matrix_host_bytes"] == 0 and st["train_ms"] > 0 and st["walk_ms"] > 0 and st["wavefronts"] == 1
    assert g.last_stats["total_steps"] > 0                                  # the walk call's statistics were noted
    mat = g.simulate_walks_array(6, 25)
    want = train_sgns(mat, 34, dim=12, window=4, epochs=2, workers=1, seed=2)
    assert got.dtype == np.float32 and got.shape == (34, 12) and np.array_equal(got, want)
    emb = g.embed(dim=8, num_walks=10, walk_length=20, window_size=4, epochs=3)
    assert emb.shape == (34, 8) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert g.last_embed_stats["walk_matrix_host_bytes"] == 0


def test_hogwild_through_the_device_route_agrees_in_similarity_structure():
    walks, n = karate_walks(num_walks=40, L=40, seed=3)
    want, _ = orc.sgns_train(walks, n, dim=16, window=5, epochs=30, seed=5)
    got = train_sgns_device(on_device(walks), n, dim=16, window=5, epochs=30, seed=5, workers=0).cpu().numpy()
    assert train_sgns_device.last_stats["wavefronts"] > 1

    def cos(v):
        u = v / np.linalg.norm(v, axis=1, keepdims=True)
        return u @ u.T

    a, b = cos(want), cos(got)
    off = ~np.eye(n, dtype=bool)
    corr = np.corrcoef(a[off], b[off])[0, 1]
    na = np.argsort(-np.where(off, a, -2), axis=1)[:, :5]
    nb = np.argsort(-np.where(off, b, -2), axis=1)[:, :5]
    overlap = np.mean([len(set(x) & set(y)) / 5 for x, y in zip(na, nb)])
    print(f"correlation {corr:.4f}, top-5 overlap {overlap:.4f}")
    assert corr > 0.85
    assert overlap > 0.5, overlap


def _karate_edg(path):
    """An edge list whose first-appearance numbering is irrelevant here: every edge once, IDs as in demo/karate.edg."""
    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    indptr, indices, ids = k["indptr"], k["indices"], k["ids"]
    with open(path, "w") as f:
        for u in range(34):
            for v in indices[indptr[u]:indptr[u + 1]]:
                if u < v:
                    f.write(f"{ids[u]}\t{ids[v]}\n")


ARGS = ["--mode", "SparseOTF", "--p", "1", "--q", "0.5", "--random_state", "1", "--num-walks", "20", "--walk-length", "40",
        "--dimensions", "16", "--epochs", "40", "--window-size", "5"]


def test_cli_goes_from_graph_to_vectors_without_id_lists(tmp_path, monkeypatch):
    pytest.importorskip("torch")
    try:
        import gensim  # noqa: F401
        pytest.skip("gensim present: the reference's trainer is used")
    except ImportError:
        pass
    monkeypatch.delenv("PECANPY_AMD_DUMP_WALKS", raising=False)

    def no_id_lists(args, g):
        raise AssertionError("simulate_walks must not be reached on the device route")

    monkeypatch.setattr(cli, "simulate_walks", no_id_lists)
    edg, out = tmp_path / "karate.edg", tmp_path / "karate.emb"
    _karate_edg(edg)
    cli.main(["--input", str(edg), "--output", str(out)] + ARGS)
    lines = out.read_text().splitlines()
    assert lines[0].split() == ["34", "16"] and len(lines) == 35
    names = [ln.split()[0] for ln in lines[1:]]
    vec = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[1:]])
    assert sorted(names, key=int) == [str(i) for i in range(1, 35)]
    assert np.isfinite(vec).all() and np.abs(vec).max() > 0.1             # trained, not the initial noise (|x| < 0.032)
    unit = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    sim = unit @ unit.T
    same = np.array([[(a in MR_HI) == (b in MR_HI) for b in names] for a in names])
    off = ~np.eye(34, dtype=bool)
    gap = sim[same & off].mean() - sim[~same].mean()
    print(f"faction gap {gap:.4f}")
    assert gap > 0.15


def test_cli_walk_dump_route_is_unchanged(tmp_path, monkeypatch):
    monkeypatch.setenv("PECANPY_AMD_DUMP_WALKS", "1")
    reached = []
    real = cli.simulate_walks

    def spy(args, g):
        reached.append(1)
        return real(args, g)

    monkeypatch.setattr(cli, "simulate_walks", spy)
    edg, out = tmp_path / "karate.edg", tmp_path / "karate.walks"
    _karate_edg(edg)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cli.main(["--input", str(edg), "--output", str(out)] + ARGS)
    assert reached == [1]
    rows = out.read_text().splitlines()
    assert len(rows) == 20 * 34 and all(len(r.split()) == 41 for r in rows)


def test_malformed_device_matrices_are_rejected_and_the_next_call_succeeds():
    walks, n = karate_walks(num_walks=2, L=10, seed=1)
    bad = walks.copy()
    bad[3, 2] = 99                                   # node id outside the vocabulary
    with pytest.raises(PwError, match="node id"):
        train_sgns_device(on_device(bad), n, dim=8, window=3, epochs=1, seed=1)
    bad = walks.copy()
    bad[5, -1] = 50                                  # length cell beyond the row
    with pytest.raises(PwError, match="length cell"):
        train_sgns_device(on_device(bad), n, dim=8, window=3, epochs=1, seed=1)
    with pytest.raises(PwError, match="dim"):
        train_sgns_device(on_device(walks), n, dim=513, window=3, epochs=1, seed=1)
    import torch

    out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    got = train_sgns_device(on_device(walks), n, dim=8, window=3, epochs=1, seed=1, workers=1, out=out)
    assert got is out
    want, _ = orc.sgns_train(walks, n, dim=8, window=3, epochs=1, seed=1)
    close_to_oracle(out.cpu().numpy(), want)
