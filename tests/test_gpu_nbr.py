"""The neighbourhood baselines on the GPU: the selftest hook with ``on_device = 1`` -- upload, the kernels of
csrc/nbr_scores.hip.h, download -- at every forced cut between the lane form and the wavefront form against the plain statement
``linkpred.neighbour_scores_host`` on every case of tests/nbr_cases.py, bit for bit; ``Base.neighbour_scores`` on the sparse
classes; the degree tables; the refusals; the protocol end to end on an R-MAT graph; ``--task baseline``."""
import numpy as np
import pytest

import nbr_cases as nc
from pecanpy_amd import _lib, linkpred

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cut", list(nc.SHORT_MAXES))
@pytest.mark.parametrize("name", nc.GRAPHS)
def test_kernel_equals_the_statement_at_every_cut(name, cut):
    for kind in nc.KINDS:
        for m in nc.MS:
            rc, score = nc.selftest(name, *nc.pairs(name, m), kind, on_device=1, short_max=nc.SHORT_MAXES[cut])
            assert rc == 0, nc.last_error()
            assert nc.same_bits(score, nc.statement(name, m, kind)), (kind, m)


@pytest.mark.parametrize("name", nc.GRAPHS)
def test_degrees_kernel_equals_the_statement(name):
    rc, deg = nc.degrees_selftest(name, on_device=1)
    assert rc == 0, nc.last_error()
    assert np.array_equal(deg, linkpred.neighbour_degrees_host(*nc.graph(name)))


def test_many_tiles_per_wavefront():
    """More tiles than the grid holds wavefronts (m = 1 200 000 on ``er-loops``): every wavefront walks several.  The pairs are
    the 200 of the case list repeated, so the statement's 200 values answer them all."""
    u, v = (np.tile(x, 6000) for x in nc.pairs("er-loops", 200))
    for kind in ("jaccard", "wide"):
        rc, score = nc.selftest("er-loops", u, v, kind, on_device=1)
        assert rc == 0, nc.last_error()
        assert nc.same_bits(score, np.tile(nc.statement("er-loops", 200, kind), 6000)), kind


def test_refusals_write_nothing():
    name = "er-loops"
    u, v = nc.pairs(name, 65)
    for which, pos, needle in (("u", 40, b"u[40] = 300 is outside the 300 rows"), ("v", 9, b"v[9] = 300 is outside the 300 rows")):
        bu, bv = u.copy(), v.copy()
        (bu if which == "u" else bv)[pos] = 300
        (bu if which == "u" else bv)[pos + 5] = 4000000000
        rc, score = nc.selftest(name, bu, bv, "wide", on_device=1)
        assert rc == _lib.ERR_INVALID and needle in nc.last_error(), nc.last_error()
        assert np.isnan(score).all()
    bu, bv = u.copy(), v.copy()
    bu[7], bv[7] = 300, 301
    rc, score = nc.selftest(name, bu, bv, "jaccard", on_device=1)
    assert rc == _lib.ERR_INVALID and b"u[7] = 300" in nc.last_error() and np.isnan(score).all()
    rc, score = nc.selftest(name, u, v, "common_neighbours", on_device=1, kind_number=4)
    assert rc == _lib.ERR_INVALID and b"kind" in nc.last_error() and np.isnan(score).all()
    rc, score = nc.selftest(name, u, v, "wide", on_device=1, tab=None)
    assert rc == _lib.ERR_INVALID and b"needs a table" in nc.last_error() and np.isnan(score).all()


# ---- the Python layer --------------------------------------------------------------------------------------------------
def _graph(cls, name, data=None, **kw):
    g = cls.from_csr(*nc.graph(name), data, **kw)
    g.device = 0
    return g


def test_base_neighbour_scores_on_the_sparse_classes():
    """A SparseOTF, a PreComp and a weighted SparseOTF handle (weights are not looked at: a weight of 0 is an entry), the row
    numbers as CUDA tensors, CPU tensors and NumPy arrays: the statement's bits every time."""
    import torch

    from pecanpy_amd import pecanpy as node2vec

    name = "er-loops"
    u, v = nc.pairs(name, 200)
    weights = np.random.default_rng(1).random(nc.graph(name)[1].size).astype(np.float32)
    weights[::7] = 0.0
    graphs = (_graph(node2vec.SparseOTF, name), _graph(node2vec.PreComp, name, p=0.5, q=2.0), _graph(node2vec.SparseOTF, name, data=weights))
    forms = (lambda x: torch.from_numpy(x.astype(np.int64)).cuda(), lambda x: torch.from_numpy(x.astype(np.int32)), lambda x: x.copy(),
             lambda x: x.astype(np.int64).tolist())
    for g in graphs:
        for kind in ("common_neighbours", "jaccard", "preferential_attachment", "adamic_adar", "resource_allocation"):
            want = nc.statement(name, 200, kind)
            for form in forms:
                got = g.neighbour_scores(form(u), form(v), kind)
                assert got.is_cuda and got.dtype == torch.float64 and nc.same_bits(got.cpu().numpy(), want), kind
        wide = nc.table(name, "wide")
        for tab in (wide, torch.from_numpy(wide.copy()).cuda()):
            assert nc.same_bits(g.neighbour_scores(u, v, "weighted", table=tab).cpu().numpy(), nc.statement(name, 200, "wide"))
        assert g.neighbour_scores(u[:0], v[:0], "jaccard").shape == (0,)
    g = graphs[0]
    with pytest.raises(ValueError, match=r"v\[2\] = 300 is outside the 300 rows"):
        g.neighbour_scores([0, 1, 2], [0, 1, 300], "jaccard")
    with pytest.raises(ValueError, match=r"u\[1\] = 4000000000"):
        g.neighbour_scores([0, 4000000000], [0, 1], "adamic_adar")
    with pytest.raises(ValueError, match="one float64 per vertex"):
        g.neighbour_scores([0], [1], "weighted", table=np.ones(299))
    with pytest.raises(ValueError, match="one length"):
        g.neighbour_scores([0, 1], [1], "jaccard")
    dense = node2vec.DenseOTF.from_mat(np.ones((4, 4)) - np.eye(4), ["a", "b", "c", "d"])
    dense.device = 0
    with pytest.raises(NotImplementedError, match="sparse"):
        dense.neighbour_scores([0], [1], "jaccard")
    with pytest.raises(NotImplementedError, match="sparse"):
        linkpred.neighbour_degrees(dense)


@pytest.mark.parametrize("name", nc.GRAPHS)
def test_degree_tables_equal_the_statement(name):
    import torch

    from pecanpy_amd import pecanpy as node2vec

    g = _graph(node2vec.SparseOTF, name)
    deg = linkpred.neighbour_degrees(g)
    assert deg.is_cuda and deg.dtype == torch.int64
    assert np.array_equal(deg.cpu().numpy(), linkpred.neighbour_degrees_host(*nc.graph(name)))
    for kind in ("adamic_adar", "resource_allocation"):
        t = linkpred.degree_table(g, kind)
        assert t.is_cuda and t.dtype == torch.float64 and nc.same_bits(t.cpu().numpy(), nc.table(name, kind)), kind
    with pytest.raises(ValueError, match="adamic_adar"):
        linkpred.degree_table(g, "jaccard")


# ---- the protocol end to end and the command line ----------------------------------------------------------------------
HEURISTICS = ("common_neighbours", "jaccard", "adamic_adar", "resource_allocation", "preferential_attachment")


@pytest.fixture(scope="module")
def rmat_split():
    """A 2048-vertex R-MAT graph, half of its edges held out, as many non-edges of the ORIGINAL: ``(train, pos, neg)``."""
    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.synth import rmat_csr

    indptr, indices, _ = rmat_csr(11, seed=5)
    g = node2vec.SparseOTF.from_csr(indptr, indices, None, node_ids=[f"v{i}" for i in range(indptr.size - 1)])
    g.device = 0
    train, (eu, ev, _), _ = g.holdout_edges(0.5, seed=9)
    nu, nv, _ = g.sample_non_edges(int(eu.numel()), seed=9)
    return train, (eu, ev), (nu, nv)


def test_baseline_auc_end_to_end(rmat_split):
    train, (eu, ev), (nu, nv) = rmat_split
    assert eu.numel() > 1000
    hu, hv, hnu, hnv = (x.cpu().numpy() for x in (eu, ev, nu, nv))
    for kind in HEURISTICS:
        got = linkpred.baseline_auc(train, (eu, ev), (nu, nv), kind)
        want = linkpred.auc_host(linkpred.neighbour_scores_host(train.indptr, train.indices, hu, hv, kind),
                                 linkpred.neighbour_scores_host(train.indptr, train.indices, hnu, hnv, kind))
        print(f"baseline_auc {kind}: {got}")
        assert got[1:] == want[1:] and got[0] == want[0], kind
    stacked = np.stack([hu, hv], axis=1)   # [m, 2], on the host
    assert linkpred.baseline_auc(train, stacked, (nu, nv), "jaccard")[1:] == linkpred.baseline_auc(train, (eu, ev), (nu, nv), "jaccard")[1:]


def test_cli_task_baseline(rmat_split, tmp_path, capsys):
    from pecanpy_amd import cli

    train, (eu, ev), (nu, nv) = rmat_split
    names = train.nodes
    src, out, pairs, negs = tmp_path / "train.npz", tmp_path / "scores.tsv", tmp_path / "held.tsv", tmp_path / "neg.tsv"
    train.save(src)
    hu, hv, hnu, hnv = (x.cpu().numpy() for x in (eu, ev, nu, nv))
    pairs.write_text("".join(f"{names[a]},{names[b]}\n" for a, b in zip(hu, hv)) + "\n")
    negs.write_text("".join(f"{names[a]},{names[b]}\n" for a, b in zip(hnu, hnv)))
    for kind in ("adamic_adar", "preferential_attachment"):
        cli.main(["--input", str(src), "--output", str(out), "--task", "baseline", "--pairs", str(pairs), "--neg_pairs", str(negs), "--heuristic", kind,
                  "--delimiter", ","])
        want = linkpred.neighbour_scores_host(train.indptr, train.indices, hu, hv, kind)
        value, wins, ties = linkpred.auc_host(want, linkpred.neighbour_scores_host(train.indptr, train.indices, hnu, hnv, kind))
        lines = [line.split(",") for line in out.read_text().splitlines()]
        assert [(a, b) for a, b, _ in lines] == [(names[a], names[b]) for a, b in zip(hu, hv)]
        assert nc.same_bits(np.array([float(s) for _, _, s in lines]), want)
        printed = [line for line in capsys.readouterr().out.splitlines() if not line.startswith("Took ")]
        assert printed[-1] == f"{value!r} {wins} {ties} {hu.size} {hnu.size}"
        assert (value, wins, ties) == linkpred.baseline_auc(train, (eu, ev), (nu, nv), kind)
    out.unlink()
    cli.main(["--input", str(src), "--task", "baseline", "--pairs", str(pairs), "--neg_pairs", str(negs), "--heuristic", "jaccard", "--delimiter", ","])
    printed = [line for line in capsys.readouterr().out.splitlines() if not line.startswith("Took ")]
    assert not out.exists() and len(printed[-1].split()) == 5   # without --output: the AUC line alone
