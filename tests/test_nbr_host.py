"""The neighbourhood baselines on the host (no GPU): the selftest hooks with ``on_device = 0`` -- the host build of
csrc/nbr_scores.hip.h -- against the plain statement ``linkpred.neighbour_scores_host`` on every case of tests/nbr_cases.py, bit
for bit; the integer kinds against a dense boolean count; both orders of a pair; every refusal with nothing written; the Python
layer without a device; the flags of ``--task baseline``."""
import numpy as np
import pytest

import nbr_cases as nc
from pecanpy_amd import _lib, cli, linkpred
from pecanpy_amd import pecanpy as node2vec


@pytest.mark.parametrize("kind", nc.KINDS)
@pytest.mark.parametrize("name", nc.GRAPHS)
def test_host_build_equals_the_statement(name, kind):
    for m in nc.MS:
        rc, score = nc.selftest(name, *nc.pairs(name, m), kind, on_device=0)
        assert rc == 0, nc.last_error()
        assert nc.same_bits(score, nc.statement(name, m, kind)), (m, kind)


@pytest.mark.parametrize("name", nc.GRAPHS)
def test_degrees_host_build_equals_the_statement(name):
    rc, deg = nc.degrees_selftest(name, on_device=0)
    assert rc == 0, nc.last_error()
    want = linkpred.neighbour_degrees_host(*nc.graph(name))
    assert deg.dtype == want.dtype == np.uint32 and np.array_equal(deg, want)
    rows = nc.rows_of(name)
    assert np.array_equal(want, [r.size - int(x in r) for x, r in enumerate(rows)])   # the row without its loop


def _dense(name):
    """The adjacency as a dense boolean matrix without its diagonal: an independent statement of N(x)."""
    indptr, indices = nc.graph(name)
    n = indptr.size - 1
    A = np.zeros((n, n), dtype=bool)
    A[np.repeat(np.arange(n), np.diff(indptr.astype(np.int64))), indices] = True
    A[np.arange(n), np.arange(n)] = False
    return A


@pytest.mark.parametrize("name", nc.GRAPHS)
def test_integer_kinds_equal_a_dense_boolean_count(name):
    A = _dense(name)
    u, v = (x.astype(np.int64) for x in nc.pairs(name, 200))
    if name == "hubs":   # 4300 vertices: the pairs' rows of the product only
        cn = (A[u] & A[v]).sum(axis=1)
    else:
        cn = (A.astype(np.int64) @ A.astype(np.int64).T)[u, v]
    deg = A.sum(axis=1)
    assert np.array_equal(nc.statement(name, 200, "common_neighbours"), cn.astype(np.float64))
    assert np.array_equal(nc.statement(name, 200, "preferential_attachment"), (deg[u] * deg[v]).astype(np.float64))
    assert nc.selftest(name, u, v, "common_neighbours", on_device=0)[1].tolist() == cn.tolist()
    assert nc.selftest(name, u, v, "preferential_attachment", on_device=0)[1].tolist() == (deg[u] * deg[v]).tolist()


def test_hubs_holds_what_it_promises():
    rows = nc.rows_of("hubs")
    assert [rows[r].size for r in (0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14)] == [4097, 130, 65, 0, 2000, 600, 1, 63, 64, 65, 129]
    assert np.isin(rows[1], rows[0]).all() and rows[1][0] == rows[0][0] and rows[1][-1] == rows[0][-1]   # hits at both ends
    assert not np.isin(rows[2], rows[1]).any()
    assert not (nc.graph("hubs")[1] == 3).any()                                                           # vertex 3 is isolated
    assert 20 in rows[20] and 21 in rows[21] and 22 in rows[22] and 22 in rows[20] and 22 in rows[21]     # the loops
    u, v = nc.pairs("hubs", 200)
    cn = nc.statement("hubs", 200, "common_neighbours")
    where = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(u, v))}
    assert cn[where[(0, 1)]] == 130.0 and cn[where[(1, 0)]] == 130.0 and cn[where[(1, 2)]] == 0.0 and cn[where[(3, 0)]] == 0.0
    assert cn[where[(20, 21)]] == 2.0                       # 22 and 31: 20 and 21 are in both rows and are no common neighbours
    assert cn[where[(1, 1)]] == 130.0 and cn[where[(0, 0)]] == 4097.0
    jac = nc.statement("hubs", 200, "jaccard")
    assert jac[where[(3, 3)]] == 0.0 and not np.signbit(jac[where[(3, 3)]])      # denominator 0: +0.0
    assert jac[where[(0, 1)]] == 130 / 4097 and jac[where[(1, 1)]] == 1.0
    er = nc.rows_of("er-loops")
    assert sum(int(x in r) for x, r in enumerate(er)) == 20
    assert any(r.size == 0 for r in nc.rows_of("directed")[170:])
    for name in nc.GRAPHS:   # each list: u == v, an edge, a non-edge, one pair three times, both orders of the hub-hub pair
        u, v = nc.pairs(name, 63)
        rows = nc.rows_of(name)
        assert (u[0], v[0]) == (v[1], u[1]) and u[2] == v[2] and v[3] in rows[u[3]] and v[4] not in rows[u[4]]
        assert (u[5], v[5]) == (u[6], v[6]) == (u[7], v[7])


@pytest.mark.parametrize("name", nc.GRAPHS)
def test_the_order_of_the_additions_shows(name):
    """The statement summed in DESCENDING order differs somewhere on the wide table: the bit-for-bit tests do pin the order."""
    indptr, indices = nc.graph(name)
    t = nc.table(name, "wide")
    nbrs = linkpred._neighbour_sets(indptr, indices)
    u, v = nc.pairs(name, 200)
    other = np.zeros(200)
    for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        s = 0.0
        for z in sorted(nbrs[a] & nbrs[b], reverse=True):
            s = s + t[z]
        other[i] = s
    want = nc.statement(name, 200, "wide")
    assert not nc.same_bits(other, want)
    assert np.allclose(other, want, rtol=1e-9, atol=1e-9)   # (the same sums, but for the order)
    exp = np.frexp(np.abs(t))[1]
    assert exp.max() - exp.min() >= 40


@pytest.mark.parametrize("name", nc.GRAPHS)
def test_both_orders_of_a_pair_give_the_same_bits(name):
    u, v = nc.pairs(name, 200)
    for kind in nc.KINDS:
        rc, swapped = nc.selftest(name, v, u, kind, on_device=0)
        assert rc == 0 and nc.same_bits(swapped, nc.statement(name, 200, kind)), kind


def test_degree_tables():
    indptr, indices = nc.graph("hubs")
    deg = linkpred.neighbour_degrees_host(indptr, indices).astype(np.int64)
    aa, ra = nc.table("hubs", "adamic_adar"), nc.table("hubs", "resource_allocation")
    assert (aa[deg < 2] == 0.0).all() and (ra[deg < 2] == 0.0).all() and (deg < 2).any()
    big = deg >= 2
    assert nc.same_bits(aa[big], 1.0 / np.log(deg[big].astype(np.float64))) and nc.same_bits(ra[big], 1.0 / deg[big])
    with pytest.raises(ValueError, match="adamic_adar"):
        linkpred.degree_table_host(indptr, indices, "jaccard")


def test_refusals_write_nothing():
    name = "er-loops"
    u, v = nc.pairs(name, 65)
    for which, pos, needle in (("u", 40, b"u[40] = 300 is outside the 300 rows"), ("v", 9, b"v[9] = 300 is outside the 300 rows")):
        bu, bv = u.copy(), v.copy()
        (bu if which == "u" else bv)[pos] = 300
        (bu if which == "u" else bv)[pos + 5] = 4000000000
        for kind in ("common_neighbours", "wide"):
            rc, score = nc.selftest(name, bu, bv, kind, on_device=0)
            assert rc == _lib.ERR_INVALID and needle in nc.last_error(), nc.last_error()
            assert np.isnan(score).all()
        with pytest.raises(ValueError, match=needle.decode().replace("[", r"\[").replace("]", r"\]")):
            linkpred.neighbour_scores_host(*nc.graph(name), bu, bv, "jaccard")
    bu, bv = u.copy(), v.copy()
    bu[7], bv[7] = 300, 301   # both at one position: u is named
    rc, score = nc.selftest(name, bu, bv, "jaccard", on_device=0)
    assert rc == _lib.ERR_INVALID and b"u[7] = 300" in nc.last_error() and np.isnan(score).all()
    for number in (4, -1, 99):   # an unknown kind
        rc, score = nc.selftest(name, u, v, "common_neighbours", on_device=0, kind_number=number)
        assert rc == _lib.ERR_INVALID and b"kind" in nc.last_error() and np.isnan(score).all()
    rc, score = nc.selftest(name, u, v, "wide", on_device=0, tab=None)   # weighted without a table
    assert rc == _lib.ERR_INVALID and b"needs a table" in nc.last_error() and np.isnan(score).all()
    with pytest.raises(ValueError, match="kind must be one of"):
        linkpred.neighbour_scores_host(*nc.graph(name), u, v, "katz")
    with pytest.raises(ValueError, match="needs table="):
        linkpred.neighbour_scores_host(*nc.graph(name), u, v, "weighted")
    with pytest.raises(ValueError, match="one float64 per vertex"):
        linkpred.neighbour_scores_host(*nc.graph(name), u, v, "weighted", table=np.ones(299))
    rc, score = nc.selftest(name, u, v, "wide", on_device=0)   # and the call that is in order
    assert rc == 0 and not np.isnan(score).any()


# ---- the Python layer and the CLI --------------------------------------------------------------------------------------
@pytest.mark.skipif(_lib.load().pw_device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_device_entry_points_need_a_device_and_say_so():
    g = node2vec.SparseOTF.from_csr(*nc.graph("directed"), None)
    with pytest.raises(_lib.PwError, match="no HIP device"):
        g.neighbour_scores([0], [1], "jaccard")
    with pytest.raises(_lib.PwError, match="no HIP device"):
        linkpred.neighbour_degrees(g)
    with pytest.raises(_lib.PwError, match="no HIP device"):
        linkpred.degree_table(g, "adamic_adar")
    with pytest.raises(_lib.PwError, match="no HIP device"):
        linkpred.baseline_auc(g, ([0], [1]), ([2], [3]), "common_neighbours")


def test_dense_graphs_have_no_neighbour_scores():
    g = node2vec.DenseOTF.from_mat(np.ones((4, 4)) - np.eye(4), ["a", "b", "c", "d"])
    with pytest.raises(NotImplementedError, match="sparse"):
        g.neighbour_scores([0], [1], "jaccard")


def test_the_python_layer_checks_the_kind_first():
    g = node2vec.SparseOTF.from_csr(*nc.graph("directed"), None)
    with pytest.raises(ValueError, match="kind must be one of"):
        g.neighbour_scores([0], [1], "katz")
    with pytest.raises(ValueError, match="needs table="):
        g.neighbour_scores([0], [1], "weighted")
    with pytest.raises(ValueError, match="belongs to kind 'weighted'"):
        g.neighbour_scores([0], [1], "jaccard", table=np.ones(200))


def test_cli_flags_of_task_baseline(capsys):
    args = cli.parse_args(["--input", "train.npz", "--task", "baseline", "--pairs", "p.tsv", "--neg_pairs", "n.tsv", "--heuristic", "adamic_adar"])
    assert (args.task, args.pairs, args.neg_pairs, args.heuristic, args.output, args.mode) == ("baseline", "p.tsv", "n.tsv", "adamic_adar", None,
                                                                                               "SparseOTF")
    args = cli.parse_args(["--input", "g.edg", "--output", "s.tsv", "--task", "baseline", "--pairs", "p", "--heuristic", "jaccard", "--mode", "PreComp"])
    assert (args.output, args.neg_pairs, args.heuristic, args.mode) == ("s.tsv", None, "jaccard", "PreComp")
    for argv, needle in (
            (["--input", "g", "--output", "o", "--task", "baseline", "--heuristic", "jaccard"], "--task baseline needs --pairs"),
            (["--input", "g", "--output", "o", "--task", "baseline", "--pairs", "p"], "--task baseline needs --heuristic"),
            (["--input", "g", "--output", "o", "--task", "baseline", "--pairs", "p", "--heuristic", "katz"], "invalid choice: 'katz'"),
            (["--input", "g", "--output", "o", "--task", "baseline", "--pairs", "p", "--heuristic", "jaccard", "--mode", "DenseOTF"], "sparse --mode"),
            (["--input", "g", "--task", "baseline", "--pairs", "p", "--heuristic", "jaccard"], "nothing to write"),
            (["--input", "g", "--task", "score", "--pairs", "p"], "required: --output"),
            (["--input", "g"], "required: --output")):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
        assert needle in capsys.readouterr().err, argv
    args = cli.parse_args(["--input", "a", "--output", "b"])   # every other task as before
    assert (args.task, args.pairs, args.heuristic, args.metric) == ("pecanpy", None, None, "cosine")
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "TRAIN graph" in out and "train.npz" in out and "TRAIN graph" in " ".join(cli.__doc__.split())
