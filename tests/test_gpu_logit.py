"""Exact logistic regression on the GPU (csrc/logit.hip.h): the kernels against the NumPy statement ``classify.logit_eval_host``
bit for bit on every case of tests/logit_cases.py at several grids; many chunks per wavefront; decision values alone; the
refusals; ``fit`` against ``fit_host``; the input forms; the protocol end to end; node classification; the command line."""
import numpy as np
import pytest

import logit_cases as lc
from pecanpy_amd import _lib, classify, embed, linkpred
from test_logit_host import check_refusals

pytestmark = pytest.mark.gpu
CASES = lc.cases()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_kernels_equal_the_statement_at_every_grid(case):
    loss, grad, z = lc.statement(case)
    for blocks in (1, 3, -1):
        got_loss, got_grad, got_z = lc.selftest(case, on_device=1, blocks=blocks)
        assert lc.same_bits(got_loss, loss) and lc.same_bits(got_grad, grad) and lc.same_bits(got_z, z), blocks


@pytest.fixture(scope="module")
def tiled():
    """The 5000-sample case of dim 128 tiled to m = 300 000: ``(A, u, v, y, theta)``."""
    case = next(c for c in CASES if c.m == 5000 and c.dim == 128)
    reps = 60
    return case.A, np.tile(case.u, reps), np.tile(case.v % lc.NA, reps), np.tile(case.y, reps), np.random.default_rng(5).standard_normal(129) * 0.1


@pytest.mark.parametrize("op", ["hadamard", "l1"])
def test_many_chunks_per_wavefront(tiled, op):
    A, u, v, y, theta = tiled
    assert u.size == 300_000
    loss, grad, z = classify.logit_eval_host(A, None, u, v, y, op, theta, 0.01, return_z=True)
    rc, msg, got_loss, got_grad, got_z = lc.selftest_raw(1, A, None, u, v, y, _lib.LOGIT_OPS[op], theta, 0.01, blocks=2)
    assert rc == 0, msg
    assert lc.same_bits(got_loss, loss) and lc.same_bits(got_grad, grad) and lc.same_bits(got_z, z)


def test_decision_values_alone():
    for case in [c for c in CASES if c.m == 2049][:5]:
        z = lc.statement(case)[2]
        loss, grad, only_z = lc.selftest(case, on_device=1, with_y=False)
        assert lc.same_bits(only_z, z) and np.isnan(loss) and np.isnan(grad).all()
        loss, grad, _ = lc.selftest(case, on_device=1, want_z=False)   # and the loss without z
        assert lc.same_bits(loss, lc.statement(case)[0]) and lc.same_bits(grad, lc.statement(case)[1])


def test_refusals_write_nothing():
    check_refusals(on_device=1)
    A, B = lc.matrices(3)
    with embed.KnnIndex(A) as a, embed.KnnIndex(lc.matrices(32)[1]) as wide, embed.KnnIndex(np.zeros((2, 513), np.float32)) as too_wide:
        with pytest.raises(ValueError, match="dim 3 and 32"):
            classify.logit_eval(a, [0], [0], [1], "l1", np.zeros(4), 0.0, other=wide)
        with pytest.raises(NotImplementedError, match="dim 513 is above the trainer's cap of 512"):
            classify.logit_eval(too_wide, [0], [1], [1], "average", np.zeros(514), 0.0)
        with pytest.raises(ValueError, match=r"label y\[1\] = 255 is neither 0 nor 1"):
            classify.logit_eval(a, [0, 1], [1, 2], [1, -3], "average", np.zeros(4), 0.0)
        with pytest.raises(ValueError, match=r"row number v\[1\] = 300 is outside the 300 rows"):
            classify.logit_eval(a, [0, 1], [1, 300], [1, 0], "average", np.zeros(4), 0.0)


def test_fit_equals_fit_host():
    X, u, v, y = lc.planted()
    host = classify.fit_host(X, u, v, y, "hadamard", l2=1e-3)
    with embed.KnnIndex(X) as index:
        dev = index.fit_pairs(u, v, y, "hadamard", l2=1e-3)
        z = dev.decision_function(index, u, v)
    assert dev.converged and lc.same_bits(dev.theta, host.theta) and (dev.n_iter, dev.n_eval) == (host.n_iter, host.n_eval)
    assert lc.same_bits(dev.loss, host.loss) and lc.same_bits(z.cpu().numpy(), host.decision_function_host(X, u, v))


def test_input_forms():
    import torch

    case = next(c for c in CASES if c.m == 1025 and c.second and c.op == "l2" and c.theta_kind == "random")
    loss, grad, z = lc.statement(case)
    as_list = lambda a: [int(x) for x in a]   # noqa: E731
    forms = {"arrays": lambda a: a.astype(np.int64), "lists": as_list, "cpu tensors": lambda a: torch.from_numpy(a.astype(np.int64)),
             "cuda tensors": lambda a: torch.from_numpy(a.astype(np.int32)).cuda()}
    with embed.KnnIndex(case.A) as a, embed.KnnIndex(case.B) as b:
        for name, form in forms.items():
            got = classify.logit_eval(a, form(case.u), form(case.v), form(case.y), case.op, case.theta, case.l2, other=b, return_z=True)
            assert lc.same_bits(got[0], loss) and lc.same_bits(got[1], grad) and lc.same_bits(got[2].cpu().numpy(), z), name
        assert lc.same_bits(classify.logit_eval(a, case.u, case.v, None, case.op, case.theta, 0.0, other=b).cpu().numpy(), z)
        for dtype in (torch.int8, torch.bool, torch.int64):   # every integer label type on the device, the narrow ones included
            got = classify.logit_eval(a, case.u, case.v, torch.from_numpy(case.y).cuda().to(dtype), case.op, case.theta, case.l2, other=b)
            assert lc.same_bits(got[0], loss) and lc.same_bits(got[1], grad), dtype
        bad = torch.from_numpy(case.y).cuda().to(torch.int8)
        bad[9] = -3
        with pytest.raises(ValueError, match=r"label y\[9\] = 255 is neither 0 nor 1"):
            classify.logit_eval(a, case.u, case.v, bad, case.op, case.theta, case.l2, other=b)


@pytest.fixture(scope="module")
def rmat_protocol():
    """The 2048-vertex R-MAT graph of test_gpu_nbr.py, half of its edges held out, as many non-edges of the ORIGINAL, the train
    graph embedded: ``(vectors, names, pos, neg)`` with the pairs on the host."""
    from pecanpy_amd import pecanpy as node2vec
    from pecanpy_amd.synth import rmat_csr

    indptr, indices, _ = rmat_csr(11, seed=5)
    g = node2vec.SparseOTF.from_csr(indptr, indices, None, node_ids=[f"v{i}" for i in range(indptr.size - 1)])
    g.device = 0
    train, (eu, ev, _), _ = g.holdout_edges(0.5, seed=9)
    nu, nv, _ = g.sample_non_edges(int(eu.numel()), seed=9)
    vectors = np.ascontiguousarray(train.embed_array(dim=32, num_walks=4, walk_length=20, window_size=5), dtype=np.float32)
    return vectors, train.nodes, (eu.cpu().numpy(), ev.cpu().numpy()), (nu.cpu().numpy(), nv.cpu().numpy())


def test_classifier_auc_end_to_end(rmat_protocol):
    import torch

    X, _, (eu, ev), (nu, nv) = rmat_protocol
    h = eu.size // 2
    assert h > 500
    train_pos, test_pos, train_neg, test_neg = (eu[:h], ev[:h]), (eu[h:], ev[h:]), (nu[:h], nv[:h]), (nu[h:], nv[h:])
    with embed.KnnIndex(X) as index:
        value, wins, ties, model = linkpred.classifier_auc(index, tuple(torch.from_numpy(x.astype(np.int64)).cuda() for x in train_pos), train_neg,
                                                           np.stack(test_pos, axis=1), test_neg, "hadamard", 1e-3)
    y = np.concatenate([np.ones(h, np.uint8), np.zeros(h, np.uint8)])
    host = classify.fit_host(X, np.concatenate([train_pos[0], train_neg[0]]), np.concatenate([train_pos[1], train_neg[1]]), y, "hadamard", l2=1e-3)
    want = linkpred.auc_host(host.decision_function_host(X, *test_pos), host.decision_function_host(X, *test_neg))
    print(f"classifier_auc hadamard: {value!r} ({wins} wins, {ties} ties; {model.n_iter} iterations, {model.n_eval} evaluations)")
    assert lc.same_bits(model.theta, host.theta) and (value, wins, ties) == want


def test_node_classification(rmat_protocol):
    X = rmat_protocol[0]
    rng = np.random.default_rng(8)
    rows = rng.permutation(X.shape[0])[:1500]
    Y = ((X[rows].astype(np.float64) @ rng.standard_normal((X.shape[1], 2)) + 0.2 * rng.standard_normal((1500, 2))) > 0).astype(np.uint8)
    host = classify.fit_one_vs_rest_host(X, rows, Y, l2=1e-2)
    with embed.KnnIndex(X) as index:
        dev = classify.fit_one_vs_rest(index, rows, Y, l2=1e-2)
        z = dev[0].decision_function(index, rows)
    for d, h in zip(dev, host):
        assert d.op == "row" and lc.same_bits(d.theta, h.theta) and (d.n_iter, d.n_eval, d.converged) == (h.n_iter, h.n_eval, h.converged)
    assert lc.same_bits(z.cpu().numpy(), host[0].decision_function_host(X, rows))


def test_cli_fit_then_score(rmat_protocol, tmp_path, capsys):
    from pecanpy_amd import cli

    X, names, (eu, ev), (nu, nv) = rmat_protocol
    h = 600
    emb, pos, neg, model_path, out = (tmp_path / n for n in ("x.npz", "pos.tsv", "neg.tsv", "model.tsv", "scores.tsv"))
    np.savez(emb, IDs=np.array(names), data=X)
    pos.write_text("".join(f"{names[a]}\t{names[b]}\n" for a, b in zip(eu[:h], ev[:h])))
    neg.write_text("".join(f"{names[a]}\t{names[b]}\n" for a, b in zip(nu[:h], nv[:h])))
    cli.main(["--task", "fit", "--input", str(emb), "--pairs", str(pos), "--neg_pairs", str(neg), "--operator", "l1", "--l2_penalty", "0.01",
              "--output", str(model_path)])
    y = np.concatenate([np.ones(h, np.uint8), np.zeros(h, np.uint8)])
    with embed.KnnIndex(X) as index:
        want = classify.fit(index, np.concatenate([eu[:h], nu[:h]]), np.concatenate([ev[:h], nv[:h]]), y, "l1", l2=0.01)
        z_pos, z_neg = want.decision_function(index, eu[:h], ev[:h]), want.decision_function(index, nu[:h], nv[:h])
        value, wins, ties = linkpred.auc(z_pos, z_neg)
    got = classify.LogisticModel.load(model_path)
    assert lc.same_bits(got.theta, want.theta) and (got.op, got.l2, got.n_eval) == ("l1", 0.01, want.n_eval)
    printed = [line for line in capsys.readouterr().out.splitlines() if not line.startswith("Took ")]
    assert printed[-1] == f"{want.loss!r} {want.n_iter} {want.n_eval} {int(want.converged)}"
    cli.main(["--task", "score", "--input", str(emb), "--pairs", str(pos), "--neg_pairs", str(neg), "--model", str(model_path), "--output", str(out)])
    lines = [line.split("\t") for line in out.read_text().splitlines()]
    assert lc.same_bits(np.array([float(s) for _, _, s in lines]), z_pos.cpu().numpy())
    printed = [line for line in capsys.readouterr().out.splitlines() if not line.startswith("Took ")]
    assert printed[-1] == f"{value!r} {wins} {ties} {h} {h}"

    labels = tmp_path / "labels.tsv"
    rows = np.arange(0, 900, 3)
    lab = (X[rows, 0] > 0).astype(np.uint8)
    labels.write_text("".join(f"{names[r]}\t{int(b)}\n" for r, b in zip(rows, lab)))
    cli.main(["--task", "fit", "--input", str(emb), "--labels", str(labels), "--output", str(model_path)])
    with embed.KnnIndex(X) as index:
        want = classify.fit(index, rows, None, lab, "row", l2=1e-3)
    got = classify.LogisticModel.load(model_path)
    assert got.op == "row" and lc.same_bits(got.theta, want.theta)


def test_session_fit_pairs():
    """``SgnsSession.fit_pairs`` is ``KnnIndex.fit_pairs`` on the session's matrices as they are now: against the context
    vectors (two indexes) and against the vectors themselves, equal to ``fit_host`` on the matrices copied to the host."""
    import torch

    rng = np.random.default_rng(21)
    n, m = 200, 1500
    mat = rng.integers(0, n, (300, 20)).astype(np.int32)
    mat[:, -1] = 19   # (the last column of a walk matrix: the number of vertices in the row)
    walks = torch.from_numpy(mat).cuda()
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    with embed.SgnsSession(walks, n, dim=16, window=3, epochs=1, workers=1, seed=4) as session:
        session.run(1)
        X, Ctx = session.vectors().cpu().numpy(), session.context_vectors().cpu().numpy()
        y = ((X[u].astype(np.float64) * Ctx[v].astype(np.float64)).sum(1) > 0).astype(np.uint8)
        for against, other in (("context", Ctx), ("vectors", None)):
            got = session.fit_pairs(u, v, y, "hadamard", l2=1e-2, against=against)
            want = classify.fit_host(X, u, v, y, "hadamard", l2=1e-2, other=other)
            assert lc.same_bits(got.theta, want.theta) and (got.n_iter, got.n_eval) == (want.n_iter, want.n_eval), against
            with embed.KnnIndex(X) as a:
                direct = a.fit_pairs(u, v, y, "hadamard", l2=1e-2, other=embed.KnnIndex(Ctx) if other is not None else None)
            assert lc.same_bits(direct.theta, got.theta), against
        with pytest.raises(ValueError, match="against must be"):
            session.fit_pairs(u, v, y, "hadamard", against="both")
