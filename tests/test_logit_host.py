"""Exact logistic regression without a GPU: the library's host build of the definition (csrc/logit.hip.h) against the NumPy
statement ``classify.logit_eval_host`` bit for bit on every case of tests/logit_cases.py; the definition's own ``exp`` /
``log1p``; the order of the additions; an independent gradient; the refusals; the optimiser; the model file; the command line."""
import ctypes as C

import numpy as np
import pytest

import logit_cases as lc
from pecanpy_amd import _lib, classify

CASES = lc.cases()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_host_build_equals_the_statement(case):
    loss, grad, z = lc.statement(case)
    got_loss, got_grad, got_z = lc.selftest(case, on_device=0)
    assert lc.same_bits(got_loss, loss) and lc.same_bits(got_grad, grad) and lc.same_bits(got_z, z)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    only_z = lc.selftest(case, on_device=0, with_y=False)
    assert lc.same_bits(only_z[2], z) and np.isnan(only_z[0]) and np.isnan(only_z[1]).all()   # y = NULL: z alone


def test_case_list_covers_what_it_must():
    assert {c.dim for c in CASES} == set(lc.DIMS) and {c.m for c in CASES} == set(lc.MS) and {c.op for c in CASES} == set(lc.OPS)
    assert {(c.labels, c.l2) for c in CASES} >= {(a, b) for a in lc.LABELS for b in lc.L2S}
    assert {(c.op, c.theta_kind, c.second) for c in CASES} >= {(o, t, s) for o in lc.OPS for t in lc.THETAS for s in (False, True)}
    for c in CASES:
        if c.m >= 4:
            assert c.u[1] == c.v[1] and (c.u[2], c.v[2]) == (c.u[3], c.v[3])
        assert c.u[0] == lc.NA - 1 and c.v[0] == (lc.NB if c.second else lc.NA) - 1
        if c.theta_kind == "scaled":
            z = lc.statement(c)[2]
            assert (np.abs(z) > 40).any() and (np.abs(z) > 708).any()


def _math(which, x):
    out = np.full(x.size, np.nan)
    assert _lib.load().pw_selftest_logit_math(which, C.c_void_p(x.ctypes.data), x.size, C.c_void_p(out.ctypes.data)) == 0
    return out


def _ulps(got, ref):
    return float((np.abs(got - ref) / np.spacing(ref)).max())


def test_the_two_functions():
    """lg_exp / lg_log1p of the host build equal their NumPy statements bit for bit, and are close to libm's.

    Measured against NumPy on 2 000 000 uniform points (and the composed points t = lg_exp(x) that the loss really feeds to
    lg_log1p): lg_exp at most 1.0 ulp on [-708, 0] (asserted <= 2: NumPy's own exp may be off by one); lg_log1p at most 3.0 ulp
    on [0, 1] (asserted <= 4 = the measured maximum + 1).  lg_log1p's result 2 s q carries the roundings of s, q and the
    product, 1.5 ulp of relative error, which is 3 ulp just above a power of two."""
    rng = np.random.default_rng(11)
    below = np.nextafter(-708.0, -np.inf)
    x = np.concatenate([rng.uniform(-708.0, 0.0, 100_000), [0.0, -0.0, -708.0, below, -1e-300, -745.0, -1e300]])
    got = _math(0, x)
    assert lc.same_bits(got, classify.lg_exp_host(x))
    assert got[x < -708.0].tolist() == [0.0, 0.0, 0.0] and not np.signbit(got).any() and got[0 + 100_000] == 1.0
    assert got[x == -708.0][0] > 0.0
    t = np.concatenate([rng.uniform(0.0, 1.0, 100_000), [0.0, 1.0, 5e-324, 1e-300, 0.5], got[:1000]])
    got_l = _math(1, t)
    assert lc.same_bits(got_l, classify.lg_log1p_host(t)) and got_l[100_000] == 0.0

    xs = rng.uniform(-708.0, 0.0, 2_000_000)
    e = _math(0, xs)
    exp_ulps = _ulps(e, np.exp(xs))
    ts = np.concatenate([rng.uniform(0.0, 1.0, 2_000_000), e[e > 0.0]])
    log1p_ulps = _ulps(_math(1, ts), np.log1p(ts))
    print(f"lg_exp: {exp_ulps} ulp from np.exp; lg_log1p: {log1p_ulps} ulp from np.log1p")
    assert exp_ulps <= 2.0
    assert log1p_ulps <= 4.0


def test_the_order_of_the_additions_shows():
    """The statement summed in chunks of 512, or in descending sample order, is the same number to 1e-9 and not the same bits."""
    case = next(c for c in CASES if c.m == 5000 and c.theta_kind == "random")
    loss, grad, _ = lc.statement(case)
    for other in (dict(_chunk=512), dict(_descending=True)):
        o_loss, o_grad = classify.logit_eval_host(case.A, case.B, case.u, case.v, case.y, case.op, case.theta, case.l2, **other)
        assert np.allclose(o_grad, grad, rtol=1e-9, atol=0) and np.isclose(o_loss, loss, rtol=1e-9)
        assert not (lc.same_bits(o_grad, grad) and lc.same_bits(o_loss, loss)), other


RANDOM = [c for c in CASES if c.theta_kind == "random"]   # every random-theta case of the list


def test_independent_gradient():
    """A vectorised np.exp / matrix-product expression agrees with the statement's grad, entry by entry, and with its loss, on
    every random-theta case.

    Measured over those 34 cases: the largest PER-ENTRY relative disagreement |difference| / |grad[k]| is 2.43e-13 (small
    entries are sums that cancel; against max|grad| of the case the largest is 2.15e-15), the largest of the loss 2.05e-15.
    The test asserts ten times each as a per-entry rtol with no absolute term: 2.5e-12 and 2.1e-14."""
    assert len(RANDOM) == 34 and {c.m for c in RANDOM} == set(lc.MS) and {c.dim for c in RANDOM} == set(lc.DIMS)
    worst, worst_loss = 0.0, 0.0
    for case in RANDOM:
        loss, grad, _ = lc.statement(case)
        i_loss, i_grad = lc.independent(case.A, case.B, case.u, case.v, case.y, case.op, case.theta, case.l2)
        worst = max(worst, float((np.abs(i_grad - grad) / np.abs(grad)).max()))
        worst_loss = max(worst_loss, abs(i_loss - loss) / abs(loss))
    print(f"independent gradient: worst per-entry relative disagreement {worst:.3g}, of the loss {worst_loss:.3g}")
    assert worst <= 2.5e-12 and worst_loss <= 2.1e-14


FD_COORDS = (0, 1, 31, 32, 33, 127, 128, 129)   # and dim // 2, dim - 1, the bias: both sides of the 32-column chunk and of column 128


@pytest.mark.parametrize("case", RANDOM, ids=repr)
def test_central_difference(case):
    """d loss / d theta[k] by a central difference of the statement's loss, h = 1e-6, agrees with grad[k] to 1e-6 of |grad[k]|
    itself, on every random-theta case, at a fixed spread of coordinates: 0, 1, dim // 2, dim - 1, the bias and, where the case
    has them, 31, 32, 33 and 127, 128, 129 (the last staged chunk and the lanes' second column pair).

    The difference quotient cannot know the loss better than the loss is rounded: two losses with an error of half an ulp each
    move it by up to eps * |loss| / (2 h), half a UNIT u = eps * max(1, |loss|) / h, and the sum of m terms adds to that.
    Measured over all 34 cases and these coordinates: one entry (grad[32] = -2.2e-4 of the dim 130, m = 64 case, loss 4.6) misses
    the relative bound alone, by 0.59 u; the absolute term is ten times that, 6 u (6.2e-9 at that loss)."""
    loss, grad, _ = lc.statement(case)
    h = 1e-6
    floor = 6.0 * np.finfo(np.float64).eps * max(1.0, abs(loss)) / h
    for k in sorted({k for k in FD_COORDS + (case.dim // 2, case.dim - 1, case.dim) if k <= case.dim}):
        step = np.zeros(case.dim + 1)
        step[k] = h
        up = classify.logit_eval_host(case.A, case.B, case.u, case.v, case.y, case.op, case.theta + step, case.l2)[0]
        down = classify.logit_eval_host(case.A, case.B, case.u, case.v, case.y, case.op, case.theta - step, case.l2)[0]
        assert abs((up - down) / (2 * h) - grad[k]) <= 1e-6 * abs(grad[k]) + floor, k


# ---- refusals ------------------------------------------------------------------------------------------------------------
def refusal_inputs():
    """``name -> (kwargs changed from a good call, message fragment, exception of the Python layer)``."""
    A, B = lc.matrices(3)
    m = 10
    good = dict(A=A, B=B, u=np.arange(m, dtype=np.uint32), v=np.arange(m, dtype=np.uint32), y=(np.arange(m) % 2).astype(np.uint8), op="l1",
                theta=np.array([0.5, -1.0, 2.0, 0.1]), l2=0.01)
    u_bad, v_bad, both_bad, y_bad = good["u"].copy(), good["v"].copy(), good["u"].copy(), good["y"].copy()
    u_bad[6], v_bad[4], both_bad[4], y_bad[7] = lc.NA, lc.NB, lc.NA + 3, 2
    nan_theta, huge = good["theta"].copy(), np.array([1e300, 1e300, 1e300, 0.0])
    nan_theta[1] = np.nan
    return good, {
        "u out of range": (dict(u=u_bad), f"row number u[6] = {lc.NA} is outside the {lc.NA} rows"),
        "v out of range": (dict(v=v_bad), f"row number v[4] = {lc.NB} is outside the {lc.NB} rows"),
        "u before v": (dict(u=both_bad, v=v_bad), f"row number u[4] = {lc.NA + 3}"),
        "label": (dict(y=y_bad), "label y[7] = 2 is neither 0 nor 1"),
        "rows before labels": (dict(u=u_bad, y=y_bad), "row number u[6]"),
        "theta": (dict(theta=nan_theta), "theta[1] is not finite"),
        "l2 negative": (dict(l2=-1.0), "l2 must be finite and >= 0"),
        "l2 nan": (dict(l2=float("nan")), "l2 must be finite and >= 0"),
        "z": (dict(A=A * np.float32(1e5), B=B * np.float32(1e5), theta=huge, op="hadamard"), "the decision value z[0] is not finite"),
    }


def check_refusals(on_device):
    good, bad = refusal_inputs()
    for name, (change, fragment) in bad.items():
        k = dict(good, **change)
        for y in (k["y"], None):
            if y is None and "label" in fragment:
                continue
            rc, msg, loss, grad, z = lc.selftest_raw(on_device, k["A"], k["B"], k["u"], k["v"], y, _lib.LOGIT_OPS[k["op"]], k["theta"], k["l2"])
            assert rc == _lib.ERR_INVALID and fragment in msg, (name, msg)
            assert np.isnan(loss) and np.isnan(grad).all() and np.isnan(z).all(), name   # nothing written
    rc, msg, *_ = lc.selftest_raw(on_device, good["A"], good["B"], good["u"], good["v"], good["y"], 7, good["theta"], 0.0)
    assert rc == _lib.ERR_INVALID and "op 7 is none of" in msg
    u = good["u"]
    v_ignored = np.full(u.size, 4_000_000_000, dtype=np.uint32)   # op row: v is not even range-checked
    rc, msg, loss, *_ = lc.selftest_raw(on_device, good["A"], None, u, v_ignored, good["y"], _lib.LOGIT_OPS["row"], good["theta"], 0.0)
    assert rc == 0 and np.isfinite(loss), msg


def test_refusals_of_the_host_build():
    check_refusals(on_device=0)
    wide = np.zeros((2, 513), dtype=np.float32)
    rc, msg, loss, grad, z = lc.selftest_raw(0, wide, None, [0], [1], [1], _lib.LOGIT_OPS["average"], np.zeros(514), 0.0)
    assert rc == _lib.ERR_UNSUPPORTED and "dim 513 is above the trainer's cap of 512" in msg and np.isnan(loss) and np.isnan(z).all()
    ok = lc.selftest_raw(0, wide[:, :512], None, [0], [1], [1], _lib.LOGIT_OPS["average"], np.zeros(513), 0.0)
    assert ok[0] == 0 and ok[2] == classify.logit_eval_host(wide[:, :512], None, [0], [1], [1], "average", np.zeros(513), 0.0)[0]


def test_refusals_of_the_python_layer():
    good, bad = refusal_inputs()
    for name, (change, fragment) in bad.items():
        k = dict(good, **change)
        with pytest.raises(ValueError) as e:
            classify.logit_eval_host(k["A"], k["B"], k["u"], k["v"], k["y"], k["op"], k["theta"], k["l2"])
        assert fragment in str(e.value), name
    g = good
    with pytest.raises(ValueError, match="op must be one of"):
        classify.logit_eval_host(g["A"], g["B"], g["u"], g["v"], g["y"], "xor", g["theta"], 0.0)
    with pytest.raises(ValueError, match="dim 3 and 32"):
        classify.logit_eval_host(g["A"], lc.matrices(32)[1], g["u"], g["v"], g["y"], "l1", g["theta"], 0.0)
    with pytest.raises(NotImplementedError, match="dim 513 is above the trainer's cap of 512"):
        classify.logit_eval_host(np.zeros((2, 513), np.float32), None, [0], [1], [1], "average", np.zeros(514), 0.0)
    with pytest.raises(ValueError, match="m must be in"):
        empty = np.array([], dtype=np.uint32)
        classify.logit_eval_host(g["A"], None, empty, empty, empty, "l1", g["theta"], 0.0)


# ---- the optimiser ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_fit():
    X, u, v, y = lc.planted()
    return classify.fit_host(X, u, v, y, "hadamard", l2=1e-3)


def test_fit_host_on_the_planted_problem(planted_fit):
    X, u, v, y = lc.planted()
    model = planted_fit
    assert model.converged and model.n_eval > model.n_iter > 3
    _, grad = lc.independent(X, None, u, v, y, "hadamard", model.theta, 1e-3)
    assert np.abs(grad).max() <= 10 * 1e-8
    assert ((model.decision_function_host(X, u, v) > 0) == (y == 1)).mean() > 0.85


def test_fit_host_against_scikit_learn(planted_fit):
    """Our objective at our theta, by the independent expression, is no larger than at scikit-learn's theta plus a margin.

    Measured: ours 0.13739471748567783, scikit-learn's 0.13739471748568916: ours is the smaller by 1.13e-14 (scikit-learn stops
    on its own tolerance a little short of the minimum).  The margin is ten times the magnitude observed, 1.2e-13.
    scikit-learn's lbfgs converges on this input (n_iter_ below max_iter, checked)."""
    linear_model = pytest.importorskip("sklearn.linear_model")
    X, u, v, y = lc.planted()
    F = X[u].astype(np.float64) * X[v].astype(np.float64)
    sk = linear_model.LogisticRegression(C=1.0 / (1e-3 * len(y)), tol=1e-10, max_iter=10000).fit(F, y)
    assert int(sk.n_iter_[0]) < 10000
    sk_theta = np.concatenate([sk.coef_[0], sk.intercept_])
    ours = lc.independent(X, None, u, v, y, "hadamard", planted_fit.theta, 1e-3)[0]
    theirs = lc.independent(X, None, u, v, y, "hadamard", sk_theta, 1e-3)[0]
    print(f"objective: ours {ours!r}, scikit-learn {theirs!r}, difference {ours - theirs:.3g}")
    assert ours <= theirs + 1.2e-13
    assert np.allclose(planted_fit.theta, sk_theta, rtol=0, atol=1e-4)


def test_model_file_and_one_vs_rest(tmp_path, planted_fit):
    path = tmp_path / "model.tsv"
    planted_fit.save(path)
    back = classify.LogisticModel.load(path)
    assert lc.same_bits(back.theta, planted_fit.theta) and lc.same_bits(back.loss, planted_fit.loss) and lc.same_bits(back.l2, planted_fit.l2)
    assert (back.op, back.converged, back.n_iter, back.n_eval) == (planted_fit.op, planted_fit.converged, planted_fit.n_iter, planted_fit.n_eval)
    assert len(path.read_text().splitlines()) == 6 + planted_fit.theta.size
    path.write_text(path.read_text() + "junk\n")
    with pytest.raises(ValueError, match="not a line of a model file"):
        classify.LogisticModel.load(path)

    rng = np.random.default_rng(3)
    X = rng.standard_normal((400, 8)).astype(np.float32)
    rows = rng.permutation(400)[:300]
    Y = ((X[rows].astype(np.float64) @ rng.standard_normal((8, 3)) + 0.4 * rng.standard_normal((300, 3))) > 0).astype(np.uint8)
    models = classify.fit_one_vs_rest_host(X, rows, Y, l2=1e-2)
    assert len(models) == 3
    for c, model in enumerate(models):
        single = classify.fit_host(X, rows, None, Y[:, c], "row", l2=1e-2)
        assert model.op == "row" and model.converged and lc.same_bits(model.theta, single.theta) and model.n_eval == single.n_eval
    with pytest.raises(ValueError, match="one row per sample"):
        classify.fit_one_vs_rest_host(X, rows, Y[:10])


@pytest.mark.skipif(_lib.load().pw_device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_no_device():
    from pecanpy_amd import embed

    case = CASES[0]
    rc, msg, *_ = lc.selftest_raw(1, case.A, case.B, case.u, case.v, case.y, 1, case.theta, 0.0)
    assert rc != 0 and "no HIP device" in msg
    with pytest.raises(_lib.PwError, match="no HIP device"):
        embed.KnnIndex(case.A)


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_cli_parser(capsys):
    from pecanpy_amd import cli

    args = cli.parse_args(["--task", "fit", "--input", "x.emb", "--pairs", "p.tsv", "--neg_pairs", "n.tsv", "--operator", "l1", "--l2_penalty", "0.5",
                           "--output", "model.tsv"])
    assert (args.task, args.operator, args.l2_penalty, args.pairs, args.neg_pairs, args.labels) == ("fit", "l1", 0.5, "p.tsv", "n.tsv", None)
    args = cli.parse_args(["--task", "fit", "--input", "x.emb", "--labels", "l.tsv", "--output", "model.tsv"])
    assert args.labels == "l.tsv" and args.operator == "hadamard" and args.l2_penalty == 1e-3
    args = cli.parse_args(["--task", "score", "--input", "x.emb", "--pairs", "p.tsv", "--model", "model.tsv", "--output", "s.tsv"])
    assert args.model == "model.tsv"
    for op in ("average", "hadamard", "l1", "l2"):
        assert cli.parse_args(["--task", "fit", "--input", "x", "--output", "m", "--pairs", "p", "--neg_pairs", "n", "--operator", op]).operator == op
    for op in ("row", "xor"):
        with pytest.raises(SystemExit):
            cli.parse_args(["--task", "fit", "--input", "x", "--output", "m", "--labels", "l", "--operator", op])
    capsys.readouterr()
    for missing in (["--task", "fit", "--input", "x.emb", "--output", "m.tsv"],
                    ["--task", "fit", "--input", "x.emb", "--pairs", "p.tsv", "--output", "m.tsv"],
                    ["--task", "fit", "--input", "x.emb", "--neg_pairs", "n.tsv", "--output", "m.tsv"],
                    ["--task", "fit", "--input", "x.emb", "--labels", "l.tsv", "--pairs", "p.tsv", "--neg_pairs", "n.tsv", "--output", "m.tsv"]):
        with pytest.raises(SystemExit):
            cli.main(missing)
        assert "--task fit needs either --labels, or --pairs together with --neg_pairs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(["--task", "fit", "--input", "x.emb", "--labels", "l.tsv"])
    assert "--output" in capsys.readouterr().err
    plain = cli.parse_args(["--input", "g.edg", "--output", "o"])
    for task in ("pecanpy", "tocsr", "todense", "walks", "train", "neighbours", "score", "split", "baseline"):   # as before
        args = cli.parse_args(["--task", task, "--input", "g.edg", "--output", "o", "--pairs", "p", "--heuristic", "jaccard"])
        assert args.task == task and args.model is None and args.labels is None
        assert (args.metric, args.topn, args.holdout_fraction, args.mode) == (plain.metric, plain.topn, plain.holdout_fraction, plain.mode)
    assert plain.task == "pecanpy"
    base = ["--input", "g.edg", "--output", "o"]
    for flags, told in ((["--operator", "l1"], "--operator belong"), (["--l2_penalty", "0.5", "--labels", "l"], "--labels, --l2_penalty belong"),
                        (["--model", "m.tsv"], "--model belongs to --task score"),
                        (["--task", "score", "--pairs", "p", "--model", "m.tsv", "--metric", "dot"], "--metric is ignored"),
                        (["--task", "fit", "--labels", "l", "--operator", "l2"], "--operator is ignored")):   # a misapplied flag is told
        with pytest.warns(UserWarning, match=told):
            cli.parse_args(base + flags)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # and the right uses are silent
        cli.parse_args(base + ["--task", "score", "--pairs", "p", "--model", "m.tsv"])
        cli.parse_args(base + ["--task", "fit", "--pairs", "p", "--neg_pairs", "n", "--operator", "l2", "--l2_penalty", "0.1"])
        cli.parse_args(base + ["--task", "score", "--pairs", "p", "--metric", "dot"])
    assert "--task fit" in cli.__doc__ and "--model" in cli.__doc__ and "--labels" in cli.__doc__
