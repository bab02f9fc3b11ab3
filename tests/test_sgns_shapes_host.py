"""(CPU) The cases of tests/sgns_shape_cases.py before the kernel sees them: each one reaches the path it is for, and the
float32 restatement the kernel is compared with (oracle/sgns_ref.c) is itself near an independent float64 evaluation of the
algorithm (tests/sgns_f64.py).

Reach conditions are counts from the float64 reference's diagnostics, not tolerances: a group case that never evaluates a
draw of index >= 6, or a saturation case whose dot products stay inside (-6, 6), would pass whatever the kernel does there.
The sigmoid jumps by 2.5e-3 at +-6, so a saturation case must keep 1e-2 away from the border in float64 and the float32
restatement must take each saturated branch exactly as often: then rounding cannot decide a branch in either reference.

``e_ref = max|want32 - want64|`` is the restatement's own error; it is held to the project's one-wavefront bound
``2e-5 * max|want64| + 1e-6``, which the GPU comparison with ``want64`` then inherits (MEASUREMENTS.md, "Skip-gram trainer
across its instances": the table this file prints)."""
import numpy as np
import pytest

from sgns_corpora import counts_by_numpy
from sgns_shape_cases import BY_ID, CASES, EDGE_DIMS, HOST_ENTRY, IDS, bound, per_of, reference


@pytest.mark.parametrize("case_id", IDS)
def test_case_reaches_its_path_and_the_restatement_is_near_float64(case_id):
    case, ref = BY_ID[case_id], reference(case_id)
    d, kw, reach = ref["diag"], ref["kw"], case["reach"]
    dim = kw["dim"]
    ratio = ref["e_ref"] / bound(ref["want64"])
    moved = np.abs(ref["want64"] - ref["initial"])[:, 64 * (per_of(dim) - 1):].max()
    print(f"| {case_id} | {dim} | {per_of(dim)} | {kw['negative']} | {d['kept']}/{d['occurrences']} | {d['pairs']} | "
          f"{d['second_group_evaluations']} | {d['in_group_repeats']}/{d['cross_group_repeats']} | {d['skipped_draws']} | "
          f"{d['saturated_high']}/{d['saturated_low']} | {d['margin']:.3f} | {np.abs(ref['want64']).max():.3g} | "
          f"{ref['e_ref']:.2e} | {ratio:.3f} |")
    # the case is small, and it trains
    assert 0 < d["pairs"] <= 3000
    assert ref["unused"].size and (np.isin(ref["unused"] - 1, ref["unused"], invert=True)).any()   # an unused id after a used one
    # the last component slot of a lane moves by far more than the bound: an instance that dropped it would be seen
    assert moved > 20 * bound(ref["want64"]), (moved, bound(ref["want64"]))
    # reach conditions
    if "small_vocab" in reach:
        assert d["skipped_draws"] > 0
        assert kw["negative"] < 2 or d["in_group_repeats"] > 0
    if "second_group" in reach:
        assert kw["negative"] >= 6 and d["second_group_evaluations"] > 0 and d["cross_group_repeats"] > 0
    else:
        assert d["second_group_evaluations"] == 0
    if "sat_low" in reach:
        assert d["saturated_low"] >= 20
    if "sat_high" in reach:
        assert d["saturated_high"] >= 20
    if reach & {"sat_low", "sat_high"}:
        assert d["margin"] >= 1e-2
        assert np.abs(ref["want64"]).max() < 4.0                            # (no diverging configuration: the initial scale is 0.5 / dim)
    assert ref["saturated32"] == (d["saturated_high"], d["saturated_low"])  # the same branches in both references
    if "thinned" in reach:
        assert d["kept"] < 0.9 * d["occurrences"]
    else:
        assert d["kept"] == d["occurrences"]
    # the counters: both references and the NumPy evaluation of the two hashes
    counts = counts_by_numpy(ref["mat"], ref["n"], kw["window"], kw["epochs"], kw["sample"], kw["seed"])
    assert counts == ref["counts32"] == (d["kept"], d["pairs"])
    # the restatement against float64
    assert np.isfinite(ref["want32"]).all() and np.isfinite(ref["want64"]).all()
    assert np.array_equal(ref["want32"][ref["unused"]], ref["initial"][ref["unused"]])
    assert np.array_equal(ref["want64"][ref["unused"]], ref["initial"][ref["unused"]].astype(np.float64))
    assert ref["e_ref"] <= bound(ref["want64"]), (ref["e_ref"], bound(ref["want64"]))


def test_the_table_covers_the_template_and_group_space():
    dims = {}
    for case in CASES:
        if case["workers"] == 1:
            dims.setdefault(per_of(case["kw"]["dim"]), set()).add(case["kw"]["dim"])
    for per in range(1, 9):
        lo, hi = 64 * (per - 1) + 1, 64 * per
        assert {lo, hi} <= dims[per] and any(lo < x < hi for x in dims[per]), (per, sorted(dims[per]))
    assert set(EDGE_DIMS) >= {1, 2, 63, 511}
    assert sorted(per_of(BY_ID[i]["kw"]["dim"]) for i in HOST_ENTRY) == list(range(1, 9))   # the host-matrix entry: every instance
    negatives = {c["kw"]["negative"] for c in CASES}
    assert negatives >= {0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13}
    assert any(c["kw"]["negative"] in (6, 12) and per_of(c["kw"]["dim"]) >= 3 for c in CASES)
    assert reference("table-above-its-floor")["n"] >= 5000
    wide = BY_ID["four-wavefronts-dim-321"]
    assert wide["wavefronts"] == 4 and wide["kw"]["negative"] == 0


def test_float64_reference_is_deterministic_and_quick():
    import time

    import sgns_f64

    ref = reference("negative-13")
    t = time.perf_counter()
    again, diag = sgns_f64.train(ref["mat"], ref["n"], **ref["kw"])
    t = time.perf_counter() - t
    print(f"{diag['pairs']} pairs, {diag['evaluations']} evaluations in {t:.2f} s")
    assert np.array_equal(again, ref["want64"]) and diag == ref["diag"]
    assert t < 5.0   # (well under a second per thousand pairs on an idle machine; the limit only catches a per-component loop)
