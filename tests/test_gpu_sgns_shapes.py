"""The ARITHMETIC of the skip-gram trainer (csrc/sgns.hip.h) across its template and group space: every
``sgns_walk_kernel<PER>`` at the low edge, inside and at the high edge of its range of ``dim``, ``negative + 1`` targets
filling the groups of six in every way, both saturated branches of the sigmoid, a noise table above its floor, another
schedule, subsampling at a wide instance (tests/sgns_shape_cases.py; what each case reaches is asserted on the CPU in
tests/test_sgns_shapes_host.py).

One wavefront in sentence order against two references:

* the float32 restatement in the kernel's lane order (oracle/sgns_ref.c) within the project's one-wavefront bound
  ``B(w) = 2e-5 * max|w| + 1e-6``;
* the float64 evaluation (tests/sgns_f64.py) within ``e_ref + B(want64)``: ``e_ref = max|want32 - want64|`` is the
  restatement's own distance from float64, recomputed here, and the kernel gets one more unit of the same bound for its fused
  multiply-adds and fast ``exp``.  The printed ratio is a finding, not a number to tune.

Both counters equal the references', a second call is bit-equal, and every row whose id occurs in no walk -- such an id lies
directly after a used one in every case -- keeps the bits of its seeded initial value: a store through a wrong lane guard
would land there."""
import numpy as np
import pytest

from pecanpy_amd.embed import train_sgns
from sgns_corpora import close_to_oracle, held_to_one_wavefront_and_the_restatement, on_device, run
from sgns_shape_cases import BY_ID, HOST_ENTRY, ONE_WAVEFRONT, bound, per_of, reference

pytestmark = pytest.mark.gpu


def held_to_both_references(got, ref):
    close_to_oracle(got, ref["want32"])
    err, limit = np.abs(got - ref["want64"]).max(), ref["e_ref"] + bound(ref["want64"])
    print(f"max|got - want64| = {err:.3e}, e_ref {ref['e_ref']:.3e}, bound {limit:.3e}, ratio {err / limit:.3f}")
    assert err <= limit, (err, limit)
    assert np.isfinite(got).all()
    unused = ref["unused"]
    touched = unused[(got[unused] != ref["initial"][unused]).any(axis=1)]
    assert touched.size == 0, f"rows {touched[:8]} of ids that occur in no walk were written"


@pytest.mark.parametrize("case_id", ONE_WAVEFRONT)
def test_one_wavefront_equals_both_references(case_id):
    ref = reference(case_id)
    d_walks = on_device(ref["mat"])
    got, st = run(d_walks, ref["n"], workers=1, **ref["kw"])
    print(f"dim {ref['kw']['dim']} (PER {per_of(ref['kw']['dim'])}), negative {ref['kw']['negative']}, "
          f"kept {st['kept_occurrences']}, pairs {st['trained_pairs']}")
    assert st["wavefronts"] == 1
    held_to_both_references(got, ref)
    assert (st["kept_occurrences"], st["trained_pairs"]) == ref["counts32"] == (ref["diag"]["kept"], ref["diag"]["pairs"])
    again, st2 = run(d_walks, ref["n"], workers=1, **ref["kw"])
    assert np.array_equal(again, got)
    assert (st2["kept_occurrences"], st2["trained_pairs"]) == ref["counts32"]
    assert np.array_equal(d_walks.cpu().numpy().view(np.uint32), ref["mat"])                      # read, never written


@pytest.mark.parametrize("case_id", HOST_ENTRY)
def test_host_matrix_entry_equals_both_references(case_id):
    """One case per instance through ``train_sgns`` (upload, the same launch, download)."""
    ref = reference(case_id)
    held_to_both_references(train_sgns(ref["mat"], ref["n"], workers=1, **ref["kw"]), ref)


def test_four_wavefronts_at_a_wide_instance_equal_one():
    """``PER = 6`` at its low edge (one live lane in the last component) in the parallel form: a component per wavefront and
    no negatives, so the vectors equal those of ``workers=1`` bit for bit."""
    case, ref = BY_ID["four-wavefronts-dim-321"], reference("four-wavefronts-dim-321")
    got = held_to_one_wavefront_and_the_restatement(ref["mat"], ref["n"], ref["kw"], case["workers"], case["wavefronts"])
    held_to_both_references(got, ref)
