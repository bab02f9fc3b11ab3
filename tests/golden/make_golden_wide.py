#!/usr/bin/env python3
"""Reference-generated fixtures on wide-range weights (tests/wide_weight_cases.py), through the machinery of make_golden.py
as it is (stubs, ``SeqArray``): ``wide_*.npz``, each the 64-vertex R-MAT with 2 x 64 walks of 12 steps.

Every case records in ``ref_warnings`` the categories and messages of the warnings the reference raised under NumPy (the
``huge`` case: float32 overflow in the sequential row total, which Numba does not report); a case on which the reference
raises writes no fixture and prints the exception.

usage:  python tests/golden/make_golden_wide.py
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402
import wide_weight_cases as wc  # noqa: E402

# Not a case: node2vec+ on ``loguniform``.  The reference's own ``get_noise_thresholds`` overflows in float32 there (NumPy:
# "overflow encountered in multiply", "invalid value encountered in multiply") and returns NaN thresholds for rows that are
# walked; what a comparison with NaN and a search over a CDF of NaNs mean differs between NumPy and Numba, so there is no
# reference to pin.  The GPU tests take their thresholds from the project's ``get_noise_thresholds`` with NaN -> 0 instead.
DROPPED = ("wide_loguniform_SparseOTF_n2vplus_p0.3_q1.7",)

# name, mode, family, p, q, extend
CASES = [
    ("wide_loguniform_SparseOTF_n2v_p0.5_q2", "SparseOTF", "loguniform", 0.5, 2, False),
    ("wide_spike_SparseOTF_n2v_p0.5_q2", "SparseOTF", "spike", 0.5, 2, False),
    ("wide_spike_SparseOTF_n2vplus_p0.5_q2", "SparseOTF", "spike", 0.5, 2, True),
    ("wide_moderate_PreComp_n2v_p0.5_q2", "PreComp", "moderate", 0.5, 2, False),
    ("wide_loguniform64_DenseOTF_n2v_p0.5_q2", "DenseOTF", "loguniform64", 0.5, 2, False),
    ("wide_huge_SparseOTF_n2v_p0.5_q2", "SparseOTF", "huge", 0.5, 2, False),
]


def csr_of_dense(a):
    n = a.shape[0]
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum((a != 0).sum(axis=1))
    r, c = np.nonzero(a)
    return indptr, c.astype(np.uint32), a[r, c].copy()


def main():
    for name, mode, family, p, q, extend in CASES:
        if family.endswith("64"):
            indptr, indices, data = csr_of_dense(wc.dense(family, True, n=64, density=0.15))
        else:
            indptr, indices, data = wc.graph("rmat6", family)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            try:
                mg.walk_case(name, mode, indptr, indices, data, p, q, extend, 0.0, wc.SEED, 2, 12,
                             n_prob_samples=0 if mode == "DenseOTF" else 40)
            except Exception as e:  # noqa: BLE001 (the reference's own behaviour on this input: reported, no fixture)
                print(f"{name}: the reference raised {type(e).__name__}: {e}")
                continue
        seen = sorted({f"{w.category.__name__}: {w.message}" for w in rec})
        print(f"{name}: {len(rec)} warnings {seen}")
        path = os.path.join(HERE, name + ".npz")
        z = dict(np.load(path))
        z["ref_warnings"] = np.array(seen, dtype=str)
        np.savez_compressed(path, **z)


if __name__ == "__main__":
    main()
