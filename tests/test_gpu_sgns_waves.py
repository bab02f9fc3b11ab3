"""The PARALLEL form of the skip-gram trainer (csrc/sgns.hip.h: several wavefronts, several workgroups -- what ``workers=0``,
``Base.embed`` and the command line run) held to the sequential restatement exactly.

Two yardsticks, neither with a tolerance of its own (tests/sgns_corpora.py, tests/test_sgns_order_host.py):

* on a component corpus with ``negative=0`` no two wavefronts touch the same row and every wavefront visits its walks in
  sentence order, so the vectors equal those of ``workers=1`` BIT FOR BIT, and the restatement within the one-wavefront bound
  ``2e-5 * max|want| + 1e-6`` of tests/test_gpu_sgns.py (same arithmetic per row);
* ``kept_occurrences`` and ``trained_pairs`` are hashes of (seed, epoch, walk, position): they equal the restatement's counts
  in ANY run, a racing one with negatives included.

Every row of ``WAVE_CASES`` is built for the wavefront count its ``workers`` must become, and that count is asserted first:
with another rounding two wavefronts would share a component and race."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from pecanpy_amd.embed import train_sgns, train_sgns_device
from pecanpy_amd.engine import PwError
from sgns_corpora import (SEED, WAVE_CASES, case_corpus, case_kw, close_to_oracle, component_corpus,
                          held_to_one_wavefront_and_the_restatement, karate_walks, on_device, run)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", WAVE_CASES, ids=[c["id"] for c in WAVE_CASES])
def test_several_wavefronts_equal_one_on_a_component_corpus(case):
    mat, n = case_corpus(case)
    held_to_one_wavefront_and_the_restatement(mat, n, case_kw(case), case["workers"], case["wavefronts"])


def test_default_launch_rule_equals_one_wavefront_through_both_entries():
    """``workers=0``: a component per walk is free of races for any wavefront count.  71 cells per walk: a wavefront owns
    ``ceil(256 / 71) = 4`` walks."""
    mat, n = component_corpus(40, 40, 70, seed=40)
    kw = dict(dim=24, window=5, epochs=3, sample=0.05, negative=0, seed=SEED)
    got = held_to_one_wavefront_and_the_restatement(mat, n, kw, workers=0)
    assert np.array_equal(train_sgns(mat, n, workers=0, **kw), got)         # the host-matrix entry: same launch, same bits


@pytest.mark.parametrize("workers", [0, 8])
def test_counters_of_a_racing_run_equal_the_restatement(workers):
    """With negatives the vectors of a parallel run are comparable only statistically (tests/test_gpu_sgns.py); which
    occurrences survive and how many pairs each trains do not depend on the race."""
    mat, n = karate_walks(40, 40, seed=3)
    kw = dict(dim=16, window=5, epochs=3, sample=1e-3, negative=5, seed=5)
    counts = orc.sgns_train(mat, n, return_counts=True, **kw)[2]
    got, st = run(on_device(mat), n, workers=workers, **kw)
    print(f"wavefronts {st['wavefronts']}, kept {st['kept_occurrences']}, pairs {st['trained_pairs']} (restatement {counts})")
    assert st["wavefronts"] > 1 and (workers == 0 or st["wavefronts"] == workers)
    assert (st["kept_occurrences"], st["trained_pairs"]) == counts
    assert 0 < counts[0] < 3 * int(mat[:, -1].sum())                        # thinned
    assert np.isfinite(got).all()


def test_walk_length_8192_is_refused_and_the_next_call_succeeds():
    """``2 * 4 * (L + 1)`` bytes of LDS per wavefront: 8191 is the last length that fits 64 KiB."""
    import torch

    d_walks = torch.zeros((2, 8192 + 2), dtype=torch.int32, device="cuda")
    d_walks[:, -1] = 5
    with pytest.raises(PwError, match="below 8192"):
        train_sgns_device(d_walks, 4, dim=8, window=3, epochs=1, seed=1, workers=2)
    mat, n = component_corpus(4, 12, 30, seed=3)
    kw = dict(dim=8, window=3, epochs=2, sample=0.0, seed=SEED)           # negatives: one wavefront, sentence order
    want, _, counts = orc.sgns_train(mat, n, return_counts=True, **kw)
    got, st = run(on_device(mat), n, workers=1, **kw)
    close_to_oracle(got, want)
    assert (st["kept_occurrences"], st["trained_pairs"]) == counts
