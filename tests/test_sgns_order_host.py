"""(CPU) The yardstick the multi-wavefront skip-gram trainer is held to, shown on the restatement itself.

csrc/sgns.hip.h: the SET of updates is a function of the seed alone, the hardware adds only their ORDER.  On a component
corpus (tests/sgns_corpora.py) with ``negative=0`` no two components share a row, so every visiting order that keeps the
walks of each component in ascending order -- the wavefront-major one, and any random interleaving of the components --
gives the sentence-order vectors bit for bit (reordering the walks INSIDE a component does not: a control).  ``oracle/sgns_ref.c`` takes the visiting order as
an argument (``order``); the hashes and the learning-rate position keep the walk's own index.  With negatives the noise
table crosses components and the orders differ: that control also fails if ``order`` is ignored.  The two counters
(occurrences kept, pairs trained) are hashes of (seed, epoch, walk, position) and equal in ANY order; one small corpus pins
them to a NumPy evaluation of those hashes."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from sgns_corpora import SEED, WAVE_CASES, case_corpus, case_kw, component_corpus, counts_by_numpy, wavefront_major

IDS = [c["id"] for c in WAVE_CASES]
# so few occurrences survive sample=1e-3 on these two (9 and 338) that no vector moves by the initial range
LIGHTLY_TRAINED = {"many-walks-per-wavefront", "idle-wavefronts"}


def initial_vectors(mat, n, case):
    """syn0 before the first update: a run whose learning rate is zero."""
    return orc.sgns_train(mat, n, **case_kw(case, epochs=1, alpha=0.0, min_alpha=0.0))[0]


def component_preserving_permutation(rng, n_walks, n_components):
    """A random interleaving of the components that keeps the walks of each in ascending order."""
    queues = [list(range(c, n_walks, n_components)) for c in range(n_components)]
    tags = rng.permutation(np.repeat(np.arange(n_components), [len(q) for q in queues]))
    return np.array([queues[c].pop(0) for c in tags], dtype=np.uint64)


@pytest.mark.parametrize("case", WAVE_CASES, ids=IDS)
def test_order_cannot_matter_on_a_component_corpus(case):
    mat, n = case_corpus(case)
    want, _, counts = orc.sgns_train(mat, n, return_counts=True, **case_kw(case))
    occurrences = case["epochs"] * int(mat[:, -1].sum())
    assert 0 < counts[0] <= occurrences and counts[1] > 0
    if case["sample"] == 0.0:
        assert counts[0] == occurrences
    if case["sample"] == 0.05:
        assert counts[0] < 0.96 * occurrences                               # thins visibly
    # trained, not two copies of the initial noise
    moved = np.abs(want - initial_vectors(mat, n, case)).max()
    print(f"{case['id']}: kept {counts[0]} of {occurrences}, {counts[1]} pairs, moved {moved * case['dim'] / 0.5:.2f} initial ranges")
    assert moved > (0.0 if case["id"] in LIGHTLY_TRAINED else 0.5 / case["dim"])
    rng = np.random.default_rng(5)
    orders = [wavefront_major(case["walks"], case["wavefronts"])]
    orders += [component_preserving_permutation(rng, case["walks"], case["wavefronts"]) for _ in range(3)]
    if case["walks"] <= case["wavefronts"]:                                 # a component per walk: any permutation will do
        orders.append(rng.permutation(case["walks"]).astype(np.uint64))
    assert sum(not np.array_equal(order, np.arange(case["walks"])) for order in orders) >= 2
    for order in orders:
        assert sorted(order) == list(range(case["walks"]))
        got, _, got_counts = orc.sgns_train(mat, n, order=order, return_counts=True, **case_kw(case))
        assert np.array_equal(got, want) and got_counts == counts


@pytest.mark.parametrize("case", [c for c in WAVE_CASES if c["id"] not in LIGHTLY_TRAINED],
                         ids=[i for i in IDS if i not in LIGHTLY_TRAINED])
def test_with_negatives_the_order_matters(case):
    """Control: the noise table crosses components, so the wavefront-major order gives other vectors -- and the same counts.
    Fails if ``order`` is ignored."""
    mat, n = case_corpus(case)
    kw = case_kw(case, negative=5)
    want, _, counts = orc.sgns_train(mat, n, return_counts=True, **kw)
    got, _, got_counts = orc.sgns_train(mat, n, order=wavefront_major(case["walks"], case["wavefronts"]), return_counts=True, **kw)
    assert not np.array_equal(got, want)
    assert np.abs(got - want).max() > 1e-3 * np.abs(want).max()             # not a rounding difference
    assert got_counts == counts == orc.sgns_train(mat, n, return_counts=True, **case_kw(case))[2]   # negatives add no pair


def test_an_arbitrary_permutation_matters_inside_a_component():
    """Control of the construction: walks of ONE component visited in another order give other vectors even without
    negatives, so the equalities above are those of the component structure, not of an order that is never applied."""
    case = WAVE_CASES[0]
    mat, n = case_corpus(case)
    want, _, counts = orc.sgns_train(mat, n, return_counts=True, **case_kw(case))
    got, _, got_counts = orc.sgns_train(mat, n, order=np.arange(case["walks"])[::-1], return_counts=True, **case_kw(case))
    assert not np.array_equal(got, want) and got_counts == counts


def test_default_order_and_old_entry_point_are_unchanged():
    case = WAVE_CASES[0]
    mat, n = case_corpus(case)
    kw = case_kw(case, negative=5)
    plain = orc.sgns_train(mat, n, **kw)
    assert len(plain) == 2
    same = orc.sgns_train(mat, n, order=np.arange(case["walks"]), return_counts=True, **kw)
    assert np.array_equal(plain[0], same[0]) and plain[1] == same[1]
    for bad in (np.zeros(case["walks"]), np.arange(case["walks"]) + 1):    # not a permutation
        with pytest.raises(ValueError):
            orc.sgns_train(mat, n, order=bad, **kw)
    with pytest.raises(ValueError):
        orc.sgns_train(mat, n, order=np.arange(case["walks"] - 1), **kw)


@pytest.mark.parametrize("sample,window,epochs", [(0.05, 5, 3), (1e-3, 3, 2), (0.0, 4, 1)])
def test_counts_equal_a_numpy_evaluation_of_the_two_hashes(sample, window, epochs):
    mat, n = component_corpus(4, 37, 70, seed=92)
    want = counts_by_numpy(mat, n, window, epochs, sample, SEED)
    for negative in (0, 5):
        got = orc.sgns_train(mat, n, dim=8, window=window, epochs=epochs, sample=sample, negative=negative, seed=SEED,
                             return_counts=True)[2]
        assert got == want
    occurrences = epochs * int(mat[:, -1].sum())
    assert want[0] == occurrences if sample == 0.0 else want[0] < 0.96 * occurrences


def test_component_corpus_is_what_it_says():
    for case in WAVE_CASES:
        mat, n = case_corpus(case)
        L, nc = case["L"], case["wavefronts"]
        assert mat.dtype == np.uint32 and mat.shape == (case["walks"], L + 2) and n == nc * 6
        lengths = mat[:, -1]
        assert lengths.max() <= L + 1 and (L + 1 <= 64 or (lengths > 64).any())
        if case["lengths"] is None:
            assert set(lengths) <= {0, 1, 2, L // 2, L, L + 1}
        assert (lengths == 0).any() and (lengths == 1).any()
        for wk, row in enumerate(mat):
            assert (row[:lengths[wk]] // 6 == wk % nc).all()                # the ids that count: its own component
            assert (row[lengths[wk]:L + 1] // 6 == (wk + 1) % nc).all()     # past the length: valid ids of another one
