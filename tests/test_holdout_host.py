"""Edge hold-out without a GPU: the host build of the definition (csrc/holdout.hip.h through ``pw_selftest_holdout_edges`` with
``on_device = 0``) against the plain-loop statement ``linkpred.holdout_edges_host`` on every case of tests/holdout_cases.py,
array for array; the properties the definition promises; the refusal of a CSR that is not symmetric; the threshold."""
import math
from fractions import Fraction

import numpy as np
import pytest

import holdout_cases as hc
from pecanpy_amd import _lib, linkpred

GRAPHS = list(hc.graphs())


@pytest.mark.parametrize("name", GRAPHS)
def test_host_build_equals_the_statement(name):
    graph = hc.graphs()[name]
    for fraction, protect, first_word in hc.parameter_sets():
        got = hc.selftest(graph, fraction, protect, first_word, on_device=0)
        assert got.rc == 0, hc.last_error()
        assert hc.equals_statement(got, name, fraction, protect, first_word), (fraction, protect, first_word)


def _entries(indptr, indices):
    """The ordered pairs of a CSR, in entry order."""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr.astype(np.int64)))
    return list(zip(rows.tolist(), indices.tolist()))


@pytest.mark.parametrize("name", GRAPHS)
def test_the_promised_properties_hold(name):
    indptr, indices, data, directed = graph = hc.graphs()[name]
    weights = np.ones(indices.size, dtype=np.float32) if data is None else data
    original = _entries(indptr, indices)
    position = {rc: e for e, rc in enumerate(original)}
    for fraction, protect, first_word in hc.parameter_sets():
        got = hc.selftest(graph, fraction, protect, first_word, on_device=0)
        assert got.rc == 0, hc.last_error()
        (t_indptr, t_indices, t_data), (u, v, w) = got.train, got.held
        kept, held, units, protected = got.counts
        train = _entries(t_indptr, t_indices)
        held_pairs = list(zip(u.tolist(), v.tolist()))
        # train + held (both entries of an undirected unit) is the original, nothing twice; weights are the entries' own
        gone = held_pairs if directed else held_pairs + [(b, a) for a, b in held_pairs]
        assert len(train) == kept and len(held_pairs) == held and len(set(train)) == kept and len(set(gone)) == len(gone)
        train_set = set(train)
        assert not train_set & set(gone) and sorted(train + gone) == original
        assert train == [rc for rc in original if rc in train_set]   # in order: rows still ascending
        assert np.array_equal(t_data.view(np.uint32), weights[[position[rc] for rc in train]].view(np.uint32))
        assert np.array_equal(w.view(np.uint32), weights[[position[rc] for rc in held_pairs]].view(np.uint32))
        places = [position[rc] for rc in held_pairs]
        assert places == sorted(places) and all(a != b for a, b in held_pairs)   # ascending unit position; loops stay
        if not directed:
            assert all(a < b for a, b in held_pairs) and train_set == {(b, a) for a, b in train}   # u < v; train symmetric
        if protect:   # every row that had a non-loop entry keeps one
            had = {a for a, b in original if a != b}
            assert had == {a for a, b in train if a != b}
        else:
            assert protected == 0
        assert units == sum(1 for a, b in original if a != b and (directed or a < b))
        if fraction == 0:   # the input bit for bit, an empty list
            assert held == 0 and hc.same_arrays(got.train, (indptr, indices, weights))
        if fraction == hc.FRACTIONS[-1]:   # threshold 2^32 - 1: every unit that is not protected goes
            assert held == units - protected
            assert sum(1 for a, b in train if a != b and (directed or a < b)) == protected


def test_protection_is_by_the_first_non_loop_entry():
    """The self-loop graph by hand.  Rows: 0 = [0, 1, 2], 1 = [0, 2], 2 = [0, 1, 2, 3], 3 = [2, 4], 4 = [3], 5 = [5].  Units
    (0,1) (0,2) (1,2) (2,3) (3,4).  f(0) = position 1, the entry behind the loop: (0,1) is protected, and it is f(1) as well;
    (0,2) is f(2) seen from its mate; (1,2) is protected by neither row; (2,3) is f(3) seen from its mate; (3,4) is f(4)."""
    graph = hc.graphs()["self-loops"]
    got = hc.selftest(graph, hc.FRACTIONS[-1], True, 0, on_device=0)
    assert got.rc == 0 and got.counts == (3 + 2 * 4, 1, 5, 4)
    assert got.held[0].tolist() == [1] and got.held[1].tolist() == [2] and got.held[2].tolist() == [hc._asymmetric(1, 2)]
    assert got.train[0].tolist() == [0, 3, 4, 7, 9, 10, 11] and got.train[1].tolist() == [0, 1, 2, 0, 0, 2, 3, 2, 4, 3, 5]
    bare = hc.selftest(graph, hc.FRACTIONS[-1], False, 0, on_device=0)   # without protection only the loops stay
    assert bare.counts == (3, 5, 5, 0) and bare.train[0].tolist() == [0, 1, 1, 2, 2, 2, 3] and bare.train[1].tolist() == [0, 2, 5]


@pytest.mark.parametrize("first_word", hc.FIRST_WORDS)
def test_half_the_free_units_are_held_out(first_word):
    """fraction 0.5 on the random graph: the held count within six standard deviations of Binomial(units - protected, 0.5) -- a
    comparison with the wrong sense, the wrong width or the wrong word would not pass."""
    for seed in (hc.SEED, hc.SEED + 1):
        got = hc.selftest(hc.graphs()["er-700"], Fraction(1, 2), True, first_word, on_device=0, seed=seed)
        assert got.rc == 0
        _, held, units, protected = got.counts
        free = units - protected
        assert free > 3000 and abs(held - free / 2) <= 6 * math.sqrt(free / 4), (held, free)


def test_seeds_and_offsets_give_other_splits_and_the_next_offset_continues():
    graph = hc.graphs()["er-700"]
    nnz = graph[1].size
    a = hc.selftest(graph, Fraction(1, 2), True, 0, on_device=0)
    b = hc.selftest(graph, Fraction(1, 2), True, 0, on_device=0, seed=hc.SEED + 1)
    c = hc.selftest(graph, Fraction(1, 2), True, nnz, on_device=0)
    assert not hc.same_arrays(a.held[:2], b.held[:2]) and not hc.same_arrays(a.held[:2], c.held[:2])
    train, held, used = linkpred.holdout_edges_host(*graph[:3], Fraction(1, 2), hc.SEED, first_word=nnz)
    assert used == nnz and hc.same_arrays(c.train, train) and hc.same_arrays(c.held, held)


def test_a_csr_without_a_mate_is_refused_and_nothing_is_written():
    got = hc.selftest(hc.MISSING_MATE, Fraction(1, 2), True, 0, on_device=0)
    assert got.rc == _lib.ERR_INVALID and f"position {hc.MISSING_AT} has no mate".encode() in hc.last_error(), hc.last_error()
    assert got.untouched()
    with pytest.raises(ValueError, match=f"position {hc.MISSING_AT} has no mate"):
        linkpred.holdout_edges_host(*hc.MISSING_MATE[:3], Fraction(1, 2), hc.SEED)
    as_directed = hc.selftest(hc.MISSING_MATE, Fraction(1, 2), True, 0, on_device=0, directed=True)   # the same arrays, directed: fine
    train, held, _ = linkpred.holdout_edges_host(*hc.MISSING_MATE[:3], Fraction(1, 2), hc.SEED, directed=True)
    assert as_directed.rc == 0 and hc.same_arrays(as_directed.train, train) and hc.same_arrays(as_directed.held, held)


def test_the_threshold_is_exact_integer_arithmetic():
    assert [linkpred.holdout_threshold(f) for f in hc.FRACTIONS] == [0, 2 ** 31, 2 ** 32 - 1]
    assert linkpred.holdout_threshold(0.5) == 2 ** 31 and linkpred.holdout_threshold(0.1) == int(Fraction(0.1) * 2 ** 32)
    assert linkpred.holdout_threshold(Fraction(1, 3)) == (2 ** 32) // 3
    for bad in (1, 1.5, -0.25, Fraction(-1, 2 ** 40)):
        with pytest.raises(ValueError, match="fraction"):
            linkpred.holdout_threshold(bad)


def test_the_names_are_public_and_split_is_a_task():
    from pecanpy_amd import cli, pecanpy as node2vec

    assert {"holdout_edges", "holdout_edges_host"} <= set(linkpred.__all__)
    assert callable(node2vec.SparseOTF.holdout_edges)
    args = cli.parse_args(["--input", "g.edg", "--output", "train.npz", "--task", "split", "--pairs", "held.tsv"])
    assert args.holdout_fraction == 0.5 and not args.no_protect and args.neg_pairs is None
    with pytest.raises(SystemExit):
        cli.parse_args(["--input", "g.edg", "--output", "train.npz", "--task", "split"])   # no --pairs
