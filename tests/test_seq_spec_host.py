"""The seeded alias / first-order modes without a GPU: the raw stream words (``pw_mt_words``) against NumPy, and the
speculation rounds' plan / candidate / resolve / commit logic in its host build (``pw_selftest_seq_offsets``,
csrc/seq_spec.h + seq_spec_host.hpp) against the plain sequential loop: the word offset at which every job starts.  The
sequential loop's words per job are held to NumPy's own ``randint``, and all three modes' rows and counters
(``pw_selftest_seq_walks`` on the oracle's alias tables) to the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import seq_spec_cases as sc
from oracle import pyoracle as orc
from pecanpy_amd import _lib
from pecanpy_amd._lib import PwSeqConfig, PwSeqInfo

L, WALKS, SEED = 30, 3, 4


def mt_words(seed, offset, n):
    out = np.zeros(n, dtype=np.uint32)
    _lib.check(_lib.load().pw_mt_words(seed, offset, n, C.c_void_p(out.ctypes.data)))
    return out


def numpy_words(seed, offset, n):
    """NumPy hands out the raw words: ``randint(0, 2**32, dtype=np.uint64)`` takes one word per value."""
    rs = np.random.RandomState(seed)
    if offset > 10**6:
        rs._bit_generator.random_raw(offset, output=False)    # the same words, generated and dropped
        offset = 0
    return rs.randint(0, 2**32, size=offset + n, dtype=np.uint64)[offset:].astype(np.uint32)


def test_numpy_raw_words_are_the_words_of_random_sample():
    w = numpy_words(4, 0, 2000).astype(np.uint64)
    want = np.random.RandomState(4).random_sample(1000)
    assert np.array_equal(((w[0::2] >> 5) * 2.0**26 + (w[1::2] >> 6)) / 2.0**53, want)


@pytest.mark.parametrize("seed", sc.STREAM_SEEDS)
@pytest.mark.parametrize("offset", sc.STREAM_OFFSETS)
def test_mt_words_match_numpy(seed, offset):
    n = 1300 if offset < 10**6 else 64        # (more than two blocks from the shallow offsets)
    assert np.array_equal(mt_words(seed, offset, n), numpy_words(seed, offset, n))


def offsets(graph, starts, cfg):
    indptr, indices, _ = graph
    c = PwSeqConfig()
    for k, v in cfg.items():
        setattr(c, k, v)
    out = np.zeros(starts.size + 1, dtype=np.uint64)
    info = PwSeqInfo()
    _lib.check(_lib.load().pw_selftest_seq_offsets(
        C.c_void_p(indptr.ctypes.data), C.c_void_p(indices.ctypes.data), indptr.size - 1, C.c_void_p(starts.ctypes.data),
        starts.size, L, SEED, C.byref(c), C.c_void_p(out.ctypes.data), C.byref(info)))
    return out, info.as_dict()


def starts_of(graph, walks=WALKS):
    n = graph[0].size - 1
    return np.random.RandomState(SEED).permutation(np.tile(np.arange(n, dtype=np.uint32), walks))


_sequential = {}


def sequential(name):
    """The reference of every comparison, computed once per graph and not touched after."""
    if name not in _sequential:
        graph = sc.GRAPHS[name]()
        starts = starts_of(graph)
        off, info = offsets(graph, starts, dict(min_jobs=sc.ONE_LANE))
        assert info["committed_jobs"] == starts.size and off[-1] == info["words_consumed"]
        off.setflags(write=False)
        _sequential[name] = (graph, starts, off)
    return _sequential[name]


@pytest.mark.parametrize("cfg", list(sc.ADVERSE), ids=list(sc.ADVERSE))
@pytest.mark.parametrize("name", list(sc.GRAPHS))
def test_speculative_offsets_equal_sequential(name, cfg):
    graph, starts, want = sequential(name)
    got, info = offsets(graph, starts, dict(sc.ADVERSE[cfg], min_jobs=1))
    assert np.array_equal(got, want)
    assert info["path"] == 1
    assert got[-1] == info["words_consumed"]
    assert info["committed_jobs"] == starts.size
    assert info["rounds"] <= starts.size
    if cfg == "centre_only" and name not in ("path9", "star64"):   # (those two consume a fixed number of words per job)
        assert info["window_misses"] > 0


def test_sequential_offsets_are_plausible():
    """Degree 64: one word per step at the hub, none at a leaf (randint(1)); isolated starts consume nothing."""
    graph, starts, off = sequential("star64")
    per_job = np.diff(off.astype(np.int64))
    assert (per_job == L // 2).all()       # (from the hub or from a leaf: every other step is at the hub)
    graph, starts, off = sequential("isolated")
    per_job = np.diff(off.astype(np.int64))
    assert (per_job[starts >= 12] == 0).all() and (per_job[starts < 12] >= L).all()


def test_default_configuration_commits_many_jobs_per_round():
    graph = sc.karate()
    starts = starts_of(graph, walks=10)
    want, _ = offsets(graph, starts, dict(min_jobs=sc.ONE_LANE))
    got, info = offsets(graph, starts, dict(min_jobs=1))
    assert np.array_equal(got, want)
    assert info["committed_jobs"] == starts.size
    assert info["rounds"] < starts.size / 4


def numpy_words_per_job(graph, starts):
    """FirstOrderUnweighted replayed on NumPy's legacy generator, ``randint(degree)`` per step: the words every job takes,
    read from the generator's own position (a step takes far fewer than a block)."""
    indptr, indices, _ = graph
    rs = np.random.RandomState(SEED)
    per_job = np.zeros(starts.size, dtype=np.int64)
    for i, cur in enumerate(starts):
        for _ in range(L):
            d = int(indptr[cur + 1] - indptr[cur])
            if d == 0:
                break
            before = rs.get_state()[2]
            cur = indices[indptr[cur] + rs.randint(d)]
            per_job[i] += (rs.get_state()[2] - before) % 624
    return per_job


@pytest.mark.parametrize("name", list(sc.GRAPHS))
def test_sequential_words_per_job_are_numpys(name):
    graph, starts, off = sequential(name)
    assert np.array_equal(np.diff(off.astype(np.int64)), numpy_words_per_job(graph, starts))


MODES = {"PreComp": 2, "FirstOrderUnweighted": 3, "PreCompFirstOrder": 4}


def host_walks(mode, graph, tables, starts, cfg):
    """``pw_selftest_seq_walks``: (walk matrix, offsets, [steps, overflow, clamped, dead ends], info)."""
    indptr, indices, data = graph
    aip, aj, aq = tables
    c = PwSeqConfig()
    for k, v in cfg.items():
        setattr(c, k, v)
    out = np.full((starts.size, L + 2), 0xFFFFFFFF, dtype=np.uint32)
    off = np.zeros(starts.size + 1, dtype=np.uint64)
    counts = np.zeros(4, dtype=np.uint64)
    info = PwSeqInfo()
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    _lib.check(_lib.load().pw_selftest_seq_walks(
        MODES[mode], ptr(indptr), ptr(indices), ptr(data), indptr.size - 1, ptr(aip), ptr(aj), ptr(aq), 0 if aj is None else aj.size,
        ptr(starts), starts.size, L, SEED, C.byref(c), ptr(off), ptr(out), ptr(counts), C.byref(info)))
    return out, off, counts, info.as_dict()


def weighted(graph, seed=11):
    indptr, indices, _ = graph
    return indptr, indices, (np.random.default_rng(seed).random(indices.size) + 0.05).astype(np.float32)


def oracle_case(name, mode):
    """(graph, alias tables, starts, the oracle's walk matrix): weighted karate and the undirected edge graphs."""
    graph = weighted(sc.GRAPHS[name]())
    indptr, indices, data = graph
    starts = starts_of(graph)
    if mode == "PreComp":
        tables = orc.precomp_tables(indptr, indices, data, 0.5, 2.0)
        want = orc.walks_precomp(indptr, indices, data, 0.5, 2.0, starts, L, SEED, tables=tables)
    elif mode == "PreCompFirstOrder":
        aj, aq = orc.first_order_tables(indptr, data)
        tables = (indptr.astype(np.uint64), aj, aq)
        want = orc.walks_first_order(indptr, indices, data, starts, L, SEED, precomp=True)
    else:
        tables = (None, None, None)
        want = orc.walks_first_order(indptr, indices, data, starts, L, SEED, precomp=False)
    return graph, tables, starts, want


# (the directed graph with the first-order modes only: second-order tables of a directed graph are outside what the oracle pins)
ORACLE_CASES = [(name, mode) for name in ("karate", "path9", "star65", "isolated", "sink_heavy") for mode in MODES
                if not (name == "sink_heavy" and mode == "PreComp")]


@pytest.mark.parametrize("name,mode", ORACLE_CASES, ids=[f"{n}-{m}" for n, m in ORACLE_CASES])
def test_rows_and_counters_equal_the_oracle_in_every_mode(name, mode):
    graph, tables, starts, want = oracle_case(name, mode)
    lens = want[:, L + 1].astype(np.int64)
    want_counts = [int((lens - 1).sum()), None, None, int(((lens > 1) & (lens < L + 1)).sum())]
    seq_rows, seq_off, seq_counts, _ = host_walks(mode, graph, tables, starts, dict(min_jobs=sc.ONE_LANE))
    assert np.array_equal(seq_rows, want)
    for cfg in (dict(), sc.ADVERSE["round7"], sc.ADVERSE["centre_only"], sc.ADVERSE["smallest_buffer"]):
        rows, off, counts, info = host_walks(mode, graph, tables, starts, dict(cfg, min_jobs=1))
        assert info["path"] == 1 and info["committed_jobs"] == starts.size
        assert np.array_equal(rows, want)
        assert np.array_equal(off, seq_off)
        assert np.array_equal(counts, seq_counts)             # candidates never count
        assert counts[0] == want_counts[0] and counts[3] == want_counts[3]
        assert counts[2] <= counts[1] <= counts[0]
