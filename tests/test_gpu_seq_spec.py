"""The raw MT19937 stream words on the device (jump-ahead tree + ``mt_words_kernel`` through ``pw_stream_words_device``)
against the host service ``pw_mt_words``, itself pinned to NumPy in test_seq_spec_host.py: the words the seeded alias /
first-order modes consume, at block boundaries and at an offset that needs jump-ahead.  And the host form of the
speculation rounds against the one-lane kernel that serves seeded calls on the device: rows and counters."""
import ctypes as C

import numpy as np
import pytest

import seq_spec_cases as sc
from oracle import pyoracle as orc
from pecanpy_amd import _lib
from pecanpy_amd._lib import MODE_IDS, PwSeqConfig, PwSeqInfo
from pecanpy_amd.engine import WalkEngine
from pecanpy_amd.synth import rmat_csr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", sc.STREAM_SEEDS)
def test_device_words_match_host_words(seed):
    eng = WalkEngine.from_csr(*sc.path())
    lib = _lib.load()
    for off in sc.STREAM_OFFSETS:
        n = 1300            # (more than two blocks)
        want = np.zeros(n, dtype=np.uint32)
        _lib.check(lib.pw_mt_words(seed, off, n, C.c_void_p(want.ctypes.data)))
        assert np.array_equal(eng.stream_words(seed, off, n), want), off


def test_device_words_many_blocks_per_generator():
    """More than 512 blocks: every generator expands several blocks and the last one fewer (the shape of a real word
    buffer), from an offset inside a block, with an odd tail."""
    eng = WalkEngine.from_csr(*sc.path())
    seed, off, n = 4, 1000, 1027 * 624 + 77
    want = np.zeros(n, dtype=np.uint32)
    _lib.check(_lib.load().pw_mt_words(seed, off, n, C.c_void_p(want.ctypes.data)))
    assert np.array_equal(eng.stream_words(seed, off, n), want)


L, SEED = 30, 4
MODES = [("PreComp", 0.5, 2.0), ("FirstOrderUnweighted", 1, 1), ("PreCompFirstOrder", 1, 1)]


@pytest.mark.parametrize("mode,p,q", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("name", ["karate", "rmat8", "star65"])
def test_host_rounds_equal_the_one_lane_kernel(name, mode, p, q):
    """The host form of the rounds (``pw_selftest_seq_walks`` on the tables the device built) against ``walk_seq_kernel``:
    the walk matrix and the four counters of ``pw_stats``; and both against the oracle."""
    graph = rmat_csr(8, seed=3, weighted=True) if name == "rmat8" else sc.GRAPHS[name]()
    indptr, indices, data = (np.ascontiguousarray(a) for a in graph)
    starts = orc.shuffled_starts(indptr.size - 1, 3, SEED)
    eng = WalkEngine.from_csr(indptr, indices, data)
    lane = eng.simulate(mode, p, q, False, starts, L, seed=SEED)
    st = eng.last_stats
    if mode == "PreComp":
        want = orc.walks_precomp(indptr, indices, data, p, q, starts, L, SEED)
    else:
        want = orc.walks_first_order(indptr, indices, data, starts, L, SEED, precomp=mode == "PreCompFirstOrder")
    assert np.array_equal(lane, want)
    tables = (None, None, None) if mode == "FirstOrderUnweighted" else eng.precomp_export(mode == "PreCompFirstOrder")
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    for min_jobs in (sc.ONE_LANE, 1):
        cfg, info = PwSeqConfig(), PwSeqInfo()
        cfg.min_jobs = min_jobs
        rows = np.full_like(lane, 0xFFFFFFFF)
        off = np.zeros(starts.size + 1, dtype=np.uint64)
        counts = np.zeros(4, dtype=np.uint64)
        _lib.check(_lib.load().pw_selftest_seq_walks(
            MODE_IDS[mode], ptr(indptr), ptr(indices), ptr(data), indptr.size - 1, *(ptr(t) for t in tables),
            0 if tables[1] is None else tables[1].size, ptr(starts), starts.size, L, SEED, C.byref(cfg), ptr(off), ptr(rows),
            ptr(counts), C.byref(info)))
        assert info.path == (1 if min_jobs == 1 else 0)
        assert np.array_equal(rows, lane)
        assert [int(c) for c in counts] == [st["total_steps"], st["overflow_reads"], st["clamped_reads"], st["dead_end_walks"]]
