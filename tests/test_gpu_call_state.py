"""What one walk call leaves in its handle for the next: the per-call state of the driver (lane statistics, verification
counts, the weighted lane form's flags, the (p, q) index time) and the random stream's hold.

Calls with different switches follow each other on ONE handle; every call's walk matrix and statistics must be those of the
same call on a fresh handle, or of the same call made earlier.  All comparisons are exact but one: that a hold served its calls shows only in their stream time.  One small graph: an undirected
unit R-MAT of scale 10 (and a weighted copy), 512 walks of length 8, seeded."""
import numpy as np
import pytest

from pecanpy_amd.engine import WalkEngine
from pecanpy_amd.synth import hash_edge_weights, rmat_csr

pytestmark = pytest.mark.gpu

L = 8
SEED = 11
P, Q = 0.5, 2.0      # dyadic: the unit graph's calls take the exact lane form
VERIFY = ("verify_checked", "verify_mismatch", "verify_dropped", "verify_ties")


@pytest.fixture(scope="module")
def graph():
    indptr, indices, _ = rmat_csr(10, seed=4)
    starts = np.random.default_rng(4).integers(0, indptr.size - 1, 512).astype(np.uint32)
    return indptr, indices, starts


def _call(eng, starts, **kw):
    walks = eng.simulate("SparseOTF", P, Q, False, starts, L, seed=SEED, **kw)
    return walks, dict(eng.last_stats)


def _integers(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms")}


def test_a_call_without_lanes_between_two_verified_lane_calls(graph, monkeypatch):
    indptr, indices, starts = graph
    eng, fresh = WalkEngine.from_csr(indptr, indices), WalkEngine.from_csr(indptr, indices)
    # A: the lane kernel, every settled step verified
    monkeypatch.setenv("PECANPY_AMD_VERIFY_TIGHT", "1")
    walks_a, st_a = _call(eng, starts)
    assert st_a["lane_kernel"] == 1 and st_a["lane_rounds"] > 0 and st_a["verify_checked"] > 0, st_a
    # B: straight afterwards, no lanes and no verification -- the statistics of a fresh handle that makes only this call
    monkeypatch.delenv("PECANPY_AMD_VERIFY_TIGHT")
    monkeypatch.setenv("PECANPY_AMD_NO_LANES", "1")
    walks_b, st_b = _call(eng, starts)
    want_b, st_fresh = _call(fresh, starts)
    monkeypatch.delenv("PECANPY_AMD_NO_LANES")
    for k in ("lane_kernel", "lane_rounds", "lane_kernel_ms") + VERIFY:
        assert st_b[k] == 0 and st_fresh[k] == 0, (k, st_b, st_fresh)
    assert st_b["total_steps"] == st_fresh["total_steps"]
    assert np.array_equal(walks_b, want_b)
    assert _integers(st_b) == _integers(st_fresh)
    # C: A again
    monkeypatch.setenv("PECANPY_AMD_VERIFY_TIGHT", "1")
    walks_c, st_c = _call(eng, starts)
    assert np.array_equal(walks_c, walks_a) and np.array_equal(walks_a, walks_b)
    assert _integers(st_c) == _integers(st_a)
    eng.close()
    fresh.close()


def test_weighted_lane_form_between_and_after_other_calls(graph, monkeypatch):
    indptr, indices, starts = graph
    data = hash_edge_weights(indptr, indices, seed=4)
    eng, fresh = WalkEngine.from_csr(indptr, indices, data), WalkEngine.from_csr(indptr, indices, data)
    # 512 walks of 8 steps sample fewer steps than the graph has entries: the per-(p, q) tables the weighted lane form needs
    # are built for such a call only when asked for (PECANPY_AMD_FORCE_TOT), and its rounds queue only with CHAIN_TAIL=0
    assert starts.size * L < indices.size
    monkeypatch.setenv("PECANPY_AMD_FORCE_TOT", "1")
    monkeypatch.setenv("PECANPY_AMD_CHAIN_TAIL", "0")
    walks_a, st_a = _call(eng, starts)
    assert st_a["lane_kernel"] == 3 and st_a["lane_rounds"] > 0, st_a
    assert st_a["param_index_ms"] > 0, st_a          # (this call built the tables)
    # B: the weighted lane form switched off -- as on a fresh handle
    monkeypatch.setenv("PECANPY_AMD_NO_WLANES", "1")
    walks_b, st_b = _call(eng, starts)
    want_b, st_fresh = _call(fresh, starts)
    monkeypatch.delenv("PECANPY_AMD_NO_WLANES")
    assert st_b["lane_kernel"] != 3 and st_b["lane_rounds"] == 0 and st_b["lane_kernel_ms"] == 0, st_b
    assert np.array_equal(walks_b, want_b) and np.array_equal(walks_b, walks_a)
    assert _integers(st_b) == _integers(st_fresh)
    # C: A again; the tables are in place, so no (p, q) index time is reported
    walks_c, st_c = _call(eng, starts)
    assert np.array_equal(walks_c, walks_a)
    assert _integers(st_c) == _integers(st_a)
    assert st_b["param_index_ms"] == 0 and st_c["param_index_ms"] == 0, (st_b, st_c)
    eng.close()
    fresh.close()


def test_chunked_calls_inside_a_stream_hold_and_a_call_behind_it(graph):
    indptr, indices, starts = graph
    eng, plain = WalkEngine.from_csr(indptr, indices), WalkEngine.from_csr(indptr, indices)
    skip = 1000                                      # (not a multiple of the stream's 312-draw blocks)
    half = starts.size // 2
    draws_all, draws_a = plain.count_stream_draws(starts, L), plain.count_stream_draws(starts[:half], L)

    def calls(e):
        first, st1 = _call(e, starts[:half], stream_skip=skip)
        second, st2 = _call(e, starts[half:], stream_skip=skip + draws_a)
        return first, second, (st1["rng_kernel_ms"], st2["rng_kernel_ms"])

    eng.stream_hold(SEED, skip, draws_all)
    held = calls(eng)
    eng.stream_release()
    behind = _call(eng, starts, stream_skip=5)[0]     # (outside the range that was held: its own expansion)
    want = calls(plain)
    assert np.array_equal(held[0], want[0]) and np.array_equal(held[1], want[1])
    assert np.array_equal(behind, _call(plain, starts, stream_skip=5)[0])
    whole = _call(plain, starts, stream_skip=skip)[0]   # (an undirected graph: the chunks are the rows of one call)
    assert np.array_equal(np.concatenate(held[:2]), whole)
    # The hold SERVED both chunks.  A hold that kept too few blocks would be dropped and the chunk's range expanded again --
    # the same draws, so the walks above cannot tell.  The stream time can: a served call records its two events back to back,
    # an expansion puts its jump-ahead launches (here about ten, one behind the other) and the generator kernel between them, as
    # `plain` does for the same chunks, which it expands for the first time.  Not an exact comparison, so with a margin:
    # no launch against some ten dependent ones must come out under a quarter.
    print("rng_kernel_ms held", held[2], "expanded", want[2])
    for h_ms, e_ms in zip(held[2], want[2]):
        assert h_ms < e_ms / 4, (held[2], want[2])
    eng.close()
    plain.close()
