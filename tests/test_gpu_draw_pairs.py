"""The lane kernel fetches a walk's draws as aligned 16-byte pairs and keeps the second double for the next step
(walk_lanes.hip.h: next_draw).  What can go wrong is the parity of a walk's place in the stream, a held draw that outlives the
walk's stay in its lane (deferral to the pool, parking in the queue, end of walk, refill), and a pair at the very end of the
expanded stream.  Every case compares the lane kernel's walk matrix bit for bit with the CPU oracle and with the wave-per-walk
kernel on the same jobs, and checks that the lane kernel ran."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from pecanpy_amd.engine import WalkEngine
from pecanpy_amd.synth import csr_from_edges, rmat_csr

pytestmark = pytest.mark.gpu


def _engines(indptr, indices, data):
    """(lane engine, wave-per-walk engine) of one graph."""
    lane = WalkEngine.from_csr(indptr, indices, data)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PECANPY_AMD_NO_LANES", "1")
        wave = WalkEngine.from_csr(indptr, indices, data)
    return lane, wave


def _check(lane, wave, csr, p, q, starts, L, seed, form=1, skip=0):
    indptr, indices, data = csr
    want = orc.walks_sparse_otf(indptr, indices, data, p, q, starts, L, seed, stream_skip=skip)
    got = lane.simulate("SparseOTF", p, q, False, starts, L, seed=seed, stream_skip=skip)
    st = dict(lane.last_stats)
    assert st["lane_kernel"] == form
    assert np.array_equal(got, want)
    got_w = wave.simulate("SparseOTF", p, q, False, starts, L, seed=seed, stream_skip=skip)
    assert wave.last_stats["lane_kernel"] == 0
    assert np.array_equal(got_w, want)
    return st


@pytest.fixture(scope="module")
def rmat12():
    csr = rmat_csr(12, seed=32)
    lane, wave = _engines(*csr)
    return csr, lane, wave


@pytest.mark.parametrize("L", [1, 2, 3, 5, 80])
def test_walk_lengths_of_both_parities(rmat12, L):
    """Odd lengths: consecutive walks start on alternating parities of the stream.  Length 1 never uses a held draw."""
    csr, lane, wave = rmat12
    starts = orc.shuffled_starts(csr[0].size - 1, 3, 5)
    _check(lane, wave, csr, 0.5, 2, starts, L, 5)


@pytest.mark.parametrize("skip", [157, 1000])
def test_stream_skip_odd_and_even_up_to_the_last_draw_of_the_last_block(rmat12, skip):
    """A job slice addressed into the stream at an odd and at an even offset, neither a multiple of the block of 312 draws;
    the slice's last walk takes the last draw of the last expanded block (undirected graph: every start with neighbours
    draws L times), so the last pair ends where the buffer ends."""
    csr, lane, wave = rmat12
    L = 5
    has = csr[0][1:] != csr[0][:-1]
    starts = orc.shuffled_starts(csr[0].size - 1, 3, 6)
    starts = starts[has[starts]]
    m = 2000
    while (skip + m * L) % 312:
        m += 1
    assert skip % 312 and m <= starts.size
    st = _check(lane, wave, csr, 0.5, 2, starts[:m], L, 6, skip=skip)
    assert st["total_steps"] == m * L


def test_dead_ends_end_walks_in_the_middle_of_a_pair():
    rng = np.random.default_rng(8)
    n = 3000
    src = rng.integers(0, n, 24000)
    dst = rng.integers(0, n, 24000)
    keep = (src != dst) & (src % 50 != 0)            # 2 % of the vertices have no out-edges
    csr = csr_from_edges(src[keep], dst[keep], n)
    lane, wave = _engines(*csr)
    st = _check(lane, wave, csr, 0.25, 4, orc.shuffled_starts(n, 2, 3), 12, 3)
    assert st["dead_end_walks"] > 0


def _hub_graph(rng, n=60000, hub_deg=40000):
    hub = np.arange(1, hub_deg + 1)
    src = [np.zeros(hub.size, dtype=np.int64), rng.integers(1, n, 300000), np.full(3000, 7, dtype=np.int64)]
    dst = [hub, rng.integers(1, n, 300000), rng.integers(1, n, 3000)]
    s, d = np.concatenate(src), np.concatenate(dst)
    keep = s != d
    s, d = s[keep], d[keep]
    return csr_from_edges(np.concatenate([s, d]), np.concatenate([d, s]), n)


def test_walks_leave_and_re_enter_lanes_on_both_parities(monkeypatch):
    """The hub graph: most steps are deferred to the pool, many are parked in the queue and resumed by the next round
    (PECANPY_AMD_CHAIN_TAIL=0: every open step), or wait in the pool for a chain pass (PECANPY_AMD_LANE_CHAINS=1) -- at
    any step of the walk, so on either parity.  The held draw must not follow the lane to its next walk."""
    rng = np.random.default_rng(13)
    csr = _hub_graph(rng)
    n = csr[0].size - 1
    starts = np.concatenate([np.zeros(200, dtype=np.uint32), rng.integers(0, n, 6000).astype(np.uint32)])
    L, seed = 25, 4
    want = orc.walks_sparse_otf(*csr, 0.5, 2, starts, L, seed)
    lane, wave = _engines(*csr)
    assert np.array_equal(wave.simulate("SparseOTF", 0.5, 2, False, starts, L, seed=seed), want)
    assert wave.last_stats["lane_kernel"] == 0
    for name, env in (("queue", {"PECANPY_AMD_CHAIN_TAIL": "0"}), ("chains", {"PECANPY_AMD_LANE_CHAINS": "1"}), ("default", {})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = lane.simulate("SparseOTF", 0.5, 2, False, starts, L, seed=seed)
        for k in env:
            monkeypatch.delenv(k)
        st = dict(lane.last_stats)
        assert st["lane_kernel"] == 1, name
        assert st["ambiguous_steps"] > 0 and st["wave_chain_steps"] > 0, name
        assert np.array_equal(got, want), name
        if name == "queue":
            assert st["lane_rounds"] > 1
        if name == "chains":
            assert st["lane_rounds"] == 1


def test_floats_form_non_dyadic(rmat12):
    csr, lane, wave = rmat12
    starts = orc.shuffled_starts(csr[0].size - 1, 3, 7)
    _check(lane, wave, csr, 0.3, 1.7, starts, 31, 7, form=2)
