"""Call scripts for the tables a graph handle keeps between calls, with what the CPU oracle gives for every step.

A handle caches five families of device tables (per-edge normalisers, the weighted lane form, unit row totals, alias tables,
thresholds), each under its own keys.  A wrong key does not crash: it returns walks sampled from another call's distribution.
A script is a list of steps on ONE handle; consecutive steps change one key at a time and some return to an earlier state, so
that a table reused under the wrong key, or not rebuilt, shows as walks (or alias words) that are not the oracle's.

No GPU and no marker here: ``test_table_history_host.py`` checks on the CPU that the steps that are meant to differ do so in
the oracle (or the GPU test could not tell a stale table from a fresh one), ``test_gpu_table_history.py`` runs the scripts.

Graphs: the undirected R-MAT of scale 8, seed 3 (256 vertices), weighted and unit.  512 walks of 20 steps, seed 4.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import pyoracle as orc
from pecanpy_amd.synth import csr_from_edges, hash_edge_weights, rmat_csr

L = 20
SEED = 4
SMALL = 100           # starts of a call that samples fewer steps than the graphs have entries (asserted by the host test)

# One call on the handle.  thr: "T0" / "T1" = the thresholds uploaded at this step or before it (gamma 0 / 1), None = none yet.
#   differs: the oracle's walks must differ from the previous step's in at least half of the rows
#   same_as: index of an earlier step whose oracle walks (and alias tables) this step returns to
#   fresh:   the GPU test also makes this call on a fresh handle (same walks, same integer statistics)
#   built:   this call builds per-(p, q) tables (param_index_ms > 0); False: it must find or need none (== 0); None: not checked
#   lane:    lane_kernel of the call (None: not checked); not_lane: a value lane_kernel must NOT have
#   n:       number of starts (the first n of the 512)
Step = namedtuple("Step", "mode p q extend thr env differs same_as fresh built lane not_lane n")


def step(mode, p, q, extend, thr, env=(), differs=True, same_as=None, fresh=False, built=None, lane=None, not_lane=None, n=None):
    return Step(mode, float(p), float(q), bool(extend), thr, tuple(env), differs, same_as, fresh, built, lane, not_lane, n)


# ---- alias tables: thresholds, extend, (p, q), the kind (sum(deg^2) against sum(deg) entries) and back --------------------
ALIAS = [
    step("PreComp", 0.5, 2, True, "T0", differs=False),
    step("PreComp", 0.5, 2, True, "T1"),                       # only the thresholds changed
    step("PreComp", 0.5, 2, False, "T1"),
    step("PreComp", 1.3, 0.7, False, "T1"),
    step("PreCompFirstOrder", 1, 1, False, "T1"),
    step("PreComp", 0.5, 2, True, "T1", same_as=1),
    step("PreComp", 0.5, 2, True, "T0", same_as=0),
]

# the same through the mode class: (p, q, gamma) of a PreComp(extend=True) object, preprocess + walk at every step
PY_ALIAS = [
    step("PreComp", 0.5, 2, True, "T0", differs=False),
    step("PreComp", 0.5, 2, True, "T1"),
    step("PreComp", 1.3, 0.7, True, "T1"),
    step("PreComp", 1.3, 0.7, True, "T0"),
]

# ---- per-edge normaliser table (the weighted lane form off) --------------------------------------------------------------------
TOT_ENV = (("PECANPY_AMD_FORCE_TOT", "1"), ("PECANPY_AMD_NO_WLANES", "1"))
NORMALISER = [
    step("SparseOTF", 0.5, 2, True, "T0", TOT_ENV, differs=False, built=True),
    step("SparseOTF", 0.5, 2, True, "T1", TOT_ENV, built=True),
    step("SparseOTF", 0.5, 2, False, "T1", TOT_ENV, built=True),
    step("SparseOTF", 0.5, 2, True, "T1", TOT_ENV, built=True, same_as=1),
    step("SparseOTF", 0.3, 1.7, True, "T1", TOT_ENV, built=True),
    step("SparseOTF", 0.5, 2, True, "T1", TOT_ENV, built=True, same_as=1),
    step("SparseOTF", 0.5, 2, True, "T0", TOT_ENV, built=True, same_as=0),
    # no FORCE_TOT, fewer sampled steps than entries, a (p, q) no table was built for: the two-pass step, no table read or built
    step("SparseOTF", 1.3, 0.7, True, "T0", (("PECANPY_AMD_NO_WLANES", "1"),), built=False, n=SMALL, differs=False),
]

# ---- weighted lane form: the same keys, and a p outside the form's [1/1024, 1024] -----------------------------------------------
WL_ENV = (("PECANPY_AMD_FORCE_TOT", "1"), ("PECANPY_AMD_CHAIN_TAIL", "0"))
WLANE = [
    step("SparseOTF", 0.5, 2, True, "T0", WL_ENV, differs=False, built=True, lane=3),
    step("SparseOTF", 0.5, 2, True, "T1", WL_ENV, built=True, lane=3),
    step("SparseOTF", 0.5, 2, False, "T1", WL_ENV, built=True, lane=3),
    step("SparseOTF", 0.5, 2, True, "T1", WL_ENV, built=True, lane=3, same_as=1),
    step("SparseOTF", 0.3, 1.7, True, "T1", WL_ENV, built=True, lane=3),
    step("SparseOTF", 2048, 1.7, True, "T1", WL_ENV, built=True, not_lane=3),    # normalisers only: the lane tables stay
    step("SparseOTF", 0.3, 1.7, True, "T1", WL_ENV, built=True, lane=3, same_as=4),   # ... and serve this call (built two steps ago)
    step("SparseOTF", 0.5, 2, True, "T1", WL_ENV, built=True, lane=3, same_as=1),
    step("SparseOTF", 0.5, 2, True, "T0", WL_ENV, built=True, lane=3, same_as=0),
]

# ---- unit row totals: keyed by float32 1/q and 1/p -------------------------------------------------------------------------------
UNIT_ENV = (("PECANPY_AMD_FORCE_TOT", "1"),)
UNIT = [
    step("SparseOTF", 0.3, 1.7, False, None, UNIT_ENV, differs=False, fresh=True, built=True, lane=2),
    step("SparseOTF", 0.3, 1.3, False, None, UNIT_ENV, fresh=True, built=True, lane=2),      # same 1/p, other 1/q
    step("SparseOTF", 0.7, 1.7, False, None, UNIT_ENV, fresh=True, built=True, lane=2),      # other 1/p, a 1/q seen before
    step("SparseOTF", 0.5, 2, False, None, UNIT_ENV, fresh=True, built=False, lane=1),       # dyadic: the exact form, no table
    step("SparseOTF", 0.3, 1.7, False, None, UNIT_ENV, fresh=True, built=True, lane=2, same_as=0),
    step("SparseOTF", 0.9, 1.1, False, None, (), fresh=True, built=False, lane=2, n=SMALL, differs=False),
]

# ---- the modes of one weighted handle, one after the other -------------------------------------------------------------------------
INTERLEAVED = [
    step("SparseOTF", 0.5, 2, True, "T0", differs=False),
    step("PreComp", 0.5, 2, True, "T0"),
    step("SparseOTF", 0.5, 2, True, "T1"),
    step("PreComp", 0.5, 2, True, "T1"),
    step("FirstOrderUnweighted", 1, 1, False, "T1"),
    step("SparseOTF", 0.5, 2, False, "T1"),
]

SCRIPTS = {"alias": ("weighted", ALIAS), "py_alias": ("weighted", PY_ALIAS), "normaliser": ("weighted", NORMALISER),
           "wlane": ("weighted", WLANE), "unit": ("unit", UNIT), "interleaved": ("weighted", INTERLEAVED)}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def graph(kind):
    """``(indptr, indices, data)`` of the "weighted" or the "unit" graph (shared, read-only)."""
    return _frozen(*rmat_csr(8, seed=3, weighted=(kind == "weighted")))


@functools.lru_cache(maxsize=None)
def thresholds(name):
    """T0 / T1: the reference expression (sparse_rw.py:22-35) at gamma 0 / 1 for the weighted graph, through the host
    mirror; NaN (the mean of an empty row, never read) -> 0."""
    from pecanpy_amd import pecanpy as node2vec

    indptr, _, data = graph("weighted")
    g = node2vec.SparseOTF(gamma={"T0": 0, "T1": 1}[name], extend=True)
    g.indptr, g.data = indptr, data
    g.set_node_ids(None, implicit_ids=True, num_nodes=indptr.size - 1)
    with np.errstate(all="ignore"):
        return _frozen(np.nan_to_num(g.get_noise_thresholds(), nan=0.0))


@functools.lru_cache(maxsize=None)
def starts():
    return _frozen(orc.shuffled_starts(graph("weighted")[0].size - 1, 2, 4))


def step_starts(s):
    return starts() if s.n is None else starts()[: s.n]


def _thr_of(s):
    return thresholds(s.thr) if s.extend else None


@functools.lru_cache(maxsize=None)
def _oracle_walks(kind, mode, p, q, extend, thr, n):
    indptr, indices, data = graph(kind)
    st = starts() if n is None else starts()[:n]
    t = thresholds(thr) if extend else None
    if mode == "SparseOTF":
        return _frozen(orc.walks_sparse_otf(indptr, indices, data, p, q, st, L, SEED, thr=t))
    if mode == "PreComp":
        return _frozen(orc.walks_precomp(indptr, indices, data, p, q, st, L, SEED, thr=t))
    return _frozen(orc.walks_first_order(indptr, indices, data, st, L, SEED, precomp=(mode == "PreCompFirstOrder")))


def oracle_walks(kind, s):
    """The oracle's walk matrix of step ``s`` (computed once per distinct call, read-only).  Thresholds a call does not read
    (extend off) are no part of the key."""
    return _oracle_walks(kind, s.mode, s.p, s.q, s.extend, s.thr if s.extend else None, s.n)


@functools.lru_cache(maxsize=None)
def _oracle_tables(kind, mode, p, q, extend, thr):
    indptr, indices, data = graph(kind)
    if mode == "PreCompFirstOrder":
        aj, aq = orc.first_order_tables(indptr, data)
        return _frozen(indptr.astype(np.uint64), aj, aq)
    return _frozen(*orc.precomp_tables(indptr, indices, data, p, q, thr=thresholds(thr) if extend else None))


def oracle_tables(kind, s):
    """``(alias_indptr, alias_j, alias_q)`` of an alias step: sum(deg^2) entries for PreComp, sum(deg) for PreCompFirstOrder
    (whose alias_indptr is the CSR's)."""
    assert s.mode in ("PreComp", "PreCompFirstOrder")
    return _oracle_tables(kind, s.mode, s.p, s.q, s.extend, s.thr if s.extend else None)


def rows_differing(a, b):
    """Share of the rows of two walk matrices that differ."""
    assert a.shape == b.shape
    return float((a != b).any(axis=1).mean())


def words_differing(a, b):
    """Share of the float32 words of two alias_q arrays of one size that differ."""
    assert a.shape == b.shape
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


# ---- twin halves that disagree about the normaliser table ------------------------------------------------------------------------------
TWIN_N = 1 << 16
TWIN_EDGES = 524289                  # undirected: nnz = 1 048 578
TWIN_JOBS = (1 << 20) + 1            # halves of 2^19 and 2^19 + 1 walks
TWIN_L = 2                           # ... sample 1 048 576 < nnz and 1 048 578 >= nnz steps
TWIN_SEED = 9
TWIN_P, TWIN_Q = 0.5, 2.0


@functools.lru_cache(maxsize=None)
def twin_graph():
    """Weighted, undirected, 2^16 vertices, exactly TWIN_EDGES simple edges drawn from a seeded generator."""
    rng = np.random.default_rng(12)
    s, d = rng.integers(0, TWIN_N, 600000), rng.integers(0, TWIN_N, 600000)
    lo, hi = np.minimum(s, d), np.maximum(s, d)
    key = np.unique((lo * TWIN_N + hi)[lo != hi])
    key = rng.permutation(key)[:TWIN_EDGES]
    assert key.size == TWIN_EDGES
    lo, hi = key // TWIN_N, key % TWIN_N
    indptr, indices, _ = csr_from_edges(np.concatenate([lo, hi]), np.concatenate([hi, lo]), TWIN_N)
    return _frozen(indptr, indices, hash_edge_weights(indptr, indices, 5))


@functools.lru_cache(maxsize=None)
def twin_starts():
    st = np.concatenate([np.arange(TWIN_N, dtype=np.uint32)] * (TWIN_JOBS // TWIN_N) + [np.zeros(TWIN_JOBS % TWIN_N, dtype=np.uint32)])
    np.random.RandomState(3).shuffle(st)
    return _frozen(st)
