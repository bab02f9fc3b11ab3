"""Graphs and configurations shared by the tests of the seeded alias / first-order modes' speculation rounds
(test_seq_spec_host.py, test_gpu_seq_spec.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ONE_LANE = 2**64 - 1      # pw_seq_config.min_jobs: always the one-lane kernel / the plain sequential loop

STREAM_SEEDS = (0, 4, 2**32 - 1)
STREAM_OFFSETS = (0, 623, 624, 10**9 + 7)       # the last one needs jump-ahead

# every configuration keeps the result; a negative window_sigmas plans the centre candidate alone (nearly every window misses;
# 0 in a field of pw_seq_config is "the default"),
# force_mean = 1 centres the windows with a mean that is wrong on purpose, word_buffer_blocks = 1 is raised to the smallest
# legal buffer
ADVERSE = {
    "round1": dict(jobs_per_round=1),
    "round7": dict(jobs_per_round=7),
    "round64": dict(jobs_per_round=64),
    "centre_only": dict(window_sigmas=-1.0),
    "wrong_mean": dict(force_mean=1),
    "smallest_buffer": dict(word_buffer_blocks=1),
}


def _csr_from_adj(adj):
    indptr = np.zeros(adj.shape[0] + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(adj.sum(1))
    indices = np.nonzero(adj)[1].astype(np.uint32)
    return indptr, indices, np.ones(indices.size, dtype=np.float32)


def karate():
    z = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    return z["indptr"], z["indices"], z["data"]


def path(n=9):
    adj = np.zeros((n, n), dtype=bool)
    i = np.arange(n - 1)
    adj[i, i + 1] = adj[i + 1, i] = True
    return _csr_from_adj(adj)


def star(leaves):
    """Hub 0 with `leaves` neighbours: randint(64) rejects nothing, randint(65) about half of its words."""
    adj = np.zeros((leaves + 1, leaves + 1), dtype=bool)
    adj[0, 1:] = adj[1:, 0] = True
    return _csr_from_adj(adj)


def isolated():
    """A 12-cycle with chords among vertices 0..11; vertices 12..19 have no edges: their jobs consume nothing."""
    n = 20
    adj = np.zeros((n, n), dtype=bool)
    i = np.arange(12)
    adj[i, (i + 1) % 12] = adj[(i + 1) % 12, i] = True
    adj[0, 5] = adj[5, 0] = adj[2, 9] = adj[9, 2] = adj[0, 7] = adj[7, 0] = True
    return _csr_from_adj(adj)


def sink_heavy():
    """400 vertices, directed, 40 % sinks (the graph of test_sink_heavy_directed_graph_is_exact_by_default)."""
    rng = np.random.default_rng(5)
    n = 400
    adj = rng.random((n, n)) < 0.02
    np.fill_diagonal(adj, False)
    adj[rng.choice(n, 160, replace=False), :] = False
    return _csr_from_adj(adj)


GRAPHS = {
    "karate": karate,
    "path9": path,
    "star64": lambda: star(64),
    "star65": lambda: star(65),
    "isolated": isolated,
    "sink_heavy": sink_heavy,
}
