"""Host oracle of ``from_edge_index`` and the graphs its tests use (shared by test_edge_index_host.py and
test_gpu_edge_index.py).

The oracle is the package's own ``AdjlstGraph`` -- pinned to the reference by tests/test_edgelist.py and
tests/test_host_logic.py -- driven so that its first-appearance numbering equals the integer ids: every vertex is
registered first (``add_node(str(i))``), then the edges are added in edge order (``add_edge``: non-positive weights
dropped, reverse edge unless directed, last insertion wins), then ``to_csr()``."""
import warnings

import numpy as np

from pecanpy_amd.graph import AdjlstGraph


def oracle_csr(edge_index, edge_weight, num_nodes, directed):
    """``(indptr, indices, data, insertions, dropped)`` of the reference's edge-by-edge construction."""
    edge_index = np.asarray(edge_index)
    n = int(num_nodes) if num_nodes is not None else (int(edge_index.max()) + 1 if edge_index.size else 0)
    g = AdjlstGraph()
    for i in range(n):
        g.add_node(str(i))
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    w = [1.0] * len(src) if edge_weight is None else [float(x) for x in np.asarray(edge_weight, dtype=np.float32)]
    dropped = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (overwritten duplicates and dropped edges warn one by one)
        for s, d, x in zip(src, dst, w):
            dropped += x <= 0
            g.add_edge(str(s), str(d), x, directed)
    assert g.num_nodes == n
    indptr, indices, data = g.to_csr()
    return indptr, indices, data, g.num_edges, dropped


# ---- the graphs of the cases (deterministic: fixed seeds) ---------------------------------------------------------------
def small_unweighted():
    """34 vertices, 160 listed edges: repeats, both orientations of a pair, self loops."""
    rng = np.random.RandomState(34)
    e = rng.randint(0, 34, size=(2, 120))
    e = np.concatenate([e, e[::-1, :20], e[:, 5:15], np.array([[3, 7, 7, 33], [3, 7, 7, 33]])], axis=1)
    return e.astype(np.int64), None, 34


def weighted_conflicts(n=40, m=300, seed=5):
    """Weighted, conflicting duplicates: (a, b, w1) ... (b, a, w2) and repeats of the same orientation; self loops listed
    twice with different weights.  Every weight a distinct float32."""
    rng = np.random.RandomState(seed)
    e = rng.randint(0, n, size=(2, m))
    k = m // 6
    e = np.concatenate([e, e[::-1, :k], e[:, k:2 * k], np.array([[2, 9, 2, 9], [2, 9, 2, 9]])], axis=1)
    w = (0.25 + rng.permutation(e.shape[1]) / 16.0).astype(np.float32)
    return e.astype(np.int64), w, n


def dropped_rows():
    """Non-positive weights; vertex 6 has dropped edges only; num_nodes (12) beyond the largest id (8)."""
    e = np.array([[0, 1, 2, 6, 6, 3, 4, 0, 5, 8], [1, 2, 0, 1, 6, 4, 3, 1, 5, 2]], dtype=np.int64)
    w = np.array([1.5, 2.0, 0.0, -1.0, 0.0, 3.0, 0.5, -2.5, 1.0, 4.0], dtype=np.float32)
    return e, w, 12


def hub(n=80_000, hub_degree=70_000, background=50_007, seed=11):
    """Vertex 17 adjacent to 70 000 others (a row longer than any LDS tile), a random background over 80 000 vertices,
    and duplicates of hub edges at the two ends of the list with different weights: the winner (the last listed) lies
    far from the loser, in another wavefront's and another workgroup's part of the sort.  m = 120 019 (odd)."""
    rng = np.random.RandomState(seed)
    others = rng.permutation(np.setdiff1d(np.arange(n), [17]))[:hub_degree]
    hub_e = np.stack([np.full(hub_degree, 17), others])
    flip = rng.rand(hub_degree) < 0.5
    hub_e[:, flip] = hub_e[::-1, flip]
    bg = rng.randint(0, n, size=(2, background))
    mid = np.concatenate([hub_e, bg], axis=1)[:, rng.permutation(hub_degree + background)]
    first = np.stack([np.full(6, 17), others[:6]])           # losers: listed first ...
    last = np.stack([others[:6], np.full(6, 17)])            # ... winners: listed last, the other orientation
    e = np.concatenate([first, mid, last], axis=1).astype(np.int64)
    w = (1.0 + rng.randint(0, 1 << 20, size=e.shape[1]) / 1024.0).astype(np.float32)
    w[:6] = 0.5
    w[-6:] = 7.75
    return e, w, n


def directed_sinks():
    """Directed: vertices 5 and 9 are sinks, 11..13 isolated (14 vertices)."""
    e = np.array([[0, 0, 1, 2, 3, 3, 4, 6, 7, 8, 10, 0, 3], [1, 5, 2, 5, 9, 4, 0, 9, 6, 7, 8, 1, 3]], dtype=np.int64)
    return e, None, 14
