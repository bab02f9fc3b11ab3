"""Experimental walk modes: the reference's ``pecanpy.experimental`` (src/pecanpy/experimental.py) on the MI355X walk engine.

``Node2vecPlusPlus`` is node2vec++, the reference authors' continuous form of node2vec+ for weighted dense graphs.  Its walks
run in ``walk_dense_weighted_kernel`` (csrc/walk_dense_w.hip.h) as a third bias form beside node2vec and node2vec+; seeded
runs reproduce the reference's single-thread walks bit for bit.

``SparseNode2vecPlusPlus`` is the same walk on a CSR graph, for graphs whose dense form would not fit (the reference has
no sparse form).  Its walks equal the reference's ``Node2vecPlusPlus`` on ``A.toarray().astype(np.float64)``; they run in
``walk_sparse_pp_kernel`` (csrc/walk_sparse_pp.hip.h).
"""
import numpy as np

from .pecanpy import _DenseBase, _SparseBase

__all__ = ["Node2vecPlusPlus", "SparseNode2vecPlusPlus"]


class Node2vecPlusPlus(_DenseBase):
    """Continuous extension of node2vec+ with the DenseOTF framework (reference experimental.py:8-102).

    For a neighbour ``x`` of ``cur`` with ``w(prev, x) < thr(x)`` (``thr``: the noise thresholds, ``gamma``), the weight
    ``w(cur, x)`` is multiplied by ``t * b / (1 + (b - 1)) * |1 - 1/q| + min(1, 1/q)``, where ``t = w(prev, x) / thr(x)``
    (``1 - t`` when ``q < 1``) and ``b = w(cur, x) / thr(x)``; the return edge is divided by ``p``.  The thresholds are
    always used: ``extend`` changes nothing.  Needs finite, positive edge weights.
    """

    _mode = "Node2vecPlusPlus"
    _always_thresholds = True

    def setup_get_normalized_probs(self):
        """``(get_normalized_probs, noise_thresholds)``: the node2vec++ probabilities and the thresholds they use."""
        return self.get_normalized_probs, self.get_noise_thresholds()

    def get_normalized_probs(self, data, nonzero, p, q, cur_idx, prev_idx=None, noise_threshold_ary=None):
        """node2vec++ transition probabilities over ``cur_idx``'s neighbours (float64), with the reference's signature
        (experimental.py:62-102).  Computed on the GPU from the graph this object holds (``pw_probs``): the probabilities
        the walk kernel samples from, bit for bit; ``data``, ``nonzero`` and ``noise_threshold_ary`` are not read."""
        eng = self._get_engine()
        return eng.probs(self._mode, p, q, False, cur_idx, prev_idx)


class SparseNode2vecPlusPlus(_SparseBase):
    """node2vec++ on a CSR graph (``from_mat``, ``from_csr``, ``read_edg``, ``read_npz`` as for ``SparseOTF``).

    Walks, probabilities and steps are those of the reference's ``Node2vecPlusPlus`` run on the dense float64 form of the
    graph, bit for bit, including its noise thresholds (the dense formula: float64 mean and std of a row's non-zeros).
    The thresholds are always used: ``extend`` changes nothing.  Needs positive edge weights (no stored zeros).
    """

    _mode = "SparseNode2vecPlusPlus"
    _always_thresholds = True

    def get_noise_thresholds(self):
        """``DenseRWGraph.get_noise_thresholds`` (rw/dense_rw.py:11-19) of the dense float64 form: the native restatement
        of NumPy's reductions (``pw_noise_thresholds_csr_f64``), the NumPy loop itself when the library is not built."""
        data = np.ascontiguousarray(self.data, dtype=np.float32)
        indptr = np.ascontiguousarray(self.indptr, dtype=np.uint32)
        n = self.num_nodes
        thr = np.zeros(n, dtype=np.float32)
        try:
            from . import _lib

            lib = _lib.load()
        except Exception:  # library not built
            lib = None
        if lib is not None:
            _lib.check(lib.pw_noise_thresholds_csr_f64(indptr.ctypes.data, data.ctypes.data, n, float(self.gamma),
                                                       thr.ctypes.data))
            return thr
        with np.errstate(invalid="ignore", divide="ignore"):
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                for i in range(n):
                    w = data[indptr[i]:indptr[i + 1]].astype(np.float64)
                    w = w[w != 0]
                    thr[i] = w.mean() + self.gamma * w.std()
        return np.maximum(thr, 0)

    def setup_get_normalized_probs(self):
        """``(get_normalized_probs, noise_thresholds)``: the node2vec++ probabilities and the thresholds they use."""
        return self.get_normalized_probs, self.get_noise_thresholds()

    def get_normalized_probs(self, data, indices, indptr, p, q, cur_idx, prev_idx=None, average_weight_ary=None):
        """node2vec++ transition probabilities over ``cur_idx``'s neighbours (float64), with ``_SparseBase``'s signature.
        Computed on the GPU from the graph this object holds (``pw_probs``): the probabilities the walk kernel samples
        from, bit for bit; ``data``, ``indices``, ``indptr`` and ``average_weight_ary`` are not read."""
        eng = self._get_engine()
        return eng.probs(self._mode, p, q, False, cur_idx, prev_idx)
