"""Experimental walk modes: the reference's ``pecanpy.experimental`` (src/pecanpy/experimental.py) on the MI355X walk engine.

``Node2vecPlusPlus`` is node2vec++, the reference authors' continuous form of node2vec+ for weighted dense graphs.  Its walks
run in ``walk_dense_weighted_kernel`` (csrc/walk_dense_w.hip.h) as a third bias form beside node2vec and node2vec+; seeded
runs reproduce the reference's single-thread walks bit for bit.
"""
from .pecanpy import _DenseBase

__all__ = ["Node2vecPlusPlus"]


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
