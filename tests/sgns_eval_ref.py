"""The skip-gram session's read-only scoring pass and its change of corpus, restated in NumPy (TEST INFRASTRUCTURE ONLY; nothing
under ``pecanpy_amd/`` imports it): tests/sgns_session_ref.py's ``Session`` plus what ``pw_sgns_evaluate`` and
``pw_sgns_set_walks`` add (include/pecanpy_amd.h):

* ``evaluate(walks=None, epoch=None)``: ``_epoch``'s loops with the update lines removed -- the same hashes from the item base
  ``n_walks * (L + 1) * epoch`` of the matrix that is scored, the same subsampling, windows and negatives, the loss term of every
  evaluation from the vectors as they are; the per-walk sums are added in ascending walk order.  No learning rate is computed
  and nothing is written;
* ``set_walks(walks, recount=False)``: another matrix of the same shape; with ``recount`` the noise table and the keep
  probabilities are rebuilt from it as the constructor builds them, otherwise they stay."""
import numpy as np

import sgns_session_ref
from sgns_f64 import _F32, _GOLD, _MASK, _mix
from sgns_session_ref import softplus


def _rows_of(walks):
    mat = np.asarray(walks, dtype=np.uint32)
    L1 = mat.shape[1] - 1
    return [[int(x) for x in mat[wk, :int(mat[wk, L1])]] for wk in range(mat.shape[0])], L1


class Session(sgns_session_ref.Session):
    def __init__(self, walks, n_nodes, sample=1e-3, **kw):
        super().__init__(walks, n_nodes, sample=sample, **kw)
        self.n_nodes, self.sample = n_nodes, sample

    def set_walks(self, walks, recount=False):
        rows, L1 = _rows_of(walks)
        if (len(rows), L1) != (self.n_walks, self.L1):
            raise ValueError("another shape needs a session of its own")
        if recount:
            fresh = sgns_session_ref.Session(walks, self.n_nodes, dim=1, sample=self.sample, seed=self.seed)
            self.table, self.keep = fresh.table, fresh.keep
        self.rows = rows

    def evaluate(self, walks=None, epoch=None):
        T = self.dtype
        rows, L1 = (self.rows, self.L1) if walks is None else _rows_of(walks)
        epoch = self.state["epoch"] if epoch is None else epoch
        item_base = len(rows) * L1 * epoch
        window, negative, table, keep, seed = self.window, self.negative, self.table, self.keep, self.seed
        table_size = table.size
        syn0, syn1 = self.syn0, self.syn1
        walk_loss = []
        kept_total = pairs = evaluations = 0
        for wk, row in enumerate(rows):
            occ = [_mix(seed ^ ((item_base + wk * L1 + p) * _GOLD & _MASK)) for p in range(len(row))]
            if keep is None:
                kept = list(range(len(row)))
            else:
                kept = [p for p in range(len(row)) if _F32(occ[p] >> 40) * _F32(1.0 / 16777216.0) < keep[row[p]]]
            kept_total += len(kept)
            loss = 0.0
            for j, pos in enumerate(kept):
                rs = _mix(occ[pos])
                eff = window - rs % window
                centre = row[pos]
                for i in range(j - min(eff, j), j + min(eff, len(kept) - 1 - j) + 1):
                    if i == j:
                        continue
                    c = kept[i]
                    rs = _mix(rs + c)
                    v = syn0[row[c]]
                    for ng in range(negative + 1):
                        target = centre
                        if ng:
                            rs = _mix(rs + ng)
                            target = int(table[((rs >> 16) & 0xFFFFFFFF) % table_size])
                            if target == centre:
                                continue
                        dot = T(np.dot(v, syn1[target]))
                        loss += softplus(-dot if ng == 0 else dot)
                        evaluations += 1
                    pairs += 1
            walk_loss.append(loss)
        total = 0.0
        for x in walk_loss:
            total += x
        return dict(loss=total, evaluations=evaluations, kept_occurrences=kept_total, trained_pairs=pairs)


def random_context_vectors(n_nodes, dim, seed=5):
    """A seeded ``syn1`` of the size of trained context vectors: with the initial zeros every dot product would be 0."""
    return (np.random.default_rng(seed).standard_normal((n_nodes, dim)) * 0.5).astype(np.float32)
