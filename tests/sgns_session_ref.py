"""The skip-gram trainer as a SESSION, restated in NumPy (TEST INFRASTRUCTURE ONLY; nothing under ``pecanpy_amd/`` imports it):
tests/sgns_f64.py's algorithm -- the same hashes, the same float32 discrete decisions and learning rate, the same vector
operations in the same order -- plus what ``pw_sgns`` adds (include/pecanpy_amd.h):

* the state: ``epoch`` (the global epoch index of the hashes), ``sched_pos`` / ``sched_total`` (where the learning rate stands),
  ``alpha``, ``min_alpha``; ``run(n)`` trains the next ``n`` epochs, ``reschedule`` starts a new schedule on the vectors;
* the loss of an epoch: for every trained evaluation ``softplus(-dot)`` (centre) or ``softplus(dot)`` (negative), with
  ``softplus(x) = max(x, 0) + log1p(exp(-|x|))`` in float64, from the ``dot`` the update uses, before the update and whether
  or not the sigmoid is clipped; summed per walk in evaluation order, the walks then in ascending order;
* ``syn1`` is kept.

``dtype=np.float64`` (default) is tests/sgns_f64.py bit for bit (tests/test_sgns_session_host.py); ``dtype=np.float32`` rounds
every vector value, the dot product, the sigmoid and the gradient to float32 -- ``np.dot``'s order and NumPy's ``exp``, not the
kernel's lane order and fast ``exp``: its distance from the float64 run is the scale of a float32 trainer's own error, from
which the loss tolerance of tests/test_gpu_sgns_session.py is taken."""
import math

import numpy as np

import sgns_f64
from sgns_f64 import _F32, _GOLD, _MASK, _mix


def softplus(x):
    x = float(x)
    return max(x, 0.0) + math.log1p(math.exp(-abs(x)))


class Session:
    def __init__(self, walks, n_nodes, dim=128, window=10, epochs=1, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=0,
                 dtype=np.float64):
        mat = np.asarray(walks, dtype=np.uint32)
        self.n_walks, L = mat.shape[0], mat.shape[1] - 2
        self.L1 = L + 1
        lengths = [int(x) for x in mat[:, self.L1]]
        self.rows = [[int(x) for x in mat[wk, :lengths[wk]]] for wk in range(self.n_walks)]
        self.seed = int(seed) & 0xFFFFFFFF
        self.dim, self.window, self.negative, self.dtype = dim, window, negative, np.dtype(dtype).type
        cnt = np.zeros(n_nodes, dtype=np.int64)
        for r in self.rows:
            np.add.at(cnt, r, 1)
        total = float(cnt.sum())
        self.table = sgns_f64.noise_table(cnt)
        sample = _F32(sample)
        self.keep = None
        if sample > 0:
            thr = float(sample) * total
            with np.errstate(divide="ignore", invalid="ignore"):
                k = np.where(cnt > 0, (np.sqrt(cnt / thr) + 1.0) * thr / cnt, 1.0)
            self.keep = np.minimum(k, 1.0).astype(_F32)
        self.syn0 = sgns_f64.initial_vectors(n_nodes, dim, self.seed).astype(self.dtype)
        self.syn1 = np.zeros((n_nodes, dim), dtype=self.dtype)
        self.n_items = self.n_walks * self.L1
        self.state = dict(epoch=0, sched_pos=0, sched_total=int(epochs), alpha=_F32(alpha), min_alpha=_F32(min_alpha))

    def reschedule(self, epochs, alpha=None, min_alpha=None):
        st = self.state
        st.update(sched_pos=0, sched_total=int(epochs), alpha=st["alpha"] if alpha is None else _F32(alpha),
                  min_alpha=st["min_alpha"] if min_alpha is None else _F32(min_alpha))

    def run(self, n_epochs=1):
        st = self.state
        if st["sched_pos"] + n_epochs > st["sched_total"]:
            raise ValueError("run past the end of the schedule")
        out = []
        for _ in range(n_epochs):
            out.append(self._epoch(self.n_items * st["epoch"], self.n_items * st["sched_pos"], self.n_items * st["sched_total"]))
            st["epoch"] += 1
            st["sched_pos"] += 1
        return out

    def _epoch(self, item_base, lr_base, lr_total):
        T = self.dtype
        alpha, min_alpha = self.state["alpha"], self.state["min_alpha"]
        window, negative, table, keep, L1, seed = self.window, self.negative, self.table, self.keep, self.L1, self.seed
        table_size = table.size
        syn0, syn1 = self.syn0, self.syn1
        one, zero = T(1.0), T(0.0)
        walk_loss = []
        kept_total = pairs = evaluations = 0
        for wk in range(self.n_walks):
            row = self.rows[wk]
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
                q = _F32(float(lr_base + wk * L1 + pos) / float(lr_total))
                lr = alpha - (alpha - min_alpha) * q                            # float32 throughout
                lr = T(max(lr, min_alpha))
                centre = row[pos]
                for i in range(j - min(eff, j), j + min(eff, len(kept) - 1 - j) + 1):
                    if i == j:
                        continue
                    c = kept[i]
                    rs = _mix(rs + c)
                    v = syn0[row[c]]
                    neu1e = np.zeros(self.dim, dtype=T)
                    for ng in range(negative + 1):
                        target = centre
                        if ng:
                            rs = _mix(rs + ng)
                            target = int(table[((rs >> 16) & 0xFFFFFFFF) % table_size])
                            if target == centre:
                                continue
                        u = syn1[target]
                        dot = T(np.dot(v, u))
                        loss += softplus(-dot if ng == 0 else dot)
                        evaluations += 1
                        if dot > 6.0:
                            sig = one
                        elif dot < -6.0:
                            sig = zero
                        else:
                            sig = one / (one + np.exp(-dot))
                        g = ((one if ng == 0 else zero) - sig) * lr
                        neu1e += g * u
                        u += g * v                                              # (a view: the row itself)
                    v += neu1e
                    pairs += 1
            walk_loss.append(loss)
        total = 0.0
        for x in walk_loss:
            total += x
        return dict(loss=total, evaluations=evaluations, kept_occurrences=kept_total, trained_pairs=pairs)


def train(walks, n_nodes, slices=None, dtype=np.float64, **kw):
    """``(session, per-epoch records)`` after the whole schedule, run in the given ``slices`` (default: at once)."""
    s = Session(walks, n_nodes, dtype=dtype, **kw)
    records = []
    for n in slices or [s.state["sched_total"]]:
        records += s.run(n)
    assert s.state["sched_pos"] == s.state["sched_total"]
    return s, records
