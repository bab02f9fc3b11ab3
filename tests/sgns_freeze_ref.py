"""The skip-gram session WITH FROZEN ROWS, restated in NumPy (TEST INFRASTRUCTURE ONLY; nothing under ``pecanpy_amd/`` imports
it): tests/sgns_session_ref.py's ``Session`` with the same loop, in which the write-back of ``v`` (a row of ``syn0``) and of ``u``
(a row of ``syn1``) is skipped for a locked row while ``neu1e`` is still accumulated from a locked target.  Everything that is
EVALUATED -- pairs, draws, ``dot``, the loss, ``g``, the counts -- is the unlocked session's code on the values at hand; with no
lock the class is tests/sgns_session_ref.py bit for bit (tests/test_sgns_freeze_host.py).

``coverage`` counts what the cases must reach (tests/test_sgns_freeze_host.py asserts it, so the cases cannot go hollow):
``locked_target_twice_in_group`` -- a locked ``syn1`` row trained twice within one group of ``GROUP`` targets (the kernel's
re-read path on a row nobody wrote); ``locked_ctx_free_target`` / ``free_ctx_locked_target`` -- evaluations of those kinds.

The fixed lock sets of the cases: ids 0-2 are the most frequent of the geometric corpus of tests/sgns_session_cases.py, so they
repeat inside a target group; ids 17 and 19 occur in no walk."""
import functools

import numpy as np

import sgns_session_cases as sc
import sgns_session_ref as ref
from sgns_f64 import _F32, _GOLD, _MASK, _mix

GROUP = 6                                  # csrc/sgns.hip.h: SGNS_GROUP
LOCK0 = (0, 1, 5, 16, 17)                  # frozen rows of syn0
LOCK1 = (0, 2, 16, 19)                     # frozen rows of syn1


def mask_of(rows, n):
    m = np.zeros(n, dtype=bool)
    m[list(rows)] = True
    return m


class Session(ref.Session):
    def __init__(self, walks, n_nodes, lock0=(), lock1=(), **kw):
        super().__init__(walks, n_nodes, **kw)
        self.freeze(lock0, lock1)
        self.coverage = dict(locked_target_twice_in_group=0, locked_ctx_free_target=0, free_ctx_locked_target=0)

    def freeze(self, lock0=(), lock1=()):
        n = self.syn0.shape[0]
        self.lock0, self.lock1 = mask_of(lock0, n), mask_of(lock1, n)

    def _epoch(self, item_base, lr_base, lr_total):
        T = self.dtype
        alpha, min_alpha = self.state["alpha"], self.state["min_alpha"]
        window, negative, table, keep, L1, seed = self.window, self.negative, self.table, self.keep, self.L1, self.seed
        table_size = table.size
        syn0, syn1, lock0, lock1, cov = self.syn0, self.syn1, self.lock0, self.lock1, self.coverage
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
                    ctx = row[c]
                    v = syn0[ctx]
                    neu1e = np.zeros(self.dim, dtype=T)
                    in_group = []                                               # locked targets trained in the current group
                    for ng in range(negative + 1):
                        if ng % GROUP == 0:
                            in_group = []
                        target = centre
                        if ng:
                            rs = _mix(rs + ng)
                            target = int(table[((rs >> 16) & 0xFFFFFFFF) % table_size])
                            if target == centre:
                                continue
                        u = syn1[target]
                        dot = T(np.dot(v, u))
                        loss += ref.softplus(-dot if ng == 0 else dot)
                        evaluations += 1
                        if dot > 6.0:
                            sig = one
                        elif dot < -6.0:
                            sig = zero
                        else:
                            sig = one / (one + np.exp(-dot))
                        g = ((one if ng == 0 else zero) - sig) * lr
                        neu1e += g * u                                          # (from a locked target too)
                        if not lock1[target]:
                            u += g * v                                          # (a view: the row itself)
                        else:
                            cov["locked_target_twice_in_group"] += target in in_group
                            in_group.append(target)
                        cov["locked_ctx_free_target"] += bool(lock0[ctx] and not lock1[target])
                        cov["free_ctx_locked_target"] += bool(lock1[target] and not lock0[ctx])
                    if not lock0[ctx]:
                        v += neu1e
                    pairs += 1
            walk_loss.append(loss)
        total = 0.0
        for x in walk_loss:
            total += x
        return dict(loss=total, evaluations=evaluations, kept_occurrences=kept_total, trained_pairs=pairs)


@functools.lru_cache(maxsize=None)
def reference(param, dtype="float64"):
    """The locked restatement on a case of tests/sgns_session_cases.py with ``LOCK0`` / ``LOCK1``: both matrices before and
    after the ``EPOCHS`` epochs of the schedule, the records, the state and the coverage.  Nobody writes to the arrays."""
    s = Session(sc.corpus(), sc.N_NODES, lock0=LOCK0, lock1=LOCK1, dtype=np.dtype(dtype), **sc.kw_of(param))
    before0, before1 = s.syn0.astype(np.float64), s.syn1.astype(np.float64)
    records = s.run(sc.EPOCHS)
    out = dict(before0=before0, before1=before1, syn0=s.syn0.astype(np.float64), syn1=s.syn1.astype(np.float64), records=list(records),
               state=dict(s.state), coverage=dict(s.coverage))
    for a in (out["before0"], out["before1"], out["syn0"], out["syn1"]):
        a.setflags(write=False)
    return out


def loss_gap(param):
    """The largest relative distance, over the epochs of a locked case, between the epoch losses of the float32 and the float64
    lock restatement (as ``sgns_session_cases.loss_gap``)."""
    r64, r32 = reference(param), reference(param, "float32")
    gaps = []
    for a, b in zip(r64["records"], r32["records"]):
        assert a["evaluations"] == b["evaluations"]
        gaps.append(abs(b["loss"] - a["loss"]) / a["loss"])
    return max(gaps)
