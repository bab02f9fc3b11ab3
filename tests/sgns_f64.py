"""Skip-gram with negative sampling in float64 NumPy: a second, independent reference for the HIP trainer (TEST
INFRASTRUCTURE ONLY; nothing under ``pecanpy_amd/`` imports it).

Written from the algorithm as the header of oracle/sgns_ref.c states it (word2vec.c's sg / negative path with every random
choice a hash of (seed, epoch, walk, position[, context, draw])), not from the kernel:

* what decides a DISCRETE outcome or the schedule is evaluated in the number format the definition gives it: ``keep`` is a
  float32 compared with a 24-bit float32 draw, the learning rate is a float32 expression (the quotient in double, rounded to
  float32, then ``alpha - (alpha - min_alpha) * q`` in float32, clamped), ``syn0`` starts from the float32 initial values;
* every vector operation is float64: ``np.dot`` for the dot product, an exact ``exp`` in the sigmoid, the updates unrounded.

What it therefore does NOT share with oracle/sgns_ref.c and the kernel: the order of the dot product's sum, float32 rounding of
any vector value, the fast ``exp``.  The distance of the float32 restatement from this one is the restatement's own error.

Besides the vectors it returns what a test needs to know about a case before it trusts it: how often the sigmoid saturated
on either side and how close a dot product came to the border, how many draws equalled the centre, and -- for the kernel's
grouping of a pair's targets in sixes -- how many targets repeated an earlier one inside their group or across a group
border, and how many evaluations lay beyond the first group."""
import numpy as np

from sgns_corpora import mix64

SGNS_GROUP = 6   # csrc/sgns.hip.h: target rows requested together
_MASK = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15
_F32 = np.float32


def _mix(x):
    return int(mix64(x & _MASK))


def initial_vectors(n_nodes, dim, seed):
    """float32[n_nodes, dim]: syn0 ~ U(-0.5, 0.5) / dim from the seeded 64-bit LCG, 24 bits per value."""
    x = (_GOLD ^ ((int(seed) & 0xFFFFFFFF) << 17)) & _MASK
    bits = np.empty(n_nodes * dim, dtype=np.uint32)
    for i in range(bits.size):
        x = (x * 6364136223846793005 + 1442695040888963407) & _MASK
        bits[i] = (x >> 40) & 0xFFFFFF
    v = (bits.astype(_F32) / _F32(16777216.0) - _F32(0.5)) / _F32(dim)     # (float32 at every step, as defined)
    return v.reshape(n_nodes, dim)


def noise_table(cnt):
    """uint32[max(1 << 16, min(1 << 26, 16 n))]: word ``w`` owns the share ``cnt[w] ** 0.75 / sum`` of the slots."""
    n = cnt.size
    size = min(1 << 26, max(1 << 16, 16 * n))
    pw = cnt.astype(np.float64) ** 0.75
    pow_total = 0.0
    for x in pw:                                                              # (summed in id order, as defined)
        pow_total += float(x)
    table = np.empty(size, dtype=np.uint32)
    t, last, cum = 0, 0, 0.0
    for w in np.flatnonzero(cnt):
        last = int(w)
        cum += float(pw[w]) / pow_total
        # the word takes slots t .. end - 1, end the largest count with end / size <= cum (the definition walks there slot
        # by slot; the quotient is monotonic, so start near cum * size and settle the border with the same comparison)
        end = min(size, max(t, int(cum * size)))
        while end < size and (end + 1) / size <= cum:
            end += 1
        while end > t and end / size > cum:
            end -= 1
        table[t:end] = last
        t = end
    table[t:] = last
    return table


def train(walks, n_nodes, dim=128, window=10, epochs=1, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=0):
    """``(float64[n_nodes, dim], diagnostics)`` after ``epochs`` passes over the walks in sentence order."""
    mat = np.asarray(walks, dtype=np.uint32)
    n_walks, L = mat.shape[0], mat.shape[1] - 2
    L1 = L + 1
    lengths = [int(x) for x in mat[:, L1]]
    rows = [[int(x) for x in mat[wk, :lengths[wk]]] for wk in range(n_walks)]
    seed = int(seed) & 0xFFFFFFFF
    cnt = np.zeros(n_nodes, dtype=np.int64)
    for r in rows:
        np.add.at(cnt, r, 1)
    total = float(cnt.sum())
    table = noise_table(cnt)
    table_size = table.size
    alpha, min_alpha, sample = _F32(alpha), _F32(min_alpha), _F32(sample)
    keep = None
    if sample > 0:
        thr = float(sample) * total
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(cnt > 0, (np.sqrt(cnt / thr) + 1.0) * thr / cnt, 1.0)
        keep = np.minimum(k, 1.0).astype(_F32)
    syn0 = initial_vectors(n_nodes, dim, seed).astype(np.float64)
    syn1 = np.zeros((n_nodes, dim), dtype=np.float64)
    n_items = n_walks * L1
    item_total = n_items * epochs
    d = dict(occurrences=epochs * sum(lengths), kept=0, pairs=0, evaluations=0, saturated_high=0, saturated_low=0,
             margin=float("inf"), max_abs_dot=0.0, skipped_draws=0, in_group_repeats=0, cross_group_repeats=0,
             second_group_evaluations=0)
    for ep in range(epochs):
        item_base = n_items * ep
        for wk in range(n_walks):
            row = rows[wk]
            occ = [_mix(seed ^ ((item_base + wk * L1 + p) * _GOLD & _MASK)) for p in range(len(row))]
            if keep is None:
                kept = list(range(len(row)))
            else:
                kept = [p for p in range(len(row)) if _F32(occ[p] >> 40) * _F32(1.0 / 16777216.0) < keep[row[p]]]
            d["kept"] += len(kept)
            for j, pos in enumerate(kept):
                rs = _mix(occ[pos])
                eff = window - rs % window
                q = _F32(float(item_base + wk * L1 + pos) / float(item_total))
                lr = alpha - (alpha - min_alpha) * q                        # float32 throughout
                lr = float(max(lr, min_alpha))
                centre = row[pos]
                for i in range(j - min(eff, j), j + min(eff, len(kept) - 1 - j) + 1):
                    if i == j:
                        continue
                    c = kept[i]
                    rs = _mix(rs + c)
                    v = syn0[row[c]]
                    neu1e = np.zeros(dim)
                    trained = []                                            # (draw index, target) of this pair so far
                    for ng in range(negative + 1):
                        target = centre
                        if ng:
                            rs = _mix(rs + ng)
                            target = int(table[((rs >> 16) & 0xFFFFFFFF) % table_size])
                            if target == centre:
                                d["skipped_draws"] += 1
                                continue
                        if any(t == target and e // SGNS_GROUP == ng // SGNS_GROUP for e, t in trained):
                            d["in_group_repeats"] += 1
                        elif any(t == target for e, t in trained):
                            d["cross_group_repeats"] += 1
                        trained.append((ng, target))
                        d["second_group_evaluations"] += ng >= SGNS_GROUP
                        d["evaluations"] += 1
                        u = syn1[target]
                        dot = float(np.dot(v, u))
                        d["margin"] = min(d["margin"], abs(abs(dot) - 6.0))
                        d["max_abs_dot"] = max(d["max_abs_dot"], abs(dot))
                        if dot > 6.0:
                            sig = 1.0
                            d["saturated_high"] += 1
                        elif dot < -6.0:
                            sig = 0.0
                            d["saturated_low"] += 1
                        else:
                            sig = 1.0 / (1.0 + np.exp(-dot))
                        g = ((1.0 if ng == 0 else 0.0) - sig) * lr
                        neu1e += g * u
                        u += g * v                                          # (a view: the row itself)
                    v += neu1e
                    d["pairs"] += 1
    return syn0, d
