"""Walk matrices for the skip-gram tests that need no graph (the trainer reads only the matrix), and what those tests share.

``component_corpus`` builds a corpus on which the ORDER in which several wavefronts apply their updates cannot matter: walk
``wk`` names only ids of component ``wk % n_components``, so with ``negative=0`` (the centre is the only target of a pair) a
walk reads and writes only the ``syn0`` / ``syn1`` rows of its own component.  Wavefront ``w`` of ``n_components`` visits walks
``w, w + n_components, ...``: all of component ``w``, in ascending order, which is sentence order restricted to that
component.  The parallel result is then the sequential one bit for bit (tests/test_sgns_order_host.py shows it on the
restatement, tests/test_gpu_sgns_waves.py holds the kernel to it).  With negatives the noise table crosses components and
the construction no longer holds: that is the control."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def component_corpus(n_components, n_walks, L, ids_per_component=6, seed=0, lengths=None):
    """``(uint32[n_walks, L + 2], n_nodes)``: row ``wk`` holds random ids of component ``wk % n_components`` (component ``c``
    owns ids ``c * ids_per_component .. (c + 1) * ids_per_component - 1``; low ids of a component are the frequent ones, so
    that subsampling has words to thin), its last cell the number of ids that count.

    ``lengths=None``: every length cell is drawn from ``{0, 1, 2, L // 2, L, L + 1}``; a row of length 0, one of length 1
    and one of length ``L + 1`` (more than one ballot word of occurrences when ``L + 1 > 64``) are always there.  Otherwise
    ``lengths`` gives the length cell of every row.  The cells past a row's length hold ids of ANOTHER component: valid ids
    that a trainer reading past the length cell would train on, which breaks the construction visibly."""
    if n_components < 1 or n_walks < 3 or ids_per_component < 2:
        raise ValueError("component_corpus: at least one component, three walks and two ids per component")
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths = rng.choice(np.array([0, 1, 2, L // 2, L, L + 1]), size=n_walks)
        rows = rng.permutation(n_walks)[:3]
        lengths[rows] = [0, 1, L + 1]
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.shape != (n_walks,) or lengths.min() < 0 or lengths.max() > L + 1:
        raise ValueError("component_corpus: one length in 0 .. L + 1 per walk")
    if L + 1 > 64 and not (lengths > 64).any():
        raise ValueError("component_corpus: no row longer than one ballot word")
    comp = np.arange(n_walks) % n_components
    within = np.minimum(rng.geometric(0.5, size=(n_walks, L + 1)) - 1, ids_per_component - 1)
    mat = np.empty((n_walks, L + 2), dtype=np.uint32)
    mat[:, :L + 1] = comp[:, None] * ids_per_component + within
    other = ((comp + 1) % n_components)[:, None] * ids_per_component + within
    past = np.arange(L + 1)[None, :] >= lengths[:, None]
    mat[:, :L + 1][past] = other[past]
    mat[:, L + 1] = lengths
    return mat, n_components * ids_per_component


# The launches of pw_sgns_train_device that the parallel form is held to (tests/test_gpu_sgns_waves.py; the restatement under
# the same orders in tests/test_sgns_order_host.py).  ``wavefronts`` is what ``workers`` must become: the corpus has that many
# components, so another rounding would put two wavefronts on one component and fail loudly instead of racing silently.
# ``corpus_seed``: of the corpus alone; for the two cases with sample=0.05 it is one at which that rate thins visibly (a word
# is thinned once it holds more than 13 % of the corpus, so one component must outweigh the others; the host test asserts it).
# ``lengths``: rows of full length where the length is the point, short rows otherwise (the cost of a case is its pairs).
def _case(id, corpus_seed, L, dim, window, epochs, sample, workers, wavefronts, walks, lengths=None):
    return dict(id=id, corpus_seed=corpus_seed, L=L, dim=dim, window=window, epochs=epochs, sample=sample, workers=workers,
                wavefronts=wavefronts, walks=walks, lengths=lengths)


WAVE_CASES = [
    #     id                             seed     L  dim win ep sample workers waves walks
    # wib 1..3 of one workgroup, workers rounded up to it, a walk count that is no multiple of the wavefront count
    _case("round-up-to-a-workgroup",       92,   70,  24,  5, 3, 0.05,   2,  4, 37),
    _case("two-workgroups",               394,   70,  24,  5, 3, 0.05,   8,  8, 37),
    # three ballot words per row, two components per lane with a partly filled tail, keep == nullptr
    _case("three-ballot-words",           153,  130,  70,  4, 2, 0.0,    5,  8, 23),
    # many walks per wavefront: the fence between two walks
    _case("many-walks-per-wavefront",      80,   30,   8,  3, 2, 1e-3,  12, 12, 50),
    # eleven wavefronts without a walk: the counters are touched only by those that had one
    _case("idle-wavefronts",               35,   30,   8,  3, 1, 1e-3,  16, 16, 5),
    # four wavefronts and exactly 64 KiB of dynamic LDS (rows 1 and 6: wavefronts 1 and 2 fill their whole slice)
    _case("64KiB-four-wavefronts",       2056, 2047,   8,  3, 2, 0.0,    4,  4, 9, [150, 2048, 0, 1, 199, 64, 2048, 2, 100]),
    # the first length at which a workgroup is one wavefront; no rounding of workers
    _case("one-wavefront-per-workgroup", 2057, 2048,   8,  3, 2, 0.0,    3,  3, 9, [150, 2049, 0, 1, 199, 2049, 65, 2, 100]),
    # the largest accepted length: 64 KiB per workgroup of one wavefront
    _case("largest-length",              8196, 8191,   8,  2, 1, 0.0,    2,  2, 5, [130, 8192, 0, 1, 70]),
]
SEED = 7   # of the trainer, in every case


def case_corpus(case):
    return component_corpus(case["wavefronts"], case["walks"], case["L"], seed=case["corpus_seed"], lengths=case["lengths"])


def case_kw(case, **over):
    kw = dict(dim=case["dim"], window=case["window"], epochs=case["epochs"], sample=case["sample"], negative=0, seed=SEED)
    kw.update(over)
    return kw


def wavefront_major(n_walks, n_waves):
    """The order in which ``n_waves`` wavefronts taken ONE AFTER THE OTHER visit the walks: all walks of wavefront 0
    (0, n_waves, 2 n_waves, ...), then all of wavefront 1, and so on."""
    return np.concatenate([np.arange(w, n_walks, n_waves) for w in range(n_waves)]).astype(np.uint64)


def karate_walks(num_walks=20, L=40, seed=1, p=1.0, q=0.5):
    from oracle import pyoracle as orc

    k = np.load(os.path.join(GOLDEN, "karate_csr.npz"))
    starts = orc.shuffled_starts(34, num_walks, seed)
    return orc.walks_sparse_otf(k["indptr"], k["indices"], k["data"], p, q, starts, L, seed), 34


def on_device(walks):
    import torch

    return torch.from_numpy(np.ascontiguousarray(walks, dtype=np.uint32).view(np.int32)).cuda()


def close_to_oracle(got, want):
    """The project's one-wavefront bound (tests/test_gpu_sgns.py, tests/test_gpu_embed_device.py)."""
    err, bound = np.abs(got - want).max(), 2e-5 * np.abs(want).max() + 1e-6
    print(f"max|got - want| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= bound, (err, bound)


def run(d_walks, n, **kw):
    """``train_sgns_device`` as ``(vectors on the host, what the call did)``."""
    from pecanpy_amd.embed import train_sgns_device

    got = train_sgns_device(d_walks, n, **kw).cpu().numpy()
    return got, dict(train_sgns_device.last_stats)


def held_to_one_wavefront_and_the_restatement(mat, n, kw, workers, wavefronts=None):
    """What a run of several wavefronts on a component corpus with ``negative=0`` is held to (tests/test_gpu_sgns_waves.py;
    tests/test_gpu_sgns_shapes.py at a wide instance): (a) the wavefront count, (b) bit-equal to ``workers=1``, (c) the
    restatement within the one-wavefront bound, (d) its counters, (e) a second call bit-equal.  ``wavefronts=None``: any count
    above one."""
    from oracle import pyoracle as orc

    d_walks = on_device(mat)
    want, _, counts = orc.sgns_train(mat, n, return_counts=True, **kw)
    got, st = run(d_walks, n, workers=workers, **kw)
    print(f"wavefronts {st['wavefronts']}, kept {st['kept_occurrences']}, pairs {st['trained_pairs']} (restatement {counts})")
    if wavefronts is None:
        assert st["wavefronts"] > 1
    else:
        assert st["wavefronts"] == wavefronts                                                     # (a)
    one, st1 = run(d_walks, n, workers=1, **kw)
    assert st1["wavefronts"] == 1
    differing = np.flatnonzero((got != one).any(axis=1))
    assert np.array_equal(got, one), f"rows {differing[:8]} of {differing.size} differ from workers=1"   # (b)
    close_to_oracle(got, want)                                                                    # (c)
    assert (st["kept_occurrences"], st["trained_pairs"]) == counts                                # (d)
    assert (st1["kept_occurrences"], st1["trained_pairs"]) == counts
    again, st2 = run(d_walks, n, workers=workers, **kw)
    assert np.array_equal(again, got)                                                             # (e)
    assert (st2["kept_occurrences"], st2["trained_pairs"], st2["wavefronts"]) == counts + (st["wavefronts"],)
    assert np.array_equal(d_walks.cpu().numpy().view(np.uint32), mat)                             # read, never written
    return got


# ---- the two counters, evaluated independently of oracle/sgns_ref.c ---------------------------------------------------------
_M1, _M2, _GOLD = np.uint64(0xff51afd7ed558ccd), np.uint64(0xc4ceb9fe1a85ec53), np.uint64(0x9E3779B97F4A7C15)


def mix64(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= _M1
    x ^= x >> np.uint64(33)
    x *= _M2
    x ^= x >> np.uint64(33)
    return x


def counts_by_numpy(mat, n_nodes, window, epochs, sample, seed):
    """``(kept_occurrences, trained_pairs)`` from the two hashes alone: an occurrence (epoch, walk, position) survives when
    the 24-bit draw of ``mix64(seed ^ item * golden)`` is below the float32 ``keep`` of its word; the centre at index ``j``
    of the ``nk`` survivors of a walk trains ``min(eff, j) + min(eff, nk - 1 - j)`` pairs, ``eff = window - mix64(that
    hash) % window``.  No vector is touched."""
    mat = np.asarray(mat, dtype=np.uint32)
    n_walks, L = mat.shape[0], mat.shape[1] - 2
    lengths = mat[:, L + 1].astype(np.int64)
    valid = np.arange(L + 1)[None, :] < lengths[:, None]
    cnt = np.bincount(mat[:, :L + 1][valid], minlength=n_nodes).astype(np.float64)
    keep = None
    if sample > 0:
        thr = float(np.float32(sample)) * cnt.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(cnt > 0, (np.sqrt(cnt / thr) + 1.0) * thr / cnt, 1.0)
        keep = np.minimum(k, 1.0).astype(np.float32)
    item = (np.arange(n_walks, dtype=np.uint64)[:, None] * np.uint64(L + 1) + np.arange(L + 1, dtype=np.uint64)[None, :])
    kept_total = pairs_total = 0
    with np.errstate(over="ignore"):
        for ep in range(epochs):
            occ = mix64(np.uint64(seed) ^ (np.uint64(n_walks * (L + 1) * ep) + item) * _GOLD)
            kept = valid.copy()
            if keep is not None:
                draw = (occ >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
                kept &= draw < keep[np.where(valid, mat[:, :L + 1], 0)]
            eff = (np.uint64(window) - mix64(occ) % np.uint64(window)).astype(np.int64)
            for wk in range(n_walks):
                e = eff[wk][kept[wk]]
                nk = e.size
                j = np.arange(nk)
                kept_total += nk
                pairs_total += int((np.minimum(e, j) + np.minimum(e, nk - 1 - j)).sum())
    return kept_total, pairs_total
