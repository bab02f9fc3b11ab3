"""The cases that hold the skip-gram trainer's ARITHMETIC to its references across its template and group space
(tests/test_sgns_shapes_host.py, tests/test_gpu_sgns_shapes.py): every ``sgns_walk_kernel<PER>`` (``PER = ceil(dim / 64)``,
1..8) at both ends of its range and inside it, every way ``negative + 1`` targets fill the kernel's groups of six, both
saturated branches of the sigmoid, a noise table above its ``1 << 16`` floor, another learning-rate schedule, subsampling at
a wide instance, and one wide instance on four wavefronts.

A case is a small walk matrix and the trainer's keywords; its cost is its pairs (one wavefront trains them one after the
other), a few thousand at the most.  ``reach`` names what the float64 reference's diagnostics must show before the case
means anything (asserted in the host file):

``small_vocab``    draws that equal the centre occur, and (from two negatives on) targets that repeat inside a group of six
``second_group``   evaluations with draw index >= 6 occur, and targets that repeat ACROSS the group border
``sat_low`` / ``sat_high``   at least 20 evaluations with ``dot < -6`` / ``dot > 6``, none nearer than 1e-2 to the border
``thinned``        subsampling drops occurrences

Ids that occur in no walk lie directly after ids that do (``spread``: every other id; ``alternating``: two appended ids): a
store through a wrong lane guard into the next row lands on a row that must keep its initial bits."""
import functools

import numpy as np

from sgns_corpora import component_corpus

L = 30
SEED = 7


def spread(mat, stride):
    """The same walks with id ``i`` renamed ``stride * i``: the ids between stay unused."""
    out = np.array(mat, dtype=np.uint32)
    out[:, :-1] *= np.uint32(stride)
    return out


def small(stride=2):
    """Six walks over two components of six ids, lengths L + 1, 0, L, 1, L // 2, 2: 12 ids in use, 667 pairs per epoch at
    ``window=4`` without subsampling; the low ids of a component are frequent, so the noise table repeats them."""
    mat, n = component_corpus(2, 6, L, seed=1, lengths=[L + 1, 0, L, 1, L // 2, 2])
    return spread(mat, stride), (n - 1) * stride + 2


def alternating():
    """Six full walks, walk ``wk`` alternating the ids ``2p, 2p + 1`` with ``p = wk % 3``; ids 6 and 7 never occur.  Every
    pair trains the same few rows, so the dot products grow past 6 within a thousand pairs."""
    mat = np.zeros((6, L + 2), dtype=np.uint32)
    for wk in range(6):
        mat[wk, :L + 1] = 2 * (wk % 3) + np.arange(L + 1) % 2
    mat[:, L + 1] = L + 1
    return mat, 8


def four_components():
    """The parallel form's corpus (tests/sgns_corpora.py): walk ``wk`` names only ids of component ``wk % 4``; two more ids
    that never occur."""
    mat, n = component_corpus(4, 10, L, seed=3)
    return mat, n + 2


def _case(id, corpus, reach=(), workers=1, wavefronts=1, **kw):
    kw = dict(dict(window=4, epochs=2, negative=5, sample=0.0, seed=SEED), **kw)
    return dict(id=id, corpus=corpus, kw=kw, reach=frozenset(reach), workers=workers, wavefronts=wavefronts)


# both ends of every instance's range, and dim < 64 that is no multiple of 4
EDGE_DIMS = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512]
# inside the range of the instances 2, 5 and 7 (3, 4 and 6: the group and subsampling cases below)
INTERIOR_DIMS = [100, 300, 420]

CASES = [_case(f"dim-{dim}", small, ["small_vocab"], dim=dim) for dim in EDGE_DIMS + INTERIOR_DIMS]
# negative + 1 targets in groups of six: 2, 3, 5 (a partly filled group), 7, 8 (one full, one partly filled), 12 (two full),
# 13, 14 (a third group)
CASES += [_case(f"negative-{neg}", small, ["small_vocab"] + ["second_group"] * (neg >= 6), dim=24, negative=neg)
          for neg in (1, 2, 4, 6, 7, 11, 12, 13)]
CASES += [
    _case("negative-6-dim-150", small, ["small_vocab", "second_group"], dim=150, negative=6),
    _case("negative-12-dim-350", small, ["small_vocab", "second_group"], dim=350, negative=12),
    _case("saturated-low", alternating, ["sat_low"], dim=4, window=2, negative=3, alpha=0.2),
    _case("saturated-high", alternating, ["sat_high"], dim=8, window=2, negative=1, alpha=0.8, min_alpha=0.3, epochs=4, seed=2),
    # 16 * 5502 table slots, not 1 << 16; ids 0, 500, .. 5500 in use
    _case("table-above-its-floor", functools.partial(small, 500), ["small_vocab"], dim=8),
    _case("schedule", small, ["small_vocab"], dim=100, alpha=0.05, min_alpha=0.01),
    _case("subsampled-dim-230", small, ["small_vocab", "thinned"], dim=230, sample=0.05),
    # the parallel form at a wide instance: negative = 0, a component per wavefront (test_gpu_sgns_waves.py's yardstick)
    _case("four-wavefronts-dim-321", four_components, workers=4, wavefronts=4, dim=321, negative=0),
]
IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
ONE_WAVEFRONT = [c["id"] for c in CASES if c["workers"] == 1]
# one case per instance through the host-matrix entry as well
HOST_ENTRY = ["dim-63", "dim-128", "negative-6-dim-150", "subsampled-dim-230", "dim-300", "negative-12-dim-350", "dim-420",
              "dim-512"]


def per_of(dim):
    return (dim + 63) // 64


def bound(want):
    """The project's one-wavefront bound (tests/sgns_corpora.py: close_to_oracle)."""
    return 2e-5 * np.abs(want).max() + 1e-6


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """Both references of a case, computed once per process and shared; nobody writes to the arrays."""
    import sgns_f64
    from oracle import pyoracle as orc

    case = BY_ID[case_id]
    mat, n = case["corpus"]()
    kw = case["kw"]
    want64, diag = sgns_f64.train(mat, n, **kw)
    want32, _, counts32 = orc.sgns_train(mat, n, return_counts=True, **kw)
    ref = dict(mat=mat, n=n, kw=kw, want64=want64, diag=diag, want32=want32, counts32=counts32,
               saturated32=orc.sgns_train.last_saturated, initial=sgns_f64.initial_vectors(n, kw["dim"], kw["seed"]),
               e_ref=float(np.abs(want32 - want64).max()))
    valid = np.arange(mat.shape[1] - 1)[None, :] < mat[:, -1:].astype(np.int64)
    ref["unused"] = np.setdiff1d(np.arange(n), mat[:, :-1][valid])
    for a in (mat, want64, want32, ref["initial"], ref["unused"]):
        a.setflags(write=False)
    return ref
