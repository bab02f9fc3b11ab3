"""The corpus, the parameter sets and the shared references of the skip-gram SESSION tests (tests/test_sgns_session_host.py,
tests/test_gpu_sgns_session.py).

The corpus: 12 walks of ``walk_length`` 9 (ten cells and the length cell) over 20 nodes; walk 3 has length 1, walk 7 is cut
short by its length cell (6 of its 10 ids count; the cells behind hold valid ids a trainer must not read); ids 17, 18 and 19
occur in no walk, so they are never a centre and own no slot of the noise table: their ``syn1`` rows stay zero and their
``syn0`` rows keep their initial bits.  Low ids are frequent, so ``SAMPLE`` thins them.  ``window`` is 3.

The parameter sets: ``dim`` 8 and 65 (a guarded tail at one and at two components per lane), 64 (exact), 130 (three per lane);
``negative`` 5 and 7 (the second target group); ``sample`` 0 and ``SAMPLE``.

A case costs about 600 pairs of up to 8 evaluations per epoch: the references are computed once per process and shared."""
import functools

import numpy as np

N_NODES = 20
N_WALKS = 12
L = 9
WINDOW = 3
EPOCHS = 3
SEED = 7
SAMPLE = 0.01
DIMS = (8, 64, 65, 130)
NEGATIVES = (5, 7)
SAMPLES = (0.0, SAMPLE)
PARAMS = [(dim, neg, sample) for dim in DIMS for neg in NEGATIVES for sample in SAMPLES]
IDS = [f"dim{dim}-neg{neg}-{'thinned' if sample else 'all'}" for dim, neg, sample in PARAMS]
RESCHEDULE = dict(epochs=1, alpha=0.01, min_alpha=0.01)


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(20)
    mat = np.zeros((N_WALKS, L + 2), dtype=np.uint32)
    mat[:, :L + 1] = np.minimum(rng.geometric(0.18, size=(N_WALKS, L + 1)) - 1, 16)
    mat[:, L + 1] = L + 1
    mat[3, L + 1] = 1
    mat[7, L + 1] = 6
    mat.setflags(write=False)
    return mat


def kw_of(param, **over):
    dim, negative, sample = param
    kw = dict(dim=dim, window=WINDOW, epochs=EPOCHS, negative=negative, sample=sample, seed=SEED)
    kw.update(over)
    return kw


def used_ids():
    mat = corpus()
    valid = np.arange(L + 1)[None, :] < mat[:, -1:].astype(np.int64)
    return np.unique(mat[:, :L + 1][valid])


def _snapshot(s, records):
    snap = dict(syn0=s.syn0.astype(np.float64), syn1=s.syn1.astype(np.float64), records=list(records), state=dict(s.state))
    for a in (snap["syn0"], snap["syn1"]):
        a.setflags(write=False)
    return snap


@functools.lru_cache(maxsize=None)
def reference(param, dtype="float64"):
    """The restatement on a case: ``schedule`` = after the ``EPOCHS`` epochs of the schedule, ``rescheduled`` = after one more
    epoch under ``RESCHEDULE`` (hash epoch 3).  Nobody writes to the arrays."""
    import sgns_session_ref as ref

    s = ref.Session(corpus(), N_NODES, dtype=np.dtype(dtype), **kw_of(param))
    records = s.run(EPOCHS)
    first = _snapshot(s, records)
    s.reschedule(**RESCHEDULE)
    return dict(schedule=first, rescheduled=_snapshot(s, s.run(1)))


def loss_gap(param):
    """The largest relative distance, over the epochs of a case (the rescheduled one included), between the epoch losses of
    the float32 and the float64 restatement."""
    r64, r32 = reference(param), reference(param, "float32")
    gaps = []
    for part in ("schedule", "rescheduled"):
        for a, b in zip(r64[part]["records"], r32[part]["records"]):
            assert a["evaluations"] == b["evaluations"]
            gaps.append(abs(b["loss"] - a["loss"]) / a["loss"])
    return max(gaps)


def bound(want):
    """The project's one-wavefront bound (tests/sgns_corpora.py: close_to_oracle)."""
    return 2e-5 * np.abs(want).max() + 1e-6


# ---- the racing run's corpus: two cliques -----------------------------------------------------------------------------------
CLIQUE_NODES = 16          # two cliques of 8
CLIQUE_KW = dict(dim=16, window=3, epochs=4, negative=5, sample=0.0, seed=11, alpha=0.05, min_alpha=0.05)


@functools.lru_cache(maxsize=None)
def clique_corpus(n_walks=64, L=19):
    """Uniform random walks on two disjoint cliques of 8 nodes: walk ``wk`` stays in clique ``wk % 2``.  A constant learning
    rate: the fall of the loss is the model learning which nodes share a clique, not the schedule."""
    rng = np.random.default_rng(5)
    mat = np.zeros((n_walks, L + 2), dtype=np.uint32)
    mat[:, :L + 1] = (np.arange(n_walks) % 2)[:, None] * 8 + rng.integers(0, 8, size=(n_walks, L + 1))
    mat[:, L + 1] = L + 1
    mat.setflags(write=False)
    return mat
