"""Skip-gram embeddings from a walk matrix on the GPU (reference: gensim ``Word2Vec(walks, sg=1, ...)`` in
``Base.embed`` / ``cli.learn_embeddings``, src/pecanpy/pecanpy.py:276-290, cli.py:307-325).

``save_word2vec_format_device`` writes the text file of the vectors from device memory (``pw_vectors_write_text_device``,
csrc/emb_text.hip.h: exact ``%.6f`` on the GPU, only the text crosses to the host), byte for byte what
``save_word2vec_format`` writes.

``train_sgns_device`` runs word2vec's skip-gram-with-negative-sampling update as a HIP kernel (``pw_sgns_train_device``,
csrc/sgns.hip.h: a wavefront owns a walk) on the ``[n_jobs, L+2]`` matrix where ``WalkEngine.simulate_device`` leaves it, in
device memory -- no host copy of the matrix and no ``List[List[str]]`` corpus in between; ``train_sgns`` is the same
trainer for a matrix that lives on the host (upload, same kernel, download), ``train_sgns_file`` for a walk corpus file
(``corpus.read_walks_device``: read and numbered in device memory).  Same model and defaults as gensim's
(negative=5, ns_exponent=0.75, sample=1e-3, alpha 0.025 -> 1e-4, shrunk windows over the subsampled walk); not
bit-comparable with gensim's own random streams -- the deterministic single-wavefront mode is checked against a sequential
CPU restatement of the algorithm instead (tests/test_gpu_sgns.py, tests/test_gpu_embed_device.py).

``SgnsSession`` is the same trainer kept between launches (``pw_sgns``): epochs in slices, the loss of every epoch, both
matrices, a checkpoint file, a new schedule on trained vectors (tests/test_gpu_sgns_session.py); ``sgns_session_file`` opens
one on a corpus file.  ``SgnsSession.evaluate`` scores any walk matrix with the vectors as they are, by a read-only kernel, and
``SgnsSession.set_walks`` puts another corpus of the same shape under the session (tests/test_gpu_sgns_eval.py).

``KnnIndex`` answers nearest-neighbour queries on the vectors in device memory (``pw_knn``, csrc/knn.hip.h): exact float64
scores by one written definition, ties ordered by row number, bit for bit what ``knn_host`` states in NumPy
(tests/test_knn_host.py, tests/test_gpu_knn.py); ``SgnsSession.most_similar`` / ``knn_index`` query a session's vectors.
``KnnIndex.score_pairs`` / ``SgnsSession.score_pairs`` score given pairs of rows by the same definition; ``auc``, ``link_auc``
and the host statements of link prediction live in ``linkpred.py`` and are re-exported here.
"""
import ctypes as C

import numpy as np

from . import _lib
from .linkpred import auc, auc_host, link_auc, sample_non_edges_host, score_pairs_host   # noqa: F401  (link prediction: linkpred.py)

__all__ = ["train_sgns", "train_sgns_device", "train_sgns_file", "save_word2vec_format", "save_word2vec_format_device",
           "SgnsSession", "sgns_session_file", "KnnIndex", "knn_host", "auc", "auc_host", "link_auc", "sample_non_edges_host",
           "score_pairs_host"]


def train_sgns(walk_matrix, num_nodes, dim=128, window=10, epochs=1, negative=5, alpha=0.025, min_alpha=1e-4,
               sample=1e-3, seed=None, device=0, workers=0):
    """float32[num_nodes, dim] input vectors (``wv``) after ``epochs`` passes over the walks.

    ``workers=0`` (default): hogwild, as many wavefronts as the corpus feeds; ``workers=1``: one wavefront in sentence
    order -- deterministic under ``seed`` (the counterpart of gensim's ``workers=1``), slow."""
    lib = _lib.load()
    mat = np.ascontiguousarray(walk_matrix, dtype=np.uint32)
    if mat.ndim != 2 or mat.shape[1] < 3:
        raise ValueError("walk matrix must be uint32[n_walks, walk_length + 2]")
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    out = np.zeros((int(num_nodes), int(dim)), dtype=np.float32)
    _lib.check(lib.pw_sgns_train(int(device), mat.ctypes.data, mat.shape[0], mat.shape[1] - 2, int(num_nodes), int(dim),
                                 int(window), int(negative), int(epochs), float(alpha), float(min_alpha), float(sample),
                                 int(seed) & 0xFFFFFFFF, int(workers), out.ctypes.data))
    return out


def train_sgns_device(d_walks, num_nodes, dim=128, window=10, epochs=1, negative=5, alpha=0.025, min_alpha=1e-4,
                      sample=1e-3, seed=None, workers=0, out=None):
    """``train_sgns`` on a walk matrix in device memory: ``d_walks`` is what ``WalkEngine.simulate_device`` returns, a
    contiguous int32 CUDA tensor ``[n_walks, walk_length + 2]`` (uint32 storage).  Returns a ``float32[num_nodes, dim]``
    tensor on the same device (``out`` when given: contiguous, that shape, dtype and device).  The matrix never visits the
    host.  What the call did (``pw_sgns_stats``: ``vocab_ms``, ``init_ms``, ``train_ms``, ``kept_occurrences``,
    ``trained_pairs``, ``wavefronts``) is left in ``train_sgns_device.last_stats``."""
    import torch

    if not isinstance(d_walks, torch.Tensor) or not d_walks.is_cuda or d_walks.dtype != torch.int32 or not d_walks.is_contiguous():
        raise ValueError("d_walks must be a contiguous int32 CUDA tensor")
    if d_walks.dim() != 2 or d_walks.shape[1] < 3:
        raise ValueError("walk matrix must be int32[n_walks, walk_length + 2]")
    shape = (int(num_nodes), int(dim))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=d_walks.device)
    elif (not isinstance(out, torch.Tensor) or out.device != d_walks.device or out.dtype != torch.float32
          or tuple(out.shape) != shape or not out.is_contiguous()):
        raise ValueError("out must be a contiguous float32[num_nodes, dim] tensor on the device of d_walks")
    lib = _lib.load()
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    torch.cuda.current_stream(d_walks.device).synchronize()  # the matrix was produced on torch's stream
    st = _lib.PwSgnsStats()
    _lib.check(lib.pw_sgns_train_device(d_walks.device.index, C.c_void_p(d_walks.data_ptr()), d_walks.shape[0], d_walks.shape[1] - 2,
                                        shape[0], shape[1], int(window), int(negative), int(epochs), float(alpha), float(min_alpha),
                                        float(sample), int(seed) & 0xFFFFFFFF, int(workers), C.c_void_p(out.data_ptr()), C.byref(st)))
    train_sgns_device.last_stats = st.as_dict()
    return out


train_sgns_device.last_stats = None

MAX_WALK_LENGTH = 8191   # pw_sgns_train_device: a wavefront holds its walk in LDS (walk_length < 8192)


def train_sgns_file(path, dim=128, window=10, epochs=1, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=None,
                    workers=0, device=0):
    """``train_sgns_device`` on a walk corpus FILE (what ``pecanpy --task walks`` / ``Base.walks_to_file`` write, or any
    trainer's ``LineSentence`` input): ``corpus.read_walks_device`` reads it into device memory, the names numbered by first
    appearance, and the trainer runs on that matrix with ``num_nodes = len(names)``.  Returns ``(names, d_vectors)``:
    ``d_vectors[i]`` is the vector of ``names[i]``, a ``float32[len(names), dim]`` tensor on ``device``.  A corpus without
    lines is a ``ValueError`` before any device work; so is a line of more than ``MAX_WALK_LENGTH + 1`` tokens, before the
    trainer starts.  ``train_sgns_file.last_stats``: ``"read"`` (``read_walks_device.last_stats``) and ``"train"``
    (``train_sgns_device.last_stats``)."""
    d_walks, names = _corpus_matrix(path, device)
    d_vectors = train_sgns_device(d_walks, len(names), dim=dim, window=window, epochs=epochs, negative=negative, alpha=alpha,
                                  min_alpha=min_alpha, sample=sample, seed=seed, workers=workers)
    train_sgns_file.last_stats = {"read": _corpus_matrix.last_stats, "train": train_sgns_device.last_stats}
    return names, d_vectors


train_sgns_file.last_stats = None


def _corpus_matrix(path, device):
    """``(d_walks, names)`` of a walk corpus file as the trainer takes them, with ``train_sgns_file``'s errors."""
    import os

    from .corpus import read_walks_device

    if os.path.getsize(path) == 0:
        raise ValueError(f"{path}: a corpus without lines has nothing to train on")
    d_walks, names = read_walks_device(path, device=device)
    walk_length = d_walks.shape[1] - 2
    if walk_length > MAX_WALK_LENGTH:
        raise ValueError(f"{path}: a line of {walk_length + 1} tokens exceeds the trainer's walk length limit "
                         f"(at most {MAX_WALK_LENGTH + 1} tokens per line)")
    if not names:
        raise ValueError(f"{path}: a corpus without tokens has nothing to train on")
    if walk_length < 1:   # (lines of one token: no pairs; the trainer's matrix form needs walk_length >= 1)
        import torch

        d_walks = torch.cat([d_walks[:, :1], torch.zeros_like(d_walks[:, :1]), d_walks[:, 1:]], dim=1).contiguous()
    _corpus_matrix.last_stats = read_walks_device.last_stats
    return d_walks, names


_corpus_matrix.last_stats = None


def sgns_session_file(path, dim=128, window=10, epochs=1, negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=None,
                      workers=0, device=0, compute_loss=False):
    """``train_sgns_file``'s twin: ``(names, session)``, an ``SgnsSession`` on the matrix read from the corpus file (same
    reader, same errors), nothing trained yet.  ``session.vectors()[i]`` is the vector of ``names[i]``."""
    d_walks, names = _corpus_matrix(path, device)
    return names, SgnsSession(d_walks, len(names), dim=dim, window=window, epochs=epochs, negative=negative, alpha=alpha,
                              min_alpha=min_alpha, sample=sample, seed=seed, workers=workers, compute_loss=compute_loss)


class SgnsSession:
    """The trainer of ``train_sgns_device`` kept between launches (``pw_sgns``, include/pecanpy_amd.h): the vocabulary stage
    and the initialisation run once, in the constructor; ``run`` trains the next epochs of the learning-rate schedule, one
    launch each, and reports every epoch; both matrices can be read and replaced; ``save`` / ``restore`` checkpoint a run;
    ``reschedule`` starts a new schedule on the trained vectors; ``evaluate`` scores walks without training and ``set_walks``
    changes the corpus; ``freeze`` keeps chosen rows of either matrix exactly as they are while the others train.
    ``epochs`` is the LENGTH of the schedule: ``run(1)``
    ``epochs`` times, ``run(epochs)`` once and ``train_sgns_device(epochs=epochs)`` train the same vectors -- at ``workers=1``
    bit for bit, since every random choice is a hash of (seed, epoch, walk, position) and the learning rate a function of the
    position in the schedule.

    ``compute_loss``: every epoch also reports gensim's skip-gram / negative-sampling loss, the sum over the trained
    evaluations of ``softplus(-dot)`` (centre) or ``softplus(dot)`` (negative), from the dot product the update used, before
    the update.  The vectors do not depend on the flag.

    The session holds a reference to ``d_walks`` (the library borrows the matrix) and is a context manager; after ``close``
    every use is a ``ValueError``."""

    def __init__(self, d_walks, num_nodes, dim=128, window=10, epochs=1, negative=5, alpha=0.025, min_alpha=1e-4,
                 sample=1e-3, seed=None, workers=0, compute_loss=False):
        import torch

        self._handle = None
        num_nodes, dim, window, epochs, negative, workers = (int(x) for x in (num_nodes, dim, window, epochs, negative, workers))
        if num_nodes < 1:
            raise ValueError("num_nodes must be positive")
        if not 1 <= dim <= 512:
            raise ValueError("dim must be in 1..512")
        if window < 1 or epochs < 1:
            raise ValueError("window and epochs must be positive")
        if negative < 0 or workers < 0:
            raise ValueError("negative and workers must not be negative")
        if not (np.isfinite(alpha) and np.isfinite(min_alpha) and np.isfinite(sample)) or sample < 0:
            raise ValueError("alpha, min_alpha and sample must be finite, sample not negative")
        if not isinstance(d_walks, torch.Tensor) or not d_walks.is_cuda or d_walks.dtype != torch.int32 or not d_walks.is_contiguous():
            raise ValueError("d_walks must be a contiguous int32 CUDA tensor")
        if d_walks.dim() != 2 or d_walks.shape[1] < 3:
            raise ValueError("walk matrix must be int32[n_walks, walk_length + 2]")
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1)[0])
        self.params = dict(dim=dim, window=window, epochs=epochs, negative=negative, alpha=float(alpha), min_alpha=float(min_alpha),
                           sample=float(sample), seed=int(seed) & 0xFFFFFFFF, workers=workers, compute_loss=bool(compute_loss))
        self.num_nodes = num_nodes
        self.d_walks = d_walks
        self.last_stats = None
        lib = _lib.load()
        torch.cuda.current_stream(d_walks.device).synchronize()  # the matrix was produced on torch's stream
        handle = C.c_void_p()
        _lib.check(lib.pw_sgns_create_device(d_walks.device.index, C.c_void_p(d_walks.data_ptr()), d_walks.shape[0], d_walks.shape[1] - 2,
                                             num_nodes, dim, window, negative, epochs, float(alpha), float(min_alpha), float(sample),
                                             self.params["seed"], workers, _lib.PW_SGNS_LOSS if compute_loss else 0, C.byref(handle)))
        self._handle = handle

    # ---- life time
    def close(self):
        """Free the handle (both matrices, the tables).  Closing twice is harmless."""
        if self._handle is not None:
            _lib.load().pw_sgns_destroy(self._handle)
            self._handle = None
            self.d_walks = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass

    def _open(self):
        if self._handle is None:
            raise ValueError("the session is closed")
        return self._handle

    @property
    def corpus_shape(self):
        """``(n_walks, walk_length, num_nodes)``"""
        self._open()
        return int(self.d_walks.shape[0]), int(self.d_walks.shape[1]) - 2, self.num_nodes

    # ---- training
    def run(self, epochs=1):
        """Train the next ``epochs`` epochs of the schedule; one dict per epoch: ``loss`` (a float, 0.0 without
        ``compute_loss``), ``evaluations``, ``kept_occurrences``, ``trained_pairs``.  More epochs than the schedule has left
        is a ``ValueError`` and trains nothing (``reschedule`` starts a new schedule).  ``self.last_stats``: the run's
        ``pw_sgns_stats``."""
        handle = self._open()
        epochs = int(epochs)
        st = self.state
        if epochs < 1:
            raise ValueError("epochs must be positive")
        if st["sched_pos"] + epochs > st["sched_total"]:
            raise ValueError(f"the schedule has {st['sched_total'] - st['sched_pos']} of {st['sched_total']} epochs left, "
                             f"{epochs} asked for: reschedule() starts a new one")
        cells = (_lib.PwSgnsEpoch * epochs)()
        stats = _lib.PwSgnsStats()
        _lib.check(_lib.load().pw_sgns_run(handle, epochs, C.cast(cells, C.c_void_p), C.cast(C.pointer(stats), C.c_void_p)))
        self.last_stats = stats.as_dict()
        self.last_stats["lock_instances"] = bool(self._lock_info()[2])
        return [c.as_dict() for c in cells]

    # ---- frozen rows
    def _lock_info(self):
        """``pw_sgns_lock_info``: frozen rows of ``syn0``, of ``syn1``, and whether the last run launched the kernel's lock
        instances."""
        out = (C.c_uint64 * 3)()
        _lib.check(_lib.load().pw_sgns_lock_info(self._open(), out))
        return int(out[0]), int(out[1]), int(out[2])

    def _row_mask(self, rows, name):
        """``rows`` -- a bool mask of length ``num_nodes`` or an integer index array or tensor, on the host or on the
        session's device -- as a uint8 CUDA tensor ``[num_nodes]``; every complaint is a ``ValueError``."""
        import torch

        dev = self.d_walks.device
        if isinstance(rows, torch.Tensor):
            if rows.device.type not in ("cpu", "cuda") or (rows.is_cuda and rows.device != dev):
                raise ValueError(f"{name} must be on the host or on {dev}, not on {rows.device}")
        else:
            rows = np.asarray(rows)
            if rows.dtype == object or rows.dtype.kind not in "biu":
                raise ValueError(f"{name} must be a bool mask or integer indices, not {rows.dtype}")
            if rows.dtype.kind == "u":   # (torch has no wide unsigned integers)
                if rows.size and int(rows.max()) >= self.num_nodes:
                    raise ValueError(f"{name} holds an index outside 0..{self.num_nodes - 1}")
                rows = rows.astype(np.int64)
            rows = torch.from_numpy(np.ascontiguousarray(rows))
        if rows.dtype.is_floating_point or rows.dtype.is_complex:
            raise ValueError(f"{name} must be a bool mask or integer indices, not {rows.dtype}")
        if rows.dim() != 1:
            raise ValueError(f"{name} must have one dimension, not {rows.dim()}")
        if rows.dtype == torch.bool:
            if rows.numel() != self.num_nodes:
                raise ValueError(f"a mask must have num_nodes = {self.num_nodes} entries, {name} has {rows.numel()}")
            return rows.to(dev).to(torch.uint8).contiguous()
        rows = rows.to(dev).to(torch.int64)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= self.num_nodes):
            raise ValueError(f"{name} holds an index outside 0..{self.num_nodes - 1}")
        mask = torch.zeros(self.num_nodes, dtype=torch.uint8, device=dev)
        mask[rows] = 1
        return mask

    def freeze(self, rows, context=True):
        """Freeze rows (``pw_sgns_set_locks``): a frozen row is read by every pair that names it and never written, so it
        keeps its bits however long the session trains, while the other rows train on exactly the evaluations an unfrozen
        session performs -- pairs, negatives, loss and counters are unchanged, and a free context row still learns from a
        frozen target.  ``rows``: a bool mask of length ``num_nodes`` or an integer index array or tensor, on the host or on
        the session's device: the rows of ``syn0`` (``vectors()``).  ``context=True`` freezes the same rows of ``syn1``
        (``context_vectors()``), ``context=False`` leaves ``syn1`` free, a mask or index array freezes those rows of ``syn1``
        instead.  Replaces what was frozen before.  Locks survive ``run``, ``reschedule``, ``set_walks``, ``evaluate`` and
        ``load``; ``load`` still replaces a matrix wholesale, frozen rows included.  A mask of the wrong length, an index
        outside ``0..num_nodes-1``, a tensor on another GPU, a floating-point dtype and a closed session are ``ValueError``s
        that change nothing."""
        import torch

        handle = self._open()
        m0 = self._row_mask(rows, "rows")
        if context is True:
            m1 = m0
        elif context is False or context is None:
            m1 = None
        else:
            m1 = self._row_mask(context, "context")
        torch.cuda.current_stream(self.d_walks.device).synchronize()
        _lib.check(_lib.load().pw_sgns_set_locks(handle, C.c_void_p(m0.data_ptr()), C.c_void_p(m1.data_ptr()) if m1 is not None else None))

    def unfreeze(self):
        """No row of either matrix is frozen from here on: ``run`` launches the kernel without locks again."""
        _lib.check(_lib.load().pw_sgns_set_locks(self._open(), None, None))

    @property
    def frozen(self):
        """``(mask0, mask1)``: bool CUDA tensors ``[num_nodes]``, the frozen rows of ``syn0`` and of ``syn1``."""
        import torch

        handle = self._open()
        out = torch.empty((2, self.num_nodes), dtype=torch.uint8, device=self.d_walks.device)
        torch.cuda.current_stream(self.d_walks.device).synchronize()
        _lib.check(_lib.load().pw_sgns_get_locks(handle, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr())))
        return out[0].to(torch.bool), out[1].to(torch.bool)

    # ---- scoring without training, another corpus
    @staticmethod
    def _walks_checked(d_walks):
        """The constructor's tensor checks."""
        import torch

        if not isinstance(d_walks, torch.Tensor) or not d_walks.is_cuda or d_walks.dtype != torch.int32 or not d_walks.is_contiguous():
            raise ValueError("d_walks must be a contiguous int32 CUDA tensor")
        if d_walks.dim() != 2 or d_walks.shape[1] < 3:
            raise ValueError("walk matrix must be int32[n_walks, walk_length + 2]")
        return d_walks

    def _walks_on_my_device(self, d_walks):
        import torch

        self._walks_checked(d_walks)
        if d_walks.device != self.d_walks.device:
            raise ValueError(f"d_walks must be on {self.d_walks.device}, not on {d_walks.device}")
        torch.cuda.current_stream(d_walks.device).synchronize()  # the matrix was produced on torch's stream
        return d_walks

    def evaluate(self, d_walks=None, epoch=None):
        """The loss of the vectors as they are on a walk matrix, nothing trained (``pw_sgns_evaluate``: a read-only kernel of
        its own): the record ``run`` reports for an epoch -- ``loss``, ``evaluations``, ``kept_occurrences``,
        ``trained_pairs`` (the pairs scored) -- of the evaluations that epoch ``epoch`` of a training run on that matrix
        performs, against ``syn0`` / ``syn1`` unchanged.  ``d_walks=None``: the session's own matrix; any other matrix (the
        constructor's tensor checks, the session's device) may have its own shape -- held-out walks.  ``epoch=None``:
        ``state["epoch"]``, the epoch ``run`` would train next.  Works without ``compute_loss``.  Vectors, tables and state
        are untouched, and the record is a function of (seed, epoch, matrix, vectors) bit for bit, whatever ``workers`` is."""
        handle = self._open()
        if d_walks is not None:
            self._walks_on_my_device(d_walks)
        if epoch is not None and int(epoch) < 0:
            raise ValueError("epoch must not be negative")
        epoch = self.state["epoch"] if epoch is None else int(epoch)
        cell = _lib.PwSgnsEpoch()
        if d_walks is None:
            rc = _lib.load().pw_sgns_evaluate(handle, None, 0, 0, epoch, C.byref(cell))
        else:
            rc = _lib.load().pw_sgns_evaluate(handle, C.c_void_p(d_walks.data_ptr()), d_walks.shape[0], d_walks.shape[1] - 2, epoch,
                                              C.byref(cell))
        _lib.check(rc)
        return cell.as_dict()

    def set_walks(self, d_walks, recount=False):
        """Train on another matrix from here on (``pw_sgns_set_walks``): ``d_walks`` passes the constructor's tensor checks,
        is on the session's device and has the session's shape -- the schedule arithmetic stays; another shape is a
        ``ValueError``.  ``recount=False``: the noise table and the keep probabilities stay those of the constructor's
        matrix; ``recount=True``: they are rebuilt from the new one.  Vectors and state are untouched.  The session holds
        a reference to the new matrix once the library has accepted it; on any error it keeps the old one."""
        handle = self._open()
        self._walks_on_my_device(d_walks)
        if tuple(d_walks.shape) != tuple(self.d_walks.shape):
            raise ValueError(f"the session was created on a matrix of shape {list(self.d_walks.shape)}, d_walks has the shape "
                             f"{list(d_walks.shape)}: another shape needs a session of its own")
        _lib.check(_lib.load().pw_sgns_set_walks(handle, C.c_void_p(d_walks.data_ptr()), d_walks.shape[0], d_walks.shape[1] - 2,
                                                 _lib.PW_SGNS_RECOUNT if recount else 0))
        self.d_walks = d_walks

    @property
    def state(self):
        """``epoch`` (the global epoch index the hashes use; it only grows), ``sched_pos`` / ``sched_total`` (epochs of the
        schedule done / in all), ``alpha``, ``min_alpha``."""
        st = _lib.PwSgnsState()
        _lib.check(_lib.load().pw_sgns_get_state(self._open(), C.byref(st)))
        return st.as_dict()

    def _set_state(self, **fields):
        st = _lib.PwSgnsState(**fields)
        _lib.check(_lib.load().pw_sgns_set_state(self._open(), C.byref(st)))

    def reschedule(self, epochs, alpha=None, min_alpha=None):
        """A new learning-rate schedule of ``epochs`` epochs on the vectors as they are (gensim's ``train()`` on a trained
        model): ``alpha`` / ``min_alpha`` default to the current ones.  The epoch index of the hashes goes on counting."""
        st = self.state
        epochs = int(epochs)
        if epochs < 1:
            raise ValueError("epochs must be positive")
        alpha = st["alpha"] if alpha is None else float(alpha)
        min_alpha = st["min_alpha"] if min_alpha is None else float(min_alpha)
        if not (np.isfinite(alpha) and np.isfinite(min_alpha)):
            raise ValueError("alpha and min_alpha must be finite")
        self._set_state(epoch=st["epoch"], sched_pos=0, sched_total=epochs, alpha=alpha, min_alpha=min_alpha)

    # ---- the matrices
    def _matrix(self, which):
        import torch

        handle = self._open()
        out = torch.empty((self.num_nodes, self.params["dim"]), dtype=torch.float32, device=self.d_walks.device)
        _lib.check(_lib.load().pw_sgns_vectors_get(handle, which, C.c_void_p(out.data_ptr())))
        return out

    def vectors(self):
        """A new ``float32[num_nodes, dim]`` CUDA tensor: the input vectors (``syn0``, gensim's ``wv``)."""
        return self._matrix(0)

    def context_vectors(self):
        """A new ``float32[num_nodes, dim]`` CUDA tensor: the context vectors (``syn1``, gensim's ``syn1neg``)."""
        return self._matrix(1)

    def load(self, vectors=None, context_vectors=None):
        """Replace ``syn0`` and / or ``syn1``: a CUDA tensor on the session's device, a CPU tensor or a NumPy array, each
        ``float32[num_nodes, dim]`` -- another shape, dtype or device is a ``ValueError`` and changes nothing."""
        import torch

        handle = self._open()
        shape = (self.num_nodes, self.params["dim"])
        staged = []
        for which, name, m in ((0, "vectors", vectors), (1, "context_vectors", context_vectors)):
            if m is None:
                continue
            if isinstance(m, torch.Tensor):
                if m.device.type not in ("cpu", "cuda") or (m.is_cuda and m.device != self.d_walks.device):
                    raise ValueError(f"{name} must be on the host or on {self.d_walks.device}, not on {m.device}")
                if m.dtype != torch.float32:
                    raise ValueError(f"{name} must be float32, not {m.dtype}")
            else:
                m = np.asarray(m)
                if m.dtype != np.float32:
                    raise ValueError(f"{name} must be float32, not {m.dtype}")
                m = torch.from_numpy(np.ascontiguousarray(m))
            if tuple(m.shape) != shape:
                raise ValueError(f"{name} must be float32{list(shape)}, not {list(m.shape)}")
            staged.append((which, m.to(self.d_walks.device).contiguous()))
        torch.cuda.current_stream(self.d_walks.device).synchronize()
        for which, m in staged:
            _lib.check(_lib.load().pw_sgns_vectors_set(handle, which, C.c_void_p(m.data_ptr())))

    # ---- nearest neighbours
    def knn_index(self, against="vectors"):
        """A ``KnnIndex`` on a snapshot of ``vectors()`` (``against="vectors"``) or of ``context_vectors()``
        (``against="context"``) as they are now: training on does not change it.  For callers who query more than once."""
        if against not in ("vectors", "context"):
            raise ValueError(f"against must be 'vectors' or 'context', not {against!r}")
        return KnnIndex(self.vectors() if against == "vectors" else self.context_vectors())

    def most_similar(self, rows, topn=10, metric="cosine", against="vectors"):
        """``(idx, score)`` tensors of the ``topn`` nearest rows to each of ``rows`` among the current ``vectors()`` (the row
        itself left out) or, with ``against="context"``, among ``context_vectors()`` (nothing left out).  The query vectors
        always come from ``vectors()``: ``metric="dot"`` with ``against="context"`` is the model's own score of a (centre,
        context) pair, the link score SGNS trains.  The definition is ``KnnIndex``'s."""
        with self.knn_index(against) as index:
            if against == "vectors":
                return index.query(rows=rows, topn=topn, metric=metric)
            import torch

            n = self.num_nodes
            r = _knn_rows(rows, n)
            return index.query(vectors=self.vectors()[torch.from_numpy(r.astype(np.int64)).to(self.d_walks.device)].contiguous(), topn=topn,
                               metric=metric)

    def score_pairs(self, u, v, metric="dot", against="context"):
        """A float64 ``[m]`` CUDA tensor: the score of ``vectors()[u[i]]`` against ``context_vectors()[v[i]]``
        (``against="context"``: with ``metric="dot"`` the model's own link score, what ``most_similar`` ranks by) or against
        ``vectors()[v[i]]`` (``against="vectors"``), as they are now.  The definition is ``KnnIndex.score_pairs``'s."""
        if against not in ("vectors", "context"):
            raise ValueError(f"against must be 'vectors' or 'context', not {against!r}")
        with self.knn_index("vectors") as a:
            if against == "vectors":
                return a.score_pairs(u, v, metric=metric)
            with self.knn_index("context") as b:
                return a.score_pairs(u, v, metric=metric, other=b)

    def fit_pairs(self, u, v, y, op, l2=1e-3, against="context", max_iter=200, gtol=1e-8):
        """``KnnIndex.fit_pairs`` on ``vectors()[u[i]]`` and ``context_vectors()[v[i]]`` (``against="context"``) or
        ``vectors()[v[i]]`` (``against="vectors"``), as they are now."""
        if against not in ("vectors", "context"):
            raise ValueError(f"against must be 'vectors' or 'context', not {against!r}")
        with self.knn_index("vectors") as a:
            if against == "vectors":
                return a.fit_pairs(u, v, y, op, l2=l2, max_iter=max_iter, gtol=gtol)
            with self.knn_index("context") as b:
                return a.fit_pairs(u, v, y, op, l2=l2, other=b, max_iter=max_iter, gtol=gtol)

    # ---- checkpoints
    def save(self, path):
        """An ``.npz`` with both matrices, the state, the constructor's parameters and ``(n_walks, walk_length,
        num_nodes)``: what ``restore`` needs besides the walk matrix.  With frozen rows also ``frozen_vectors`` and
        ``frozen_context`` (bool arrays), which ``restore`` applies; without, the file has no such keys."""
        st = self.state
        arrays = dict(vectors=self.vectors().cpu().numpy(), context_vectors=self.context_vectors().cpu().numpy(),
                      corpus_shape=np.array(self.corpus_shape, dtype=np.int64))
        arrays.update({"state_" + k: np.array(v) for k, v in st.items()})
        arrays.update({"param_" + k: np.array(v) for k, v in self.params.items()})
        n0, n1, _ = self._lock_info()
        if n0 or n1:   # (a session without frozen rows writes the file it always wrote)
            m0, m1 = self.frozen
            arrays.update(frozen_vectors=m0.cpu().numpy(), frozen_context=m1.cpu().numpy())
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def restore(cls, path, d_walks):
        """The session ``save`` wrote, on the same corpus: ``d_walks`` must have the saved ``(n_walks, walk_length)`` --
        another shape is a ``ValueError`` before any device work.  (The matrix itself is not in the file.)"""
        with np.load(path) as z:
            saved = {k: z[k] for k in z.files}
        n_walks, walk_length, num_nodes = (int(x) for x in saved["corpus_shape"])
        shape = tuple(getattr(d_walks, "shape", ()))
        if len(shape) != 2 or (int(shape[0]), int(shape[1]) - 2) != (n_walks, walk_length):
            raise ValueError(f"{path} was saved on a corpus of {n_walks} walks of length {walk_length}; "
                             f"d_walks has the shape {list(shape)}")
        params = {k[len("param_"):]: v.item() for k, v in saved.items() if k.startswith("param_")}
        s = cls(d_walks, num_nodes, **params)
        try:
            s.load(vectors=saved["vectors"], context_vectors=saved["context_vectors"])
            s._set_state(epoch=int(saved["state_epoch"]), sched_pos=int(saved["state_sched_pos"]),
                         sched_total=int(saved["state_sched_total"]), alpha=float(saved["state_alpha"]),
                         min_alpha=float(saved["state_min_alpha"]))
            if "frozen_vectors" in saved:
                s.freeze(saved["frozen_vectors"].astype(bool), context=saved["frozen_context"].astype(bool))
        except Exception:
            s.close()
            raise
        return s


_WRITE_ROWS = 1 << 14   # rows formatted per write


def save_word2vec_format(path, node_ids, vectors):
    """The text format gensim's ``KeyedVectors.save_word2vec_format`` writes (cli.py:323-325): a header line
    ``count dim``, then per node its name and the components as ``%.6f``, separated by single spaces.  Rows are
    formatted a block at a time (one ``%`` application and one write per block of rows, not one per component)."""
    vectors = np.asarray(vectors)
    dim = vectors.shape[1]
    row_fmt = "%s" + " %.6f" * dim + "\n"
    with open(path, "w", encoding="utf-8", newline="\n") as f:
        f.write(f"{len(node_ids)} {dim}\n")
        n = min(len(node_ids), vectors.shape[0])
        for lo in range(0, n, _WRITE_ROWS):
            hi = min(n, lo + _WRITE_ROWS)
            block = vectors[lo:hi].astype(np.float64).tolist()   # Python floats: what the f-string of a float32 formats
            fmt = row_fmt * (hi - lo)
            flat = []
            for name, row in zip(node_ids[lo:hi], block):
                flat.append(str(name))
                flat.extend(row)
            f.write(fmt % tuple(flat))


def save_word2vec_format_device(path, node_ids, d_vectors):
    """``save_word2vec_format`` for vectors in device memory: ``d_vectors`` is a contiguous float32 CUDA tensor ``[n, dim]``
    (what ``train_sgns_device`` returns), ``node_ids`` its ``n`` names (``str(name)`` encoded as UTF-8).  The text is made on
    the GPU (``pw_vectors_write_text_device``) and written by the library in chunks; the file equals
    ``save_word2vec_format(path, node_ids, d_vectors.cpu().numpy())`` byte for byte.  What the call did
    (``pw_emb_write_stats``: ``format_ms``, ``copy_ms``, ``write_ms``, ``bytes``, ``chunks``) is left in
    ``save_word2vec_format_device.last_stats``."""
    import os

    import torch

    if not isinstance(d_vectors, torch.Tensor) or not d_vectors.is_cuda:
        raise ValueError("d_vectors must be a CUDA tensor (a contiguous float32[n, dim] in device memory)")
    if d_vectors.dtype != torch.float32:
        raise ValueError(f"d_vectors must be float32, not {d_vectors.dtype}")
    if not d_vectors.is_contiguous():
        raise ValueError("d_vectors must be contiguous (row-major, dense)")
    if d_vectors.dim() != 2 or d_vectors.shape[0] < 1 or d_vectors.shape[1] < 1:
        raise ValueError("d_vectors must be float32[n, dim] with n >= 1 and dim >= 1")
    n, dim = int(d_vectors.shape[0]), int(d_vectors.shape[1])
    if len(node_ids) != n:
        raise ValueError(f"{len(node_ids)} node names for {n} rows")
    names = [str(name).encode("utf-8") for name in node_ids]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=n), out=offsets[1:])
    blob = b"".join(names)
    lib = _lib.load()
    torch.cuda.current_stream(d_vectors.device).synchronize()  # the vectors were produced on torch's stream
    st = _lib.PwEmbWriteStats()
    _lib.check(lib.pw_vectors_write_text_device(d_vectors.device.index, C.c_void_p(d_vectors.data_ptr()), n, dim, blob,
                                                C.c_void_p(offsets.ctypes.data), os.fsencode(path), C.byref(st)))
    save_word2vec_format_device.last_stats = st.as_dict()


save_word2vec_format_device.last_stats = None


# ---- nearest neighbours of embedding vectors, exact and ordered (csrc/knn.hip.h) ----------------------------------------------
def _check_value(rc):
    """``_lib.check`` with PW_ERR_INVALID as a ``ValueError``."""
    if rc == _lib.ERR_INVALID:
        msg = _lib.load().pw_last_error()
        raise ValueError(msg.decode() if msg else "invalid argument")
    _lib.check(rc)


def _knn_args(queries, rows, topn, metric, exclude_self):
    """The checks every form of the query shares: ``(topn, metric id, exclude_self)``."""
    if (queries is None) == (rows is None):
        raise ValueError("exactly one of vectors (queries) and rows must be given")
    topn = int(topn)
    if not 1 <= topn <= _lib.PW_KNN_MAX_TOPN:
        raise ValueError(f"topn = {topn} outside 1..{_lib.PW_KNN_MAX_TOPN}")
    if metric not in _lib.KNN_METRICS:
        raise ValueError(f"metric must be 'cosine' or 'dot', not {metric!r}")
    if exclude_self is None:
        exclude_self = rows is not None
    return topn, _lib.KNN_METRICS[metric], bool(exclude_self)


def _knn_rows(rows, n):
    """Row numbers -- a list, an array or a tensor of integers -- as a uint32 array; one outside ``0..n-1`` is a ``ValueError``."""
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    rows = np.asarray(rows)
    if rows.dtype == object or rows.dtype.kind not in "iu" or rows.ndim != 1:
        raise ValueError("rows must be a one-dimensional array of integers")
    if rows.size:
        lo, hi = int(rows.min()), int(rows.max())
        if lo < 0 or hi >= n:
            raise ValueError(f"row number {lo if lo < 0 else hi} is outside the {n} rows")
    return np.ascontiguousarray(rows, dtype=np.uint32)


def knn_host(vectors, queries=None, rows=None, topn=10, metric="cosine", exclude_self=None):
    """The NumPy statement of the nearest-neighbour definition (csrc/knn.hip.h), what ``KnnIndex`` is held to bit
    for bit: ``(idx int64[nq, topn], score float64[nq, topn])``, padded with -1 / -inf beyond the number of candidates.

    ``dot`` sums the float64 products of the float32 values with k ascending from +0.0; ``norm = sqrt(dot(x, x))``;
    ``cosine = dot(q, x) / (norm(q) * norm(x))``, +0.0 where that product is 0; rows rank by descending score, ties by
    ascending row number; with ``exclude_self`` (the default for ``rows``) a query given as a row number leaves that row out."""
    X = np.asarray(vectors)
    if X.dtype != np.float32 or X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("vectors must be float32[n, dim]")
    topn, metric_id, exclude_self = _knn_args(queries, rows, topn, metric, exclude_self)
    n, dim = X.shape
    if rows is not None:
        rows = _knn_rows(rows, n)
        Q = X[rows]
    else:
        Q = np.asarray(queries)
        if Q.dtype != np.float32 or Q.ndim != 2 or Q.shape[1] != dim:
            raise ValueError(f"queries must be float32[nq, {dim}]")
    nq = Q.shape[0]

    def dots(A, B):   # [len(A), len(B)]: k ascending, one rounding per addition
        acc = np.zeros((A.shape[0], B.shape[0]))
        tmp = np.empty_like(acc)
        A64, B64 = A.astype(np.float64), np.ascontiguousarray(B.astype(np.float64).T)
        for k in range(dim):
            np.multiply(A64[:, k, None], B64[k][None, :], out=tmp)
            acc += tmp
        return acc

    def self_dots(A):
        acc = np.zeros(A.shape[0])
        A64 = A.astype(np.float64)
        for k in range(dim):
            acc += A64[:, k] * A64[:, k]
        return acc

    with np.errstate(all="ignore"):
        xx, qq = self_dots(X), self_dots(Q)
        for what, d in (("row", xx), ("query", qq)):
            bad = np.flatnonzero(~np.isfinite(d))
            if bad.size and (what == "row" or rows is None):
                raise ValueError(f"{what} {int(bad[0])} holds a NaN or an infinity")
        xn, qn = np.sqrt(xx), np.sqrt(qq)
        idx = np.full((nq, topn), -1, dtype=np.int64)
        score = np.full((nq, topn), -np.inf)
        block = 4096   # rows at a time: the running sums stay in cache
        for q in range(0, nq, 64):
            qs = slice(q, min(nq, q + 64))
            s = np.concatenate([dots(Q[qs], X[b:b + block]) for b in range(0, n, block)], axis=1)
            if metric_id == _lib.KNN_METRICS["cosine"]:
                den = qn[qs, None] * xn[None, :]
                s = np.where(den == 0.0, 0.0, s / np.where(den == 0.0, 1.0, den))
            for i in range(s.shape[0]):
                si = s[i]
                cand = np.arange(n)
                if exclude_self and rows is not None:
                    cand = cand[cand != rows[q + i]]
                if cand.size > topn:   # only what reaches the topn-th score can rank (ties included)
                    cand = cand[si[cand] >= np.partition(si[cand], cand.size - topn)[cand.size - topn]]
                order = cand[np.lexsort((cand, -si[cand]))][:topn]
                idx[q + i, :order.size] = order
                score[q + i, :order.size] = si[order]
    return idx, score


class KnnIndex:
    """Nearest neighbours of embedding vectors on the GPU, exact and ordered (``pw_knn``, csrc/knn.hip.h): what gensim's
    ``wv.most_similar`` answers, by the definition ``knn_host`` states in NumPy, bit for bit.

    ``vectors``: a CUDA tensor, a CPU tensor or a NumPy array, float32 ``[n, dim]`` and contiguous (``1 <= dim <= 4096``);
    anything else is a ``ValueError`` before any device work.  The index COPIES the matrix: a snapshot.  A NaN or an infinity
    in it is a ``ValueError`` that names the first such row.  ``node_ids``: the ``n`` names ``most_similar`` speaks in.
    A context manager; after ``close`` every use is a ``ValueError``."""

    def __init__(self, vectors, node_ids=None, device=None):
        self._handle = None
        self.last_stats = None
        kind = "numpy"
        if hasattr(vectors, "is_cuda"):   # a torch tensor
            import torch

            kind = "cuda" if vectors.is_cuda else "cpu"
            if vectors.device.type not in ("cpu", "cuda"):
                raise ValueError(f"vectors must be on the host or on a GPU, not on {vectors.device}")
            if vectors.dtype != torch.float32:
                raise ValueError(f"vectors must be float32, not {vectors.dtype}")
            shape, contiguous = tuple(vectors.shape), vectors.is_contiguous()
        elif isinstance(vectors, np.ndarray):
            if vectors.dtype != np.float32:
                raise ValueError(f"vectors must be float32, not {vectors.dtype}")
            shape, contiguous = vectors.shape, vectors.flags["C_CONTIGUOUS"]
        else:
            raise ValueError(f"vectors must be a torch tensor or a NumPy array, got {type(vectors).__name__}")
        if len(shape) != 2 or shape[0] < 1 or not 1 <= shape[1] <= 4096:
            raise ValueError(f"vectors must be float32[n, dim] with n >= 1 and 1 <= dim <= 4096, not {list(shape)}")
        if not contiguous:
            raise ValueError("vectors must be contiguous (row-major, dense)")
        if shape[0] >= 2 ** 32:
            raise ValueError("vectors must have fewer than 2^32 rows")
        if node_ids is not None and len(node_ids) != shape[0]:
            raise ValueError(f"{len(node_ids)} node names for {shape[0]} rows")
        self.n, self.dim = int(shape[0]), int(shape[1])
        self.node_ids = list(node_ids) if node_ids is not None else None
        self._row_of = {name: i for i, name in enumerate(self.node_ids)} if node_ids is not None else None
        self.device = vectors.device.index if kind == "cuda" else int(device or 0)

        lib = _lib.load()
        handle = C.c_void_p()
        if kind == "cuda":
            import torch

            torch.cuda.current_stream(vectors.device).synchronize()   # the vectors were produced on torch's stream
            rc = lib.pw_knn_create_device(self.device, C.c_void_p(vectors.data_ptr()), self.n, self.dim, C.byref(handle))
        else:
            host = vectors.numpy() if kind == "cpu" else vectors
            rc = lib.pw_knn_create(self.device, C.c_void_p(host.ctypes.data), self.n, self.dim, C.byref(handle))
        _check_value(rc)
        self._handle = handle

    def close(self):
        """Free the index.  Closing twice is harmless."""
        if self._handle is not None:
            _lib.load().pw_knn_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass

    def _open(self):
        if self._handle is None:
            raise ValueError("the index is closed")
        return self._handle

    def _torch_device(self):
        import torch

        return torch.device("cuda", self.device)

    def norms(self):
        """A new float64 ``[n]`` CUDA tensor: ``sqrt(dot(x, x))`` of every row, by the definition."""
        import torch

        handle = self._open()
        out = torch.empty(self.n, dtype=torch.float64, device=self._torch_device())
        _check_value(_lib.load().pw_knn_norms_get(handle, C.c_void_p(out.data_ptr())))
        return out

    def query(self, vectors=None, rows=None, topn=10, metric="cosine", exclude_self=None):
        """``(idx, score)`` CUDA tensors, int64 ``[nq, topn]`` padded with -1 and float64 padded with -inf: the ``topn``
        nearest rows to each query, given as ``vectors`` (float32 ``[nq, dim]``: a CUDA tensor on the index's device, a CPU
        tensor or a NumPy array) or as ``rows`` (row numbers).  ``exclude_self`` defaults to True for ``rows`` -- that one
        row is left out -- and means nothing for ``vectors``.  ``self.last_stats``: ``pw_knn_stats``."""
        import torch

        handle = self._open()
        topn, metric_id, exclude_self = _knn_args(vectors, rows, topn, metric, exclude_self)
        dev = self._torch_device()
        d_q = d_r = None
        if rows is not None:
            d_r = torch.from_numpy(_knn_rows(rows, self.n).view(np.int32)).to(dev)
            nq = d_r.numel()
        else:
            q = vectors
            if isinstance(q, np.ndarray):
                if q.dtype != np.float32:
                    raise ValueError(f"query vectors must be float32, not {q.dtype}")
                q = torch.from_numpy(np.ascontiguousarray(q))
            elif not isinstance(q, torch.Tensor):
                raise ValueError(f"query vectors must be a torch tensor or a NumPy array, got {type(q).__name__}")
            if q.dtype != torch.float32:
                raise ValueError(f"query vectors must be float32, not {q.dtype}")
            if q.dim() != 2 or q.shape[1] != self.dim:
                raise ValueError(f"query vectors must be float32[nq, {self.dim}], not {list(q.shape)}")
            if q.is_cuda and q.device != dev:
                raise ValueError(f"query vectors must be on the host or on {dev}, not on {q.device}")
            d_q = q.to(dev).contiguous()
            nq = d_q.shape[0]
        idx = torch.empty((nq, topn), dtype=torch.int32, device=dev)
        score = torch.empty((nq, topn), dtype=torch.float64, device=dev)
        st = _lib.PwKnnStats()
        torch.cuda.current_stream(dev).synchronize()   # the queries were produced on torch's stream
        _check_value(_lib.load().pw_knn_query_device(handle, C.c_void_p(d_q.data_ptr()) if d_q is not None else None,
                                                     C.c_void_p(d_r.data_ptr()) if d_r is not None else None, nq, topn, metric_id,
                                                     int(exclude_self), C.c_void_p(idx.data_ptr()), C.c_void_p(score.data_ptr()), C.byref(st)))
        self.last_stats = st.as_dict()
        return idx.to(torch.int64), score   # (0xFFFFFFFF, the padding, is -1 as an int32)

    def score_pairs(self, u, v, metric="cosine", other=None):
        """A float64 ``[m]`` CUDA tensor: the score of row ``u[i]`` against row ``v[i]`` -- of ``other``, another ``KnnIndex``
        of the same ``dim`` on the same device, when one is given -- by the definition of ``query`` (``linkpred.score_pairs``;
        ``linkpred.score_pairs_host`` states it in NumPy).  ``u`` / ``v``: row numbers, torch or NumPy integer arrays, on the
        GPU or not."""
        from . import linkpred

        return linkpred.score_pairs(self, u, v, metric=metric, other=other)

    def fit_pairs(self, u, v, y, op, l2=1e-3, other=None, max_iter=200, gtol=1e-8):
        """A ``classify.LogisticModel``: the exact logistic regression of the labels ``y`` (0 / 1) on ``op`` (``average``,
        ``hadamard``, ``l1``, ``l2``; ``row``: the rows ``u`` themselves) of the rows ``u[i]`` and ``v[i]`` (``classify.fit``)."""
        from . import classify

        return classify.fit(self, u, v, y, op, l2=l2, other=other, max_iter=max_iter, gtol=gtol)

    def _row(self, node):
        if self._row_of is None:
            return int(node)
        if node in self._row_of:
            return self._row_of[node]
        if str(node) in self._row_of:
            return self._row_of[str(node)]
        raise ValueError(f"unknown node ID {node!r}")

    def most_similar(self, node, topn=10, metric="cosine"):
        """gensim's shape: ``[(id, score), ...]`` in rank order for one ``node`` -- an ID of ``node_ids``, or a row number when
        there are none -- with the padding trimmed; a list of such lists for a list of nodes.  The node itself is left out."""
        many = isinstance(node, (list, tuple, np.ndarray))
        rows = [self._row(x) for x in (node if many else [node])]
        idx, score = self.query(rows=np.asarray(rows, dtype=np.int64), topn=topn, metric=metric)
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        name = (lambda i: self.node_ids[i]) if self.node_ids is not None else int
        out = [[(name(int(i)), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]
        return out if many else out[0]
