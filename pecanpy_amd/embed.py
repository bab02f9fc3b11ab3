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
"""
import ctypes as C

import numpy as np

from . import _lib

__all__ = ["train_sgns", "train_sgns_device", "train_sgns_file", "save_word2vec_format", "save_word2vec_format_device",
           "SgnsSession", "sgns_session_file"]


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
