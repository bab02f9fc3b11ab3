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
"""
import ctypes as C

import numpy as np

from . import _lib

__all__ = ["train_sgns", "train_sgns_device", "train_sgns_file", "save_word2vec_format", "save_word2vec_format_device"]


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
    d_vectors = train_sgns_device(d_walks, len(names), dim=dim, window=window, epochs=epochs, negative=negative, alpha=alpha,
                                  min_alpha=min_alpha, sample=sample, seed=seed, workers=workers)
    train_sgns_file.last_stats = {"read": read_walks_device.last_stats, "train": train_sgns_device.last_stats}
    return names, d_vectors


train_sgns_file.last_stats = None


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
