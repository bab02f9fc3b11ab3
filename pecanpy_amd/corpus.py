"""The walk corpus as a text file: one walk per line, the names of its nodes separated by single spaces -- what gensim's
``LineSentence`` / ``Word2Vec(corpus_file=...)``, fastText and word2vec.c read, and what ``pecanpy --task walks`` and
``Base.walks_to_file`` write.

``save_walks`` is the host writer and the byte definition of the format: for a walk matrix ``uint32[n, L + 2]`` it writes what
``cli._dump_walks`` writes for the ID lists of the same rows (``Base._map_walk``).  ``save_walks_device`` makes the same bytes on
the GPU from the matrix where ``WalkEngine.simulate_device`` leaves it (``pw_walks_write_text_device``, csrc/walk_text.hip.h):
neither the matrix nor ID lists visit the host, only the text does.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

__all__ = ["save_walks", "save_walks_device"]

_WRITE_ROWS = 1 << 14   # rows formatted per write


def save_walks(path, node_ids, walk_matrix):
    """Row ``r`` with ``n = r[-1]`` gives the line ``" ".join(str(node_ids[i]) for i in r[:n]) + "\\n"`` (``n == 0``: the empty
    line), UTF-8, no header.  Cells at positions ``>= n`` are not looked at.  Rows are formatted a block at a time: one
    gather of the names and one write per block of rows, no list of lists for the whole matrix."""
    mat = np.asarray(walk_matrix)
    if mat.ndim != 2 or mat.shape[1] < 2 or mat.dtype.kind not in "ui":
        raise ValueError("walk matrix must be uint32[n_walks, walk_length + 2]")
    names = np.empty(len(node_ids), dtype=object)
    names[:] = [str(name) for name in node_ids]
    last = mat.shape[1] - 1
    cols = np.arange(last)
    with open(path, "w", encoding="utf-8", newline="\n") as f:
        for lo in range(0, mat.shape[0], _WRITE_ROWS):
            block = mat[lo:lo + _WRITE_ROWS]
            lens = block[:, last].astype(np.int64)
            bad = np.flatnonzero((lens < 0) | (lens > last))
            if bad.size:
                raise ValueError(f"row length {lens[bad[0]]} in row {lo + bad[0]} exceeds walk_length + 1 = {last}")
            tokens = block[:, :last][cols < lens[:, None]].astype(np.int64)   # the cells in front of each row's length, row by row
            bad = tokens[(tokens < 0) | (tokens >= names.size)]
            if bad.size:
                raise ValueError(f"node index {bad[0]} in rows {lo}.. outside the {names.size} names")
            words = names[tokens].tolist()
            lines, begin = [], 0
            for end in np.cumsum(lens).tolist():
                lines.append(" ".join(words[begin:end]))
                begin = end
            if lines:
                f.write("\n".join(lines) + "\n")


def save_walks_device(path, node_ids, d_walks):
    """``save_walks`` for a walk matrix in device memory: ``d_walks`` is what ``WalkEngine.simulate_device`` returns, a
    contiguous int32 CUDA tensor ``[n_walks, walk_length + 2]`` (uint32 storage); ``node_ids`` the names the node indices
    address (``str(name)`` encoded as UTF-8).  The text is made on the GPU (``pw_walks_write_text_device``) and written by the
    library in chunks; the file equals ``save_walks(path, node_ids, d_walks.cpu().numpy().view(np.uint32))`` byte for byte.  A
    row length above ``walk_length + 1`` or a node index without a name is a ``PwError``; the matrix is only read.  What the
    call did (``pw_walks_write_stats``: ``format_ms``, ``copy_ms``, ``write_ms``, ``bytes``, ``chunks``, ``rows``, ``tokens``)
    is left in ``save_walks_device.last_stats``."""
    import torch

    if not isinstance(d_walks, torch.Tensor) or not d_walks.is_cuda or d_walks.dtype != torch.int32 or not d_walks.is_contiguous():
        raise ValueError("d_walks must be a contiguous int32 CUDA tensor")
    if d_walks.dim() != 2 or d_walks.shape[1] < 2:   # (walk_length 0 is a corpus of start nodes: save_walks takes it too)
        raise ValueError("walk matrix must be int32[n_walks, walk_length + 2]")
    names = [str(name).encode("utf-8") for name in node_ids]
    n = len(names)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=n), out=offsets[1:])
    blob = b"".join(names)
    lib = _lib.load()
    torch.cuda.current_stream(d_walks.device).synchronize()  # the matrix was produced on torch's stream
    st = _lib.PwWalksWriteStats()
    _lib.check(lib.pw_walks_write_text_device(d_walks.device.index, C.c_void_p(d_walks.data_ptr()), d_walks.shape[0],
                                              d_walks.shape[1] - 2, blob, C.c_void_p(offsets.ctypes.data), n, os.fsencode(path),
                                              C.byref(st)))
    save_walks_device.last_stats = st.as_dict()


save_walks_device.last_stats = None
