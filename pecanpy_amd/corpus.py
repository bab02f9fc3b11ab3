"""The walk corpus as a text file: one walk per line, the names of its nodes separated by single spaces -- what gensim's
``LineSentence`` / ``Word2Vec(corpus_file=...)``, fastText and word2vec.c read, and what ``pecanpy --task walks`` and
``Base.walks_to_file`` write.

``save_walks`` is the host writer and the byte definition of the format: for a walk matrix ``uint32[n, L + 2]`` it writes what
``cli._dump_walks`` writes for the ID lists of the same rows (``Base._map_walk``).  ``save_walks_device`` makes the same bytes on
the GPU from the matrix where ``WalkEngine.simulate_device`` leaves it (``pw_walks_write_text_device``, csrc/walk_text.hip.h):
neither the matrix nor ID lists visit the host, only the text does.

``read_walks`` is the host reader and the byte definition of the way back: a corpus file -> the walk matrix and the names.
``read_walks_device`` makes the same matrix on the GPU from the text (``pw_corpus_read_device``, csrc/corpus_dev.hip.h), where
``embed.train_sgns_device`` takes it: only the file's bytes go up and only the names come down.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

__all__ = ["save_walks", "save_walks_device", "read_walks", "read_walks_device"]

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


def _unknown_token(token, line, n_names):
    return ValueError(f"token {token!r} in line {line} of the corpus is not among the {n_names} node ids")


def read_walks(path, node_ids=None):
    """The inverse of ``save_walks`` and the byte definition of what ``read_walks_device`` returns: ``(walk_matrix, names)``.

    The file's bytes are split on ``b"\\n"``; an empty last piece is dropped (a file that ends in a newline; the empty file).
    Every other piece is a line, an empty one included, and ``line.decode("utf-8").split()`` gives its tokens -- a ``\\r`` is
    white space wherever it stands, as it is for gensim's ``LineSentence``.  ``names`` holds the distinct tokens in order of
    first appearance and a token's index is its position there; with ``node_ids`` given the indices address ``node_ids``
    (``str(name)``) instead, ``names`` is ``[str(x) for x in node_ids]`` and a token that is not among them is a
    ``ValueError`` that names the token and its line (counted from 1).  ``walk_matrix`` is ``uint32[n_lines, W]`` with
    ``W = max(most tokens in any line, 1) + 1``: a row with ``n`` tokens holds their indices in cells ``[0, n)``, 0 in cells
    ``[n, W - 1)`` and ``n`` in cell ``W - 1`` -- the engine's row form with ``walk_length = W - 2``.  A file without lines
    gives ``uint32[0, 2]`` and ``[]``."""
    from array import array

    with open(path, "rb") as f:
        pieces = f.read().split(b"\n")
    if pieces[-1] == b"":
        pieces.pop()
    if node_ids is None:
        names, index = [], {}
    else:
        names, index = [str(x) for x in node_ids], {}
        for i, name in enumerate(names):
            index.setdefault(name, i)
    flat = array("I")   # the indices of all tokens in file order: four bytes a token, not a Python object
    lens = np.zeros(len(pieces), dtype=np.int64)
    for r, piece in enumerate(pieces):
        tokens = piece.decode("utf-8").split()
        lens[r] = len(tokens)
        if node_ids is None:
            flat.extend([index.setdefault(t, len(index)) for t in tokens])
        else:
            try:
                flat.extend([index[t] for t in tokens])
            except KeyError as e:
                raise _unknown_token(e.args[0], r + 1, len(names)) from None
    if node_ids is None:
        names = list(index)   # (a dict keeps insertion order: first appearance)
    last = max(int(lens.max(initial=0)), 1)
    mat = np.zeros((len(pieces), last + 1), dtype=np.uint32)
    mat[:, :last][np.arange(last) < lens[:, None]] = np.frombuffer(flat, dtype=np.uint32)   # row by row, in front of each length
    mat[:, last] = lens
    return mat, names


def read_walks_device(path, node_ids=None, device=0):
    """``read_walks`` with the file read in device memory (``pw_corpus_read_device``, csrc/corpus_dev.hip.h): the text is
    uploaded, tokenised and numbered by first appearance on the GPU and the matrix is laid out there.  Returns
    ``(d_walks, names)``: ``d_walks`` a contiguous int32 CUDA tensor ``[n_lines, W]`` (uint32 storage), what
    ``train_sgns_device`` and ``save_walks_device`` take, equal to ``read_walks(path, node_ids)[0]`` cell for cell; ``names``
    the same list.  Only the file's bytes go up and only the names come down.

    The device reader takes files whose bytes are all in ``{\\t, \\n, \\r, 0x20 .. 0x7E}``; any other file (a UTF-8 name,
    ``\\x0b``, NUL, ..., the empty file, 4 GiB or more) is read by ``read_walks`` and uploaded -- no error.  With ``node_ids``
    the remap from first-appearance numbers to positions in ``node_ids`` is built on the host over the names (not the tokens)
    and applied on the device; an unknown token raises ``read_walks``' ``ValueError``.  ``read_walks_device.last_stats``:
    ``"reader"`` (``"device"`` or ``"host"``), ``call_ms``, and for the device reader ``pw_corpus_dev_stats`` (``upload_ms``,
    ``scan_ms``, ``tokens_ms``, ``fill_ms``, ``file_bytes``, ``lines``, ``tokens``, ``names``), ``names_ms`` (the names'
    download and decoding) and ``remap_ms``."""
    import time

    import torch

    from .engine import _edgelist_names, _no_device

    lib = _lib.load()
    if int(lib.pw_device_count()) <= 0:
        _no_device()
    dev = torch.device("cuda", int(device or 0))
    t0 = time.perf_counter()
    h, ids, st = C.c_void_p(), C.c_void_p(), _lib.PwCorpusDevStats()
    rc = lib.pw_corpus_read_device(os.fsencode(path), dev.index, C.byref(h), C.byref(ids), C.byref(st))
    if rc in (_lib.EDGELIST_NEEDS_HOST_READER, _lib.EDGELIST_IO):
        mat, names = read_walks(path, node_ids)   # (a file that cannot be opened raises here what open() raises)
        d_walks = torch.from_numpy(mat.view(np.int32)).to(dev)
        read_walks_device.last_stats = {"reader": "host", "call_ms": (time.perf_counter() - t0) * 1e3, "lines": mat.shape[0],
                                        "tokens": int(mat[:, -1].sum()), "names": len(names)}
        return d_walks, names
    _lib.check(rc)
    try:
        stats = st.as_dict()
        shape = [C.c_uint64(0) for _ in range(3)]
        _lib.check(lib.pw_corpus_dev_shape(h, *[C.byref(s) for s in shape]))
        n_rows, width, _ = (int(s.value) for s in shape)
        d_walks = torch.empty((n_rows, width), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(lib.pw_corpus_dev_fill(h, C.c_void_p(d_walks.data_ptr())))
        t1 = time.perf_counter()
        names = _edgelist_names(lib, ids, stats["names"])
        stats["names_ms"] = (time.perf_counter() - t1) * 1e3
    finally:
        lib.pw_corpus_dev_destroy(h)
        lib.pw_edgelist_ids_destroy(ids)
    t1 = time.perf_counter()
    if node_ids is not None:
        d_walks, names = _remap_device(d_walks, names, node_ids)
    stats["remap_ms"] = (time.perf_counter() - t1) * 1e3
    stats["reader"] = "device"
    stats["call_ms"] = (time.perf_counter() - t0) * 1e3
    read_walks_device.last_stats = stats
    return d_walks, names


def _remap_device(d_walks, names, node_ids):
    """First-appearance numbers -> positions in ``node_ids``: a table over the names, gathered on the device."""
    import torch

    wanted = [str(x) for x in node_ids]
    index = {}
    for i, name in enumerate(wanted):
        index.setdefault(name, i)
    cells = d_walks[:, :-1]
    in_row = torch.arange(cells.shape[1], device=d_walks.device) < d_walks[:, -1:]   # the cells in front of each row's length
    unknown = next((k for k, name in enumerate(names) if name not in index), None)   # the first in the file: names are in that order
    if unknown is not None:
        line = int(((cells == unknown) & in_row).any(dim=1).nonzero()[0]) + 1
        raise _unknown_token(names[unknown], line, len(wanted))
    if names:
        table = torch.tensor([index[name] for name in names], dtype=torch.int32, device=d_walks.device)
        mapped = torch.where(in_row, table[cells.long()], torch.zeros((), dtype=torch.int32, device=d_walks.device))
        d_walks = torch.cat([mapped, d_walks[:, -1:]], dim=1).contiguous()
    return d_walks, wanted


read_walks_device.last_stats = None
