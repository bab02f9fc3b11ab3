"""Device-side walk engine: Python face of the C ABI (include/pecanpy_amd.h).

``WalkEngine`` owns one device-resident graph handle (``pw_csr_create`` / ``pw_dense_create``) and
exposes the walk operator that replaces the reference's ``Base._random_walks`` + ``has_nbrs`` +
``move_forward`` (reference src/pecanpy/pecanpy.py:164-210).  NumPy arrays go through
``pw_simulate`` (host pointers); torch CUDA tensors go through ``pw_simulate_device`` (nothing
crosses PCIe).  ``simulate_sharded`` is the multi-GPU path: one process per GPU, the shuffled job
array split into contiguous ranges, graph replicated, one gather of the walk shards at the end.
"""
import contextlib
import ctypes as C
import os
import time

import numpy as np

from . import _lib
from ._lib import MODE_IDS, PwError, PwStats

__all__ = ["WalkEngine", "MultiWalkEngine", "visible_devices", "shard_bounds", "auto_rank0_share", "tapered_bounds", "PwError"]


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def shard_bounds(n_jobs, world_size, rank0_share=None):
    """Contiguous job ranges [lo, hi) per rank.

    ``rank0_share`` (default 1.0 = uniform): rank 0's shard as a fraction of a uniform one.  Rank 0 is where the walk
    matrix is assembled -- it also writes the rows nobody sends and scatters what arrives -- so giving it fewer jobs to
    walk takes that work off the pass's critical path (``auto_rank0_share``); the other ranks share the rest evenly."""
    if rank0_share is None or world_size <= 1 or rank0_share == 1.0:
        return [((r * n_jobs) // world_size, ((r + 1) * n_jobs) // world_size) for r in range(world_size)]
    share = min(max(float(rank0_share), 0.0), float(world_size))
    n0 = min(n_jobs, int(round(share * n_jobs / world_size)))
    rest = n_jobs - n0
    cuts = [0, n0] + [n0 + ((r * rest) // (world_size - 1)) for r in range(1, world_size)]
    return [(cuts[r], cuts[r + 1]) for r in range(world_size)]


def auto_rank0_share(world_size, gather=True):
    """Rank 0's share of a uniform shard when it assembles the matrix (model of DESIGN.md section 6: at 8 GPUs its
    prefill of the other shards' isolated rows, the receive kernels and the scatter of 7/8 of the rows cost about half
    of a 1/8 shard's walk time; nothing extra at 1 GPU, proportionally less in between)."""
    if not gather or world_size <= 1:
        return 1.0
    return max(0.4, 1.0 - 0.5 * (min(world_size, 8) - 1) / 7.0)


def tapered_bounds(n_jobs, n_chunks):
    """Contiguous ranges [lo, hi) of decreasing size (weights n_chunks, n_chunks - 1, ..., 1): a shard walked in such
    chunks, each travelling to rank 0 while the next is walked, leaves only its SMALLEST chunk's transfer exposed at the
    end of the pass (4 chunks: 10 % of the shard instead of 25 %)."""
    n_chunks = max(1, int(n_chunks))
    total = n_chunks * (n_chunks + 1) // 2
    cuts = [0]
    acc = 0
    for c in range(n_chunks):
        acc += n_chunks - c
        cuts.append((acc * n_jobs) // total)
    return [(cuts[c], cuts[c + 1]) for c in range(n_chunks)]


def check_edge_index(edge_index, edge_weight=None, num_nodes=None):
    """Shape and dtype rules of ``from_edge_index``; returns ``m``.  Looks at metadata only (no library, no device): an
    integer ``[2, m]`` torch tensor or NumPy array, a float ``[m]`` weight vector, a non-negative ``num_nodes``."""
    def describe(x, what):
        if isinstance(x, np.ndarray):
            kind = "int" if x.dtype.kind in "iu" else "float" if x.dtype.kind == "f" else "other"
            if x.dtype == np.uint64:
                kind = "uint64"
            return tuple(x.shape), kind
        if type(x).__module__.split(".")[0] == "torch" and hasattr(x, "is_floating_point"):
            import torch

            kind = ("float" if x.is_floating_point() else
                    "other" if x.is_complex() or x.dtype == torch.bool else
                    "uint64" if x.dtype == getattr(torch, "uint64", None) else "int")
            return tuple(x.shape), kind
        raise ValueError(f"{what} must be a torch tensor or a NumPy array, got {type(x).__name__}")

    shape, kind = describe(edge_index, "edge_index")
    if len(shape) != 2 or shape[0] != 2:
        raise ValueError(f"edge_index must have shape [2, m], got {list(shape)}")
    if kind == "uint64":   # (ids of 2^63 or more would wrap negative on the way to int64)
        raise ValueError("edge_index of dtype uint64 is not accepted: pass int64 (or a narrower integer type)")
    if kind != "int":
        raise ValueError("edge_index must hold integers (vertex i is id i)")
    m = int(shape[1])
    if edge_weight is not None:
        wshape, wkind = describe(edge_weight, "edge_weight")
        if wkind != "float":
            raise ValueError("edge_weight must hold floats")
        if len(wshape) != 1 or wshape[0] != m:
            raise ValueError(f"edge_weight must have shape [{m}] (one weight per edge), got {list(wshape)}")
    if num_nodes is not None and (int(num_nodes) != num_nodes or int(num_nodes) < 0):
        raise ValueError("num_nodes must be a non-negative integer")
    if num_nodes is not None and int(num_nodes) == 0 and m > 0:
        raise ValueError("num_nodes = 0 with a non-empty edge list (omit num_nodes to have it inferred)")
    return m


def check_dense_matrix(mat, device=None):
    """Shape and dtype rules of ``from_dense_tensor``; returns ``n``.  Looks at metadata only (no library, no device): a
    square, non-empty 2-d torch tensor or NumPy array of a real dtype (float or integer; not bool, not complex), and a
    ``device`` that does not contradict the device of a CUDA tensor."""
    if isinstance(mat, np.ndarray):
        kind = {"f": "float", "i": "int", "u": "int", "b": "bool", "c": "complex"}.get(mat.dtype.kind, "other")
    elif hasattr(mat, "is_floating_point") and hasattr(mat, "is_complex") and hasattr(mat, "shape"):   # a torch tensor
        kind = ("complex" if mat.is_complex() else "float" if mat.is_floating_point() else
                "bool" if str(mat.dtype).endswith("bool") else "int")
    else:
        raise ValueError(f"dense adjacency must be a torch tensor or a NumPy array, got {type(mat).__name__}")
    shape = tuple(mat.shape)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError(f"dense adjacency must be a square 2-d matrix, got shape {list(shape)}")
    if shape[0] == 0:
        raise ValueError("dense adjacency must have at least one vertex")
    if shape[0] > 0xFFFFFFFF:
        raise ValueError("dense adjacency has more than 2^32 - 1 vertices")
    if kind not in ("float", "int"):
        raise ValueError(f"dense adjacency must hold real numbers (float or integer), got {mat.dtype}")
    if getattr(mat, "is_cuda", False) and device is not None and int(device) != mat.device.index:
        raise ValueError(f"the matrix lives on cuda:{mat.device.index}, the engine was asked for device {int(device)}")
    return int(shape[0])


def _no_device():
    """The one place the Python layer says that the library sees no GPU."""
    raise PwError("no HIP device visible (libpecanpy_amd needs a GPU; there is no CPU fallback)")


def _edge_list_to_device(lib, edge_index, edge_weight, device):
    """The device tensors ``(src, dst, w, dev, host_bytes)`` of an edge list that passed ``check_edge_index``: a CUDA tensor is
    used where it is, host input is uploaded; torch's stream is synchronised (the library works on its own streams)."""
    import torch

    host_bytes = 0
    if isinstance(edge_index, torch.Tensor) and edge_index.is_cuda:
        dev = edge_index.device
        if device is not None and int(device) != dev.index:
            raise ValueError(f"edge_index lives on cuda:{dev.index}, the engine was asked for device {int(device)}")
    else:
        dev = torch.device("cuda", int(device or 0))
        if int(lib.pw_device_count()) <= 0:
            _no_device()

    def to_dev(x, dtype):
        nonlocal host_bytes
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        if not t.is_cuda:
            host_bytes += t.numel() * t.element_size()
        return t.to(device=dev, dtype=dtype)

    ei = to_dev(edge_index, torch.int64)
    src, dst = ei[0].contiguous(), ei[1].contiguous()   # (rows of a contiguous [2, m] tensor: views, no copy)
    w = to_dev(edge_weight, torch.float32).contiguous() if edge_weight is not None else None
    if w is not None and w.device != dev:
        raise ValueError("edge_index and edge_weight must be on the same device")
    torch.cuda.current_stream(dev).synchronize()   # inputs were produced on torch's stream
    return src, dst, w, dev, host_bytes


def _edgelist_names(lib, ids, n):
    """The vertex names of a ``pw_edgelist_ids`` in first-appearance order."""
    dims = [C.c_uint64(0), C.c_uint64(0)]
    _lib.check(lib.pw_edgelist_ids_shape(ids, C.byref(dims[0]), C.byref(dims[1])))
    id_bytes = int(dims[1].value)
    offs = np.empty(n + 1, dtype=np.uint64)
    chars = np.empty(max(id_bytes, 1), dtype=np.uint8)
    _lib.check(lib.pw_edgelist_ids_export(ids, _np_ptr(offs), _np_ptr(chars)))
    blob = chars[:id_bytes].tobytes().decode("ascii")
    cuts = offs.tolist()
    return [blob[a:b] for a, b in zip(cuts, cuts[1:])]


def _csr_dev_shape(lib, c):
    """``(n_nodes, nnz, insertions, dropped, build_ms)`` of a ``pw_csr_dev``."""
    shape = [C.c_uint64(0) for _ in range(4)]
    ms = C.c_double(0)
    _lib.check(lib.pw_csr_dev_shape(c, *[C.byref(s) for s in shape], C.byref(ms)))
    return tuple(int(s.value) for s in shape) + (float(ms.value),)


@contextlib.contextmanager
def _coo_csr_dev(lib, src, dst, w, dev, m, num_nodes, directed):
    """``pw_coo_to_csr_device`` over the tensors of ``_edge_list_to_device``.  Yields ``(c, t_called, shape)``: the ``pw_csr_dev``,
    destroyed when the block is left, ``time.perf_counter()`` behind the call, and ``_csr_dev_shape``'s tuple."""
    c = C.c_void_p()
    _lib.check(lib.pw_coo_to_csr_device(dev.index, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                        C.c_void_p(w.data_ptr() if w is not None else 0), m,
                                        int(num_nodes or 0), int(bool(directed)), C.byref(c)))
    try:
        t_called = time.perf_counter()
        yield c, t_called, _csr_dev_shape(lib, c)
    finally:
        lib.pw_csr_dev_destroy(c)


@contextlib.contextmanager
def _edgelist_csr_dev(lib, path, weighted, directed, delimiter, device, flags):
    """``pw_edgelist_read_device_ex`` with ``flags``.  Yields ``None`` when the file needs the host reader (the library's two
    decline codes, a delimiter that cannot be encoded), else ``(c, st, read_call_ms, t_called, shape, names)``: the
    ``pw_csr_dev``, destroyed with the id handle when the block is left, the reader's statistics, the wall clock of the library
    call alone (the device check, which may start the runtime, and the delimiter's encoding lie in front of it),
    ``time.perf_counter()`` behind the call, ``_csr_dev_shape``'s tuple and the vertex names -- read in that order, so the
    names fall into whatever the caller times from ``t_called`` on."""
    if int(lib.pw_device_count()) <= 0:
        _no_device()
    try:
        raw_delim = delimiter.encode("utf-8", "surrogateescape")
    except (AttributeError, UnicodeError):
        raw_delim = None
    if raw_delim is None or b"\0" in raw_delim:
        yield None
        return
    t0 = time.perf_counter()
    c, ids, st = C.c_void_p(), C.c_void_p(), _lib.PwEdgelistDevStats()
    rc = lib.pw_edgelist_read_device_ex(os.fsencode(path), int(bool(weighted)), int(bool(directed)), raw_delim, int(device or 0),
                                        flags, C.byref(c), C.byref(ids), C.byref(st))
    if rc in (_lib.EDGELIST_NEEDS_HOST_READER, _lib.EDGELIST_IO):
        yield None
        return
    _lib.check(rc)
    try:
        t_called = time.perf_counter()
        shape = _csr_dev_shape(lib, c)
        yield c, st, (t_called - t0) * 1e3, t_called, shape, _edgelist_names(lib, ids, shape[0])
    finally:
        lib.pw_csr_dev_destroy(c)
        lib.pw_edgelist_ids_destroy(ids)


def _csr_engine(cls, lib, c, n, nnz, device):
    """A ``pw_csr_dev`` as a CSR engine that carries ``eng.csr``: the three arrays are exported once and
    ``pw_csr_create_device`` reads them (no second download).  Returns ``(eng, t_exported, t_created)``:
    ``time.perf_counter()`` behind the export and behind the handle."""
    indptr = np.empty(n + 1, dtype=np.uint32)
    indices = np.empty(nnz, dtype=np.uint32)
    data = np.empty(nnz, dtype=np.float32)
    _lib.check(lib.pw_csr_dev_export(c, _np_ptr(indptr), _np_ptr(indices), _np_ptr(data)))
    t_exported = time.perf_counter()
    h = C.c_void_p()
    _lib.check(lib.pw_csr_create_device(c, _np_ptr(indptr), _np_ptr(indices), _np_ptr(data), C.byref(h)))
    t_created = time.perf_counter()
    eng = cls(h, lib, "csr", n, device)
    eng._max_degree = int(np.diff(indptr.astype(np.int64)).max()) if n else 0
    eng._nnz = nnz
    eng.csr = (indptr, indices, data)
    return eng, t_exported, t_created


class WalkEngine:
    def __init__(self, handle, lib, kind, n_nodes, device):
        self._h = handle
        self._lib = lib
        self.kind = kind
        self.n_nodes = n_nodes
        self.device = device
        self.last_stats = None
        self._max_degree = n_nodes   # upper bound; from_csr / from_dense narrow it
        self._nnz = 0                # CSR entries (from_csr)

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def from_csr(cls, indptr, indices, data=None, device=0):
        lib = _lib.load()
        indptr = np.ascontiguousarray(indptr, dtype=np.uint32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float32)
        h = C.c_void_p()
        _lib.check(lib.pw_csr_create(_np_ptr(indptr), _np_ptr(indices), _np_ptr(data),
                                     indptr.size - 1, indices.size, int(device), C.byref(h)))
        eng = cls(h, lib, "csr", indptr.size - 1, int(device))
        eng._max_degree = int(np.diff(indptr.astype(np.int64)).max()) if indptr.size > 1 else 0
        eng._nnz = int(indices.size)
        return eng

    @classmethod
    def from_dense(cls, data, device=0):
        lib = _lib.load()
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[0] != data.shape[1]:
            raise ValueError("dense adjacency must be a square matrix")
        h = C.c_void_p()
        _lib.check(lib.pw_dense_create(_np_ptr(data), data.shape[0], int(device), C.byref(h)))
        return cls(h, lib, "dense", data.shape[0], int(device))

    @classmethod
    def from_dense_bits(cls, bits, n_nodes, device=0):
        """Unweighted dense graph from packed adjacency rows: ``bits`` is ``uint64[n, ceil(n/64)]`` as a
        NumPy array (host) or an int64 torch CUDA tensor (device, same bit pattern)."""
        lib = _lib.load()
        wpr = (int(n_nodes) + 63) // 64
        h = C.c_void_p()
        if isinstance(bits, np.ndarray):
            bits = np.ascontiguousarray(bits, dtype=np.uint64)
            if bits.size != int(n_nodes) * wpr:
                raise ValueError("bits must hold n * ceil(n/64) words")
            _lib.check(lib.pw_dense_create_bits(_np_ptr(bits), int(n_nodes), 0, int(device), C.byref(h)))
        else:  # torch CUDA tensor
            if not bits.is_cuda or not bits.is_contiguous() or bits.numel() != int(n_nodes) * wpr:
                raise ValueError("bits must be a contiguous CUDA tensor of n * ceil(n/64) 64-bit words")
            import torch

            torch.cuda.current_stream(bits.device).synchronize()
            _lib.check(lib.pw_dense_create_bits(C.c_void_p(bits.data_ptr()), int(n_nodes), 1, int(device), C.byref(h)))
        return cls(h, lib, "dense", int(n_nodes), int(device))

    @classmethod
    def from_edge_index(cls, edge_index, edge_weight=None, num_nodes=None, directed=False, device=None):
        """CSR handle from an edge list, built on the device (``pw_coo_to_csr_device`` + ``pw_csr_create_device``).

        ``edge_index``: integer ``[2, m]`` torch tensor or NumPy array; ``edge_weight``: float ``[m]`` or ``None``.  A
        CUDA tensor is used where it is (``device`` defaults to its device); host input is uploaded first and takes the
        same path.  Vertex ``i`` is id ``i`` (no first-appearance renumbering, unlike the edge-list file reader); the
        semantics are the reference's ``add_edge`` / ``to_csr``: non-positive weights dropped, the reverse edge inserted
        unless ``directed``, the last insertion of a pair wins.

        The engine carries the exported host arrays as ``eng.csr = (indptr, indices, data)`` (``data`` all ones when
        unweighted) and ``eng.build_stats``: ``edge_list_host_bytes`` (bytes of the edge list that crossed the host:
        0 for CUDA input), ``n_nodes``, ``nnz``, ``insertions``, ``dropped``, ``build_ms`` (device time of the CSR build)
        and the wall clock of the stages (``coo_call_ms``, ``export_ms``, ``handle_ms``)."""
        m = check_edge_index(edge_index, edge_weight, num_nodes)   # ValueError before the library or a device is touched
        lib = _lib.load()
        src, dst, w, dev, host_bytes = _edge_list_to_device(lib, edge_index, edge_weight, device)
        t0 = time.perf_counter()
        with _coo_csr_dev(lib, src, dst, w, dev, m, num_nodes, directed) as (c, t1, (n, nnz, insertions, dropped, build_ms)):
            eng, t2, t3 = _csr_engine(cls, lib, c, n, nnz, dev.index)
        eng.build_stats = {"edge_list_host_bytes": int(host_bytes), "n_nodes": n, "nnz": nnz, "insertions": insertions,
                           "dropped": dropped, "build_ms": build_ms, "coo_call_ms": (t1 - t0) * 1e3,
                           "export_ms": (t2 - t1) * 1e3, "handle_ms": (t3 - t2) * 1e3}
        return eng

    @classmethod
    def from_edgelist_file(cls, path, weighted, directed, delimiter="\t", device=None):
        """CSR handle from an edge-list FILE, parsed and built on the device (``pw_edgelist_read_device`` +
        ``pw_csr_create_device``): the text is uploaded, tokenised and numbered by first appearance in device memory and
        handed to the build of ``from_edge_index``.  The result is what ``SparseGraph.read_edg`` gives, array for array.

        Returns the engine, or ``None`` when the file needs the host reader (everything on which the reference warns or
        raises, weight literals outside the class the device parses exactly, a file that cannot be opened, ...: see
        include/pecanpy_amd.h) -- no error; the caller takes ``read_edg``.  The engine carries ``eng.csr = (indptr,
        indices, data)`` (``data`` all ones when unweighted), ``eng.ids`` (the vertex names, first-appearance order) and
        ``eng.build_stats``: the library's ``upload_ms``, ``scan_ms``, ``ids_ms``, ``build_ms`` (wall clock of the
        stages), ``lines``, ``n_nodes``, ``file_bytes``, and ``nnz``, ``insertions``, ``csr_kernels_ms`` (device time of
        the CSR build's kernels), ``read_call_ms``, ``export_ms``, ``handle_ms``."""
        lib = _lib.load()
        with _edgelist_csr_dev(lib, path, weighted, directed, delimiter, device, 0) as r:
            if r is None:
                return None
            c, st, read_call_ms, t1, (n, nnz, insertions, _, csr_kernels_ms), names = r
            eng, t2, t3 = _csr_engine(cls, lib, c, n, nnz, int(device or 0))
        eng.ids = names
        eng.build_stats = {**st.as_dict(), "nnz": nnz, "insertions": insertions, "csr_kernels_ms": csr_kernels_ms,
                           "read_call_ms": read_call_ms, "export_ms": (t2 - t1) * 1e3, "handle_ms": (t3 - t2) * 1e3}
        return eng

    @classmethod
    def from_dense_tensor(cls, mat, device=None):
        """Dense handle from a matrix, built on the device (``pw_dense_create_device``): the same handle as ``from_dense`` on
        the same values, without the host pass over the ``n * n`` entries.

        ``mat``: square 2-d torch tensor or NumPy array.  float64 and float32 are used as they are (float32 is widened to
        float64 inside the kernels, which is exact); other real dtypes are converted to float64.  A CUDA tensor is used
        where it is (made contiguous if needed; ``device`` defaults to its device); host input is uploaded first and takes
        the same path.  The matrix is not referenced after the call.

        ``eng.build_stats``: ``matrix_host_bytes`` (bytes of the matrix that crossed from the host: 0 for CUDA input),
        ``n_nodes``, ``nnz``, ``unit``, ``build_ms`` (device time of the build's kernels) and the wall clock of the stages
        (``upload_ms``: conversion / upload / making contiguous; ``create_call_ms``: the library call)."""
        n = check_dense_matrix(mat, device)   # ValueError before the library or a device is touched
        import torch

        lib = _lib.load()
        t0 = time.perf_counter()
        host_bytes = 0
        if isinstance(mat, torch.Tensor) and mat.is_cuda:
            t = mat
        else:
            if int(lib.pw_device_count()) <= 0:
                _no_device()
            if isinstance(mat, np.ndarray):
                if mat.dtype not in (np.float32, np.float64):
                    mat = mat.astype(np.float64)
                t = torch.from_numpy(np.ascontiguousarray(mat))
            else:
                t = mat if mat.dtype in (torch.float32, torch.float64) else mat.to(torch.float64)
            host_bytes = t.numel() * t.element_size()
            t = t.to(torch.device("cuda", int(device or 0)))
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        t = t.contiguous()
        dev = t.device
        torch.cuda.current_stream(dev).synchronize()   # the matrix was produced on torch's stream
        t1 = time.perf_counter()
        h, ms = C.c_void_p(), C.c_double(0)
        _lib.check(lib.pw_dense_create_device(dev.index, C.c_void_p(t.data_ptr()), int(t.dtype == torch.float32), n,
                                              C.byref(h), C.byref(ms)))
        t2 = time.perf_counter()
        del t
        eng = cls(h, lib, "dense", n, dev.index)
        shape = eng._dense_shape()
        eng._max_degree, eng._nnz = shape["max_degree"], shape["nnz"]
        eng.build_stats = {"matrix_host_bytes": int(host_bytes), "n_nodes": n, "nnz": shape["nnz"], "unit": eng._dense_flags()[0],
                           "build_ms": float(ms.value), "upload_ms": (t1 - t0) * 1e3, "create_call_ms": (t2 - t1) * 1e3}
        return eng

    @classmethod
    def dense_from_edge_index(cls, edge_index, edge_weight=None, num_nodes=None, directed=False, device=None):
        """Dense handle from an edge list, built on the device: ``pw_coo_to_csr_device`` (the rules of ``from_edge_index``),
        then ``pw_dense_create_from_csr``.  The matrix the handle stands for holds the float32 weights widened to float64
        (1.0 everywhere when ``edge_weight`` is ``None``).  ``eng.build_stats`` has the keys of ``from_edge_index``
        (``export_ms`` is 0: nothing is exported; ``handle_ms``: the dense handle) and ``dense_build_ms``, the device time
        of the dense build's kernels."""
        m = check_edge_index(edge_index, edge_weight, num_nodes)   # ValueError before the library or a device is touched
        lib = _lib.load()
        src, dst, w, dev, host_bytes = _edge_list_to_device(lib, edge_index, edge_weight, device)
        t0 = time.perf_counter()
        with _coo_csr_dev(lib, src, dst, w, dev, m, num_nodes, directed) as (c, t1, (n, nnz, insertions, dropped, build_ms)):
            h, dense_ms = C.c_void_p(), C.c_double(0)
            _lib.check(lib.pw_dense_create_from_csr(c, C.byref(h), C.byref(dense_ms)))
            t2 = time.perf_counter()
        eng = cls(h, lib, "dense", n, dev.index)
        eng._max_degree, eng._nnz = eng._dense_shape()["max_degree"], nnz
        eng.build_stats = {"edge_list_host_bytes": int(host_bytes), "n_nodes": n, "nnz": nnz, "insertions": insertions,
                           "dropped": dropped, "build_ms": build_ms, "coo_call_ms": (t1 - t0) * 1e3, "export_ms": 0.0,
                           "handle_ms": (t2 - t1) * 1e3, "dense_build_ms": float(dense_ms.value)}
        return eng

    @classmethod
    def dense_from_edgelist_file(cls, path, weighted, directed, delimiter="\t", device=None):
        """Dense handle from an edge-list FILE, parsed and built on the device: ``pw_edgelist_read_device_ex`` with the
        float64 weights kept (``PW_EDGELIST_KEEP_F64``), then ``pw_dense_create_from_csr``.  The handle is the one
        ``from_dense`` makes of ``DenseGraph.read_edg``'s matrix: the weights are the float64 literals of the file, not their
        float32 roundings.  The CSR is neither exported nor turned into a CSR handle, and no ``n * n`` host array exists.

        Returns the engine, or ``None`` when the file needs the host reader, under the rules of ``from_edgelist_file``.
        The engine carries ``eng.ids`` and ``eng.build_stats``: the reader's ``upload_ms``, ``scan_ms``, ``ids_ms``,
        ``build_ms``, ``lines``, ``n_nodes``, ``file_bytes``, and ``nnz``, ``insertions``, ``csr_kernels_ms``,
        ``dense_build_ms`` (device time of the dense build's kernels), ``read_call_ms``, ``handle_ms`` (names and the dense
        handle), ``unit`` and ``matrix_host_bytes`` (0)."""
        lib = _lib.load()
        with _edgelist_csr_dev(lib, path, weighted, directed, delimiter, device, _lib.EDGELIST_KEEP_F64) as r:
            if r is None:
                return None
            c, st, read_call_ms, t1, (n, nnz, insertions, _, csr_kernels_ms), names = r
            h, dense_ms = C.c_void_p(), C.c_double(0)
            _lib.check(lib.pw_dense_create_from_csr(c, C.byref(h), C.byref(dense_ms)))
            t2 = time.perf_counter()
        eng = cls(h, lib, "dense", n, int(device or 0))
        eng._max_degree, eng._nnz = eng._dense_shape()["max_degree"], nnz
        eng.ids = names
        eng.build_stats = {**st.as_dict(), "nnz": nnz, "insertions": insertions, "csr_kernels_ms": csr_kernels_ms,
                           "dense_build_ms": float(dense_ms.value), "read_call_ms": read_call_ms, "handle_ms": (t2 - t1) * 1e3,
                           "unit": eng._dense_flags()[0], "matrix_host_bytes": 0}
        return eng

    def _dense_shape(self):
        v = [C.c_uint32(0) for _ in range(4)]
        _lib.check(self._lib.pw_dense_shape(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_nodes", "nnz", "words_per_row", "max_degree"), (int(x.value) for x in v)))

    def _dense_flags(self):
        f = C.c_uint32(0)
        _lib.check(self._lib.pw_dense_export(self._h, None, None, None, None, None, C.byref(f)))
        return bool(f.value & 1), bool(f.value & 2)

    def dense_arrays(self, rows=True):
        """Host copies of a dense handle's arrays (``pw_dense_export``) as a dict: ``indptr`` uint32[n + 1], ``indices``
        uint32[nnz] and ``data`` float64[nnz] (the rows compressed in ascending column order; ``data`` all ones for a unit
        handle), ``adjbits`` uint64[n, words_per_row], ``deg`` uint32[n], the flags ``unit`` and ``dense_nonneg``, and
        ``nnz``, ``words_per_row``, ``max_degree``.  ``rows=False`` leaves ``indices`` / ``data`` out (handles made from
        packed bits have none)."""
        shape = self._dense_shape()
        n, nnz, wpr = shape["n_nodes"], shape["nnz"], shape["words_per_row"]
        out = {"indptr": np.zeros(n + 1, dtype=np.uint32), "adjbits": np.zeros((n, wpr), dtype=np.uint64),
               "deg": np.zeros(n, dtype=np.uint32)}
        if rows:
            out["indices"] = np.zeros(nnz, dtype=np.uint32)
            out["data"] = np.zeros(nnz, dtype=np.float64)
        flags = C.c_uint32(0)
        _lib.check(self._lib.pw_dense_export(self._h, _np_ptr(out["indptr"]), _np_ptr(out.get("indices")), _np_ptr(out.get("data")),
                                             _np_ptr(out["adjbits"]), _np_ptr(out["deg"]), C.byref(flags)))
        out.update(unit=bool(flags.value & 1), dense_nonneg=bool(flags.value & 2), nnz=nnz, words_per_row=wpr,
                   max_degree=shape["max_degree"])
        return out

    def compute_thresholds(self, gamma):
        """node2vec+ noise thresholds of a dense handle computed on the device from its compressed rows
        (``pw_dense_noise_thresholds``: what ``pw_noise_thresholds_dense`` gives for the matrix, bit for bit) and installed
        in the handle; returns them as float32[n_nodes]."""
        thr = np.zeros(self.n_nodes, dtype=np.float32)
        _lib.check(self._lib.pw_dense_noise_thresholds(self._h, float(gamma), _np_ptr(thr)))
        return thr

    def set_thresholds(self, thr):
        thr = np.ascontiguousarray(thr, dtype=np.float32)
        if thr.size != self.n_nodes:
            raise ValueError("threshold array must have one entry per node")
        _lib.check(self._lib.pw_graph_set_thresholds(self._h, _np_ptr(thr)))

    def index_info(self):
        """Device time (ms) and bytes of the per-graph index built at creation, and the number of entries of the
        lane kernel's common-neighbour lists (0 when that index was not built)."""
        ms, nbytes, entries = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.pw_graph_index_info(self._h, C.byref(ms), C.byref(nbytes), C.byref(entries)))
        return {"build_ms": float(ms.value), "index_bytes": int(nbytes.value), "lane_list_entries": int(entries.value)}

    def lane_index(self):
        """Test hook: ``(n_in, rev_pos, offsets, entries)`` of the lane index (see ``pw_lane_index_export``)."""
        n = max(self._nnz, 1)   # (dense handles / no lane index: the library's PW_ERR_UNSUPPORTED surfaces below)
        n_in = np.zeros(n, dtype=np.uint32)
        rev = np.zeros(n, dtype=np.uint32)
        _lib.check(self._lib.pw_lane_index_export(self._h, _np_ptr(n_in), _np_ptr(rev), None))   # counts first
        n_in, rev = n_in[: self._nnz], rev[: self._nnz]
        total = int(n_in.sum(dtype=np.int64))
        if total != self.index_info()["lane_list_entries"]:
            raise _lib.PwError("lane index: the per-entry counts do not add up to the number of list entries")
        entries = np.zeros(max(total, 1), dtype=np.uint32)
        _lib.check(self._lib.pw_lane_index_export(self._h, None, None, _np_ptr(entries)))
        off = np.concatenate([[0], np.cumsum(n_in, dtype=np.int64)])
        return n_in, rev, off, entries[:total]

    def close(self):
        if self._h is not None and self._h.value:
            self._lib.pw_graph_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # ---- the walk operator ----------------------------------------------------------------
    def simulate(self, mode, p, q, extend, starts, walk_length, seed=None, stream_skip=0):
        """Host-buffer variant: returns ``uint32[n_jobs, walk_length + 2]`` (NumPy)."""
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        out = np.empty((starts.size, walk_length + 2), dtype=np.uint32)
        st = PwStats()
        _lib.check(self._lib.pw_simulate(
            self._h, MODE_IDS[mode], float(p), float(q), int(bool(extend)), _np_ptr(starts),
            starts.size, int(walk_length), int(seed is not None), int(seed or 0) & 0xFFFFFFFF,
            int(stream_skip), _np_ptr(out), C.byref(st)))
        self.last_stats = st.as_dict()
        return out

    def simulate_device(self, mode, p, q, extend, d_starts, walk_length, seed=None, stream_skip=0,
                        out=None):
        """Device-buffer variant on torch CUDA tensors (int32 storage viewed as uint32)."""
        import torch

        if not d_starts.is_cuda or d_starts.dtype != torch.int32 or not d_starts.is_contiguous():
            raise ValueError("d_starts must be a contiguous int32 CUDA tensor")
        n = d_starts.numel()
        if out is None:
            out = torch.empty((n, walk_length + 2), dtype=torch.int32, device=d_starts.device)
        torch.cuda.current_stream(d_starts.device).synchronize()  # inputs were produced on torch's stream
        st = PwStats()
        _lib.check(self._lib.pw_simulate_device(
            self._h, MODE_IDS[mode], float(p), float(q), int(bool(extend)),
            C.c_void_p(d_starts.data_ptr()), n, int(walk_length), int(seed is not None),
            int(seed or 0) & 0xFFFFFFFF, int(stream_skip), C.c_void_p(out.data_ptr()), C.byref(st)))
        self.last_stats = st.as_dict()
        return out

    # ---- single transitions (the reference's move_forward / get_normalized_probs callbacks) ---------------
    def step(self, mode, p, q, extend, cur, prev=None, r=None):
        """``move_forward(cur, prev)`` on the device with the uniform draw ``r`` (default: ``np.random.random()``,
        as the reference draws it); returns the next vertex index."""
        if r is None:
            r = np.random.random()
        nxt, pos = C.c_uint32(0), C.c_uint32(0)
        _lib.check(self._lib.pw_step(self._h, MODE_IDS[mode], float(p), float(q), int(bool(extend)), int(cur),
                                     int(prev is not None), int(prev or 0), float(r), C.byref(nxt), C.byref(pos)))
        return int(nxt.value)

    def probs(self, mode, p, q, extend, cur, prev=None):
        """``get_normalized_probs(cur, prev)`` computed by the walk kernels' own step code: float32 (CSR) or
        float64 (dense, node2vec++) vector over ``cur``'s neighbours."""
        dt = np.float32 if self.kind == "csr" and mode != "SparseNode2vecPlusPlus" else np.float64
        buf = np.zeros(self.max_degree() + 1, dtype=dt)
        n = C.c_uint32(0)
        _lib.check(self._lib.pw_probs(self._h, MODE_IDS[mode], float(p), float(q), int(bool(extend)), int(cur),
                                      int(prev is not None), int(prev or 0), _np_ptr(buf), C.byref(n)))
        return buf[: int(n.value)].copy()

    def max_degree(self):
        return int(self._max_degree)

    def precomp_build(self, p, q, extend, first_order):
        """Alias tables on the device (PreComp / PreCompFirstOrder preprocessing)."""
        _lib.check(self._lib.pw_precomp_build(self._h, float(p), float(q), int(bool(extend)),
                                              int(bool(first_order))))

    def precomp_export(self, first_order):
        """Host copies ``(alias_indptr, alias_j, alias_q)`` of the tables built last."""
        n = C.c_uint64(0)
        _lib.check(self._lib.pw_precomp_export(self._h, None, None, None, C.byref(n)))
        alias_indptr = np.zeros(self.n_nodes + 1, dtype=np.uint64)
        alias_j = np.zeros(int(n.value), dtype=np.uint32)
        alias_q = np.zeros(int(n.value), dtype=np.float32)
        _lib.check(self._lib.pw_precomp_export(self._h, _np_ptr(alias_indptr), _np_ptr(alias_j),
                                               _np_ptr(alias_q), C.byref(n)))
        return alias_indptr, alias_j, alias_q

    def stream_sample(self, seed, offset, n):
        """Test hook: doubles ``#offset .. #offset + n`` of ``RandomState(seed).random_sample`` as the device's jump-ahead
        tree and expansion kernels produce them (``pw_stream_sample_device``)."""
        out = np.zeros(int(n), dtype=np.float64)
        _lib.check(self._lib.pw_stream_sample_device(self._h, int(seed) & 0xFFFFFFFF, int(offset), int(n), _np_ptr(out)))
        return out

    def stream_words(self, seed, offset, n):
        """Test hook: the raw 32-bit words ``#offset .. #offset + n`` of the same stream as the device expands them
        (``pw_stream_words_device``)."""
        out = np.zeros(int(n), dtype=np.uint32)
        _lib.check(self._lib.pw_stream_words_device(self._h, int(seed) & 0xFFFFFFFF, int(offset), int(n), _np_ptr(out)))
        return out

    def stream_hold(self, seed, stream_skip, n_draws):
        """Expand the draws ``[stream_skip, stream_skip + n_draws)`` of ``seed``'s stream once; ``simulate_device`` calls inside
        that range (same seed) use them in place until ``stream_release`` -- one jump-ahead tree for a shard walked in chunks."""
        _lib.check(self._lib.pw_stream_hold(self._h, int(seed) & 0xFFFFFFFF, int(stream_skip), int(n_draws)))

    def stream_release(self):
        _lib.check(self._lib.pw_stream_release(self._h))

    def count_stream_draws(self, starts, walk_length):
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        n = C.c_uint64(0)
        _lib.check(self._lib.pw_count_stream_draws(self._h, _np_ptr(starts), starts.size,
                                                   int(walk_length), C.byref(n)))
        return int(n.value)


def visible_devices(spec=None):
    """Device list from a spec: ``None`` / ``"all"`` = every visible GPU, an int = that many (0 = all), a bit mask given as
    ``"mask:0x0f"``, or a comma list ``"0,1,2"`` (a device may be named twice: every entry is a replica)."""
    lib = _lib.load()
    n = int(lib.pw_device_count())
    if spec is None or spec == "all" or spec == 0:
        return list(range(n))
    if isinstance(spec, int):
        return list(range(min(spec, n)))
    if isinstance(spec, str) and spec.startswith("mask:"):
        buf = (C.c_int * 64)()
        k = lib.pw_device_mask_to_list(int(spec[5:], 0), buf, 64)
        if k < 0:
            _lib.check(k)
        return [int(buf[i]) for i in range(k)]
    if isinstance(spec, str):
        return [int(t) for t in spec.split(",") if t.strip() != ""]
    return [int(d) for d in spec]


class MultiWalkEngine:
    """Replicas of one graph on several GPUs, driven from THIS process by one host thread per device inside one C-ABI call
    (``pw_csr_create_multi`` / ``pw_simulate_multi``): what the reference's single process with its Numba thread pool is to
    the CPU (src/pecanpy/cli.py:340-351, pecanpy.py:165-189).  The index is built once and copied device to device.  The
    walk matrix equals a one-device run bit for bit (one random stream, shards addressed by the draws of the earlier ones)."""

    def __init__(self, engines):
        self.engines = list(engines)
        self._lib = self.engines[0]._lib
        self.kind = self.engines[0].kind
        self.n_nodes = self.engines[0].n_nodes
        self.devices = [e.device for e in self.engines]
        self.last_stats = None

    @classmethod
    def from_csr(cls, indptr, indices, data=None, devices=None):
        lib = _lib.load()
        devices = visible_devices(devices)
        if not devices:
            _no_device()
        indptr = np.ascontiguousarray(indptr, dtype=np.uint32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float32)
        dev = (C.c_int * len(devices))(*devices)
        hs = (C.c_void_p * len(devices))()
        _lib.check(lib.pw_csr_create_multi(_np_ptr(indptr), _np_ptr(indices), _np_ptr(data), indptr.size - 1, indices.size,
                                           dev, len(devices), hs))
        engines = []
        for h, d in zip(hs, devices):
            eng = WalkEngine(C.c_void_p(h), lib, "csr", indptr.size - 1, int(d))
            eng._max_degree = int(np.diff(indptr.astype(np.int64)).max()) if indptr.size > 1 else 0
            eng._nnz = int(indices.size)
            engines.append(eng)
        return cls(engines)

    @classmethod
    def from_engine(cls, engine, devices):
        """Replicate an existing one-device engine onto ``devices`` (entries equal to its own device become replicas too)."""
        lib = engine._lib
        engines = [engine]
        for d in list(devices)[1:]:
            h = C.c_void_p()
            _lib.check(lib.pw_graph_replicate(engine._h, int(d), C.byref(h)))
            rep = WalkEngine(h, lib, engine.kind, engine.n_nodes, int(d))
            rep._max_degree, rep._nnz = engine._max_degree, engine._nnz
            engines.append(rep)
        return cls(engines)

    def set_thresholds(self, thr):
        for e in self.engines:
            e.set_thresholds(thr)

    def index_info(self):
        return self.engines[0].index_info()

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    def _handles(self):
        return (C.c_void_p * len(self.engines))(*[e._h for e in self.engines])

    def simulate(self, mode, p, q, extend, starts, walk_length, seed=None, stream_skip=0):
        """Host-buffer variant: ``uint32[n_jobs, walk_length + 2]`` (NumPy), every device writing its own rows."""
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        out = np.empty((starts.size, walk_length + 2), dtype=np.uint32)
        st = PwStats()
        _lib.check(self._lib.pw_simulate_multi(
            self._handles(), len(self.engines), MODE_IDS[mode], float(p), float(q), int(bool(extend)), _np_ptr(starts),
            starts.size, int(walk_length), int(seed is not None), int(seed or 0) & 0xFFFFFFFF, int(stream_skip),
            _np_ptr(out), 0, C.byref(st)))
        self.last_stats = st.as_dict()
        return out

    def simulate_to_device(self, mode, p, q, extend, starts, walk_length, seed=None, stream_skip=0, out=None):
        """The matrix assembled in the memory of the FIRST device (torch int32 tensor): the other devices' rows arrive by
        peer copies over xGMI ("gathered once at the end", BASELINE north star) -- without RCCL, from one process."""
        import torch

        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        dev = torch.device("cuda", self.devices[0])
        if out is None:
            out = torch.empty((starts.size, walk_length + 2), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        st = PwStats()
        _lib.check(self._lib.pw_simulate_multi(
            self._handles(), len(self.engines), MODE_IDS[mode], float(p), float(q), int(bool(extend)), _np_ptr(starts),
            starts.size, int(walk_length), int(seed is not None), int(seed or 0) & 0xFFFFFFFF, int(stream_skip),
            C.c_void_p(out.data_ptr()), 1, C.byref(st)))
        self.last_stats = st.as_dict()
        return out
