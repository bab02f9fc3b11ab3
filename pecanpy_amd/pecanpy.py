"""node2vec walk strategies: the reference's mode classes on the MI355X walk engine.

Drop-in mirror of ``pecanpy.pecanpy`` (reference src/pecanpy/pecanpy.py): same class names,
constructor signature ``(p, q, workers, verbose, extend, gamma, random_state)`` (:83-101) and
methods ``simulate_walks`` (:116-162), ``preprocess_transition_probs`` (:231-238), ``embed``
(:240-290).  What differs is where the walks run: ``Base._random_walks`` (the Numba ``prange``
kernel, :164-210) and the per-mode ``move_forward`` closures are replaced by one call into
``libpecanpy_amd.so`` (HIP kernels for gfx950).  Seeded runs reproduce the reference's
*single-thread* walks bit for bit, independent of how many GPUs execute them.
"""
import numpy as np

from .embed import SgnsSession
from .engine import WalkEngine
from .graph import BaseGraph, DenseGraph, SparseGraph
from .wrappers import Timer

__all__ = ["Base", "FirstOrderUnweighted", "PreCompFirstOrder", "PreComp", "SparseOTF", "DenseOTF",
           "WalkCorpus", "GraphSgnsSession"]


class GraphSgnsSession(SgnsSession):
    """What ``Base.embed_session(fresh_walks=..., holdout_walks=...)`` returns: an ``SgnsSession`` that knows its graph and
    draws walks from it between epochs (see there for the seeds).  ``run(n)`` trains one epoch at a time; ``last_stats`` is
    the last epoch's."""

    def __init__(self, graph, num_walks, walk_length, fresh_walks, holdout_walks, start_nodes=None, **params):
        self._graph, self._num_walks, self._walk_length, self._fresh = graph, num_walks, walk_length, fresh_walks
        self._start_nodes = start_nodes   # (None: every vertex) where every corpus of this session starts
        self.d_holdout = None
        super().__init__(graph._session_walks(num_walks, walk_length, self._seed_of(0), start_nodes), graph.num_nodes, **params)
        self._corpus_epoch = 0          # the epoch whose corpus the session holds
        try:
            if holdout_walks:
                r = graph.random_state
                seed = None if r is None else (int(r) - 1) & 0xFFFFFFFF   # (r = 0: 2^32 - 1)
                self.d_holdout = graph._session_walks(holdout_walks, walk_length, seed, start_nodes)
        except Exception:
            self.close()
            raise

    def _seed_of(self, epoch):
        r = self._graph.random_state
        return None if r is None else (int(r) + epoch) & 0xFFFFFFFF

    def run(self, epochs=1):
        st = self.state
        epochs = int(epochs)
        if epochs < 1 or st["sched_pos"] + epochs > st["sched_total"]:
            return super().run(epochs)   # (the parent's error: nothing is drawn and nothing trained)
        records = []
        for _ in range(epochs):
            epoch = self.state["epoch"]
            if self._fresh and epoch != self._corpus_epoch:
                self.set_walks(self._graph._session_walks(self._num_walks, self._walk_length, self._seed_of(epoch), self._start_nodes))
                self._corpus_epoch = epoch
            record = super().run(1)[0]
            if self.d_holdout is not None:
                held = self.evaluate(self.d_holdout, epoch=0)
                record["holdout_loss"], record["holdout_evaluations"] = held["loss"], held["evaluations"]
            records.append(record)
        return records

    def close(self):
        super().close()
        self.d_holdout = None


class WalkCorpus:
    """Re-iterable view of a walk index matrix as sentences of node IDs.

    ``simulate_walks`` has to materialise ``List[List[str]]`` (reference API, pecanpy.py:160); at
    RMAT-22 scale that is ~3.4 G Python objects.  ``WalkCorpus`` keeps the ``uint32[n_jobs, L+2]``
    matrix the GPU produced and maps rows to ID lists lazily, chunk by chunk, so gensim's
    ``Word2Vec(corpus)`` (which iterates the corpus once per epoch) can stream it
    (SURVEY.md section 8(f) rank 1).
    """

    def __init__(self, walk_idx_mat, node_ids, chunk=65536):
        self.matrix = walk_idx_mat
        self._ids = np.asarray(node_ids, dtype=object)
        self._chunk = int(chunk)

    def __len__(self):
        return int(self.matrix.shape[0])

    def __iter__(self):
        mat, ids = self.matrix, self._ids
        last = mat.shape[1] - 1
        for lo in range(0, mat.shape[0], self._chunk):
            block = mat[lo:lo + self._chunk]
            names = ids[block[:, :last]]           # vectorised index -> ID for the whole chunk
            for row, n in zip(names, block[:, last]):
                yield row[:n].tolist()

    def __getitem__(self, i):
        row = self.matrix[i]
        return self._ids[row[: row[-1]]].tolist()


class Base(BaseGraph):
    """Skeleton shared by all walk modes (reference ``Base``, pecanpy.py:27-290).

    Args mirror the reference: ``p`` return parameter, ``q`` in-out parameter, ``workers`` (used
    for Word2Vec only), ``verbose``, ``extend`` (node2vec+), ``gamma`` (noise-threshold factor),
    ``random_state`` (seed; ``None`` = entropy from the OS).
    """

    _mode = None  # name understood by the C ABI (pw_mode)
    _always_thresholds = False  # the mode's step uses the noise thresholds whatever `extend` says (node2vec++)

    def __init__(self, p=1, q=1, workers=1, verbose=False, extend=False, gamma=0, random_state=None):
        super().__init__()
        self.p = p
        self.q = q
        self.workers = workers
        self.verbose = verbose
        self.extend = extend
        self.gamma = gamma
        self.random_state = random_state
        self._preprocessed = False
        self._engine = None
        self._multi = None       # replicas on the other GPUs of this process (_multi_engine)
        self._engine_key = None
        self._thr_key = None
        self._run_seed = None
        self.device = None  # GPU index; None -> LOCAL_RANK / 0
        self.last_stats = None
        self.last_embed_stats = None
        self.last_corpus_stats = None   # walks_to_file: what the call did
        self.last_build_stats = None   # from_edge_index / from_tensor: what the device build of the graph did
        self.last_holdout_stats = None   # holdout_edges: the counts and stage times of the last split of this graph
        # the library's one-time start-up (~140 ms for the first stream it creates) runs on a helper thread beside what comes
        # next in the reference's flow -- reading the graph (cli.py:328-337) -- instead of in front of the first walk
        import os

        if os.environ.get("PECANPY_AMD_NO_WARMUP") is None:
            from . import _lib

            _lib.warmup_async(int(os.environ.get("LOCAL_RANK", "0")))

    # ---- engine plumbing -------------------------------------------------------------------
    def _device_index(self):
        if self.device is not None:
            return int(self.device)
        import os

        return int(os.environ.get("LOCAL_RANK", "0"))

    def _graph_key(self):
        raise NotImplementedError

    def _make_engine(self, device):
        raise NotImplementedError

    def _get_engine(self):
        key = (self._graph_key(), self._device_index())
        if self._engine is None or self._engine_key != key:
            if self._multi is not None:
                for rep in self._multi.engines[1:]:
                    rep.close()
                self._multi = None
            if self._engine is not None:
                self._engine.close()
            self._engine = self._make_engine(self._device_index())
            self._engine_key = key
            self._thr_key = None
        if (self.extend or self._always_thresholds) and self._thr_key != (self.gamma,):   # gamma may change between calls
            thr = self.get_noise_thresholds()
            self._engine.set_thresholds(thr)
            if self._multi is not None:
                for rep in self._multi.engines[1:]:
                    rep.set_thresholds(thr)
            self._thr_key = (self.gamma,)
        return self._engine

    #: nominal steps (jobs x walk_length) from which a call spreads over every visible GPU when PECANPY_AMD_DEVICES is unset
    MULTI_DEVICE_MIN_STEPS = 200_000_000

    def _multi_engine(self, n_jobs, walk_length):
        """In-process multi-GPU (round 6): replicas of the engine's graph on the other visible devices, driven by one host
        thread per device inside ONE C-ABI call (``pw_simulate_multi``) -- what the reference's single process with its Numba
        thread pool is on the CPU (cli.py:340-351).  ``PECANPY_AMD_DEVICES`` = ``all`` | a count | ``0,1,2`` | ``mask:0x0f``;
        unset: every visible GPU once the call is large enough to pay for the replication.  ``None``: one device."""
        import os

        if self._mode not in ("SparseOTF", "DenseOTF") or self.device is not None or "LOCAL_RANK" in os.environ:
            return None
        if self._engine is None or self._engine.kind != "csr":
            return None
        spec = os.environ.get("PECANPY_AMD_DEVICES")
        from .engine import MultiWalkEngine, visible_devices

        if spec is None:
            if n_jobs * walk_length < self.MULTI_DEVICE_MIN_STEPS:
                return None
            devices = visible_devices(None)
        else:
            devices = visible_devices(int(spec) if spec.strip().isdigit() else spec.strip())
        if len(devices) < 2:
            return None
        if devices[0] != self._engine.device:
            devices = [self._engine.device] + [d for d in devices if d != self._engine.device]
        if self._multi is None or self._multi.devices != devices:
            if self._multi is not None:
                for rep in self._multi.engines[1:]:
                    rep.close()
            self._multi = MultiWalkEngine.from_engine(self._engine, devices)
        return self._multi

    # ---- reference API ---------------------------------------------------------------------
    def _map_walk(self, walk_idx_ary):
        """Index row -> ID list; the last cell is the effective length (pecanpy.py:103-114)."""
        n = int(walk_idx_ary[-1])
        ids = self.nodes
        return [ids[i] for i in walk_idx_ary[:n].tolist()]

    @staticmethod
    def _dist():
        """``torch.distributed`` when this process is one rank of a multi-rank job, else ``None`` (torch is only
        needed for the multi-GPU path)."""
        try:
            import torch.distributed as dist
        except ImportError:
            return None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist
        return None

    def _call_seed(self):
        """Seed of this ``simulate_walks`` call.  ``random_state=None`` means entropy from the OS (reference:
        ``np.random.seed(None)``); across the ranks of a multi-GPU job that entropy must be the same, or every rank
        would shuffle -- and then shard -- a different job array: rank 0 draws it and broadcasts it."""
        if self.random_state is not None:
            return self.random_state
        dist = self._dist()
        if dist is None:
            return None
        box = [int(np.random.SeedSequence().generate_state(1)[0])]
        dist.broadcast_object_list(box, src=0)
        return box[0]

    def _indices_of(self, ids, what):
        """``uint32`` vertex indices of a sequence of node IDs (as in ``self.nodes``), in the order given; an empty
        sequence, an ID the graph does not have and a repeated ID are ``ValueError``s."""
        ids = list(ids)
        if not ids:
            raise ValueError(f"{what} is empty")
        idmap = self._node_idmap
        if len(idmap) != self.num_nodes:    # (ID lists installed without set_node_ids)
            idmap = dict(zip(self.nodes, range(self.num_nodes)))
        unknown = [i for i in ids if i not in idmap]
        if unknown:
            raise ValueError(f"{what}: {len(unknown)} IDs are not in the graph (first: {unknown[0]!r})")
        idx = np.fromiter((idmap[i] for i in ids), dtype=np.uint32, count=len(ids))
        if np.unique(idx).size != idx.size:
            raise ValueError(f"{what} names a vertex more than once")
        return idx

    def _start_array(self, num_walks, seed=None, start_idx=None):
        """Each node ``num_walks`` times, then NumPy's legacy seeded shuffle (pecanpy.py:135-141).  ``start_idx``: the
        same construction on a subset of the vertices -- its indices in the order given in place of ``0 .. N-1``."""
        nodes = np.arange(self.num_nodes, dtype=np.uint32) if start_idx is None else np.asarray(start_idx, dtype=np.uint32)
        starts = np.concatenate([nodes] * num_walks)
        np.random.seed(self.random_state if seed is None else seed)
        np.random.shuffle(starts)
        return starts

    def _starts_for(self, num_walks, start_nodes):
        """The job array of a call: every check of ``start_nodes`` comes before the seed is drawn or the device touched."""
        start_idx = None if start_nodes is None else self._indices_of(start_nodes, "start_nodes")
        self._preprocess_transition_probs()
        self._run_seed = self._call_seed()
        return self._start_array(num_walks, self._run_seed, start_idx)

    def simulate_walks_array(self, num_walks, walk_length, gather=True, start_nodes=None):
        """The walk index matrix ``uint32[n_jobs, walk_length + 2]`` (what ``_random_walks``
        returns in the reference); ``simulate_walks`` maps it to ID lists.  Under
        ``torch.distributed`` with ``gather=False`` every rank gets ``(rows, (lo, hi))``: its own
        slice [lo, hi) of that matrix, without the final collective.

        ``start_nodes``: a sequence of node IDs (as in ``self.nodes``) to walk from instead of every vertex.  The job array
        is the reference's construction on that subset -- its indices in the order given, ``num_walks`` times, the same
        seeded shuffle -- and the walks are what the engine draws for that array and seed (the reference's
        ``_random_walks`` takes any start array too).  An unknown, repeated or missing ID is a ``ValueError``."""
        starts = self._starts_for(num_walks, start_nodes)
        return self._random_walks(starts, walk_length, gather=gather)

    def simulate_walks_corpus(self, num_walks, walk_length, start_nodes=None):
        """Like ``simulate_walks`` but returns a lazy, re-iterable :class:`WalkCorpus`."""
        return WalkCorpus(self.simulate_walks_array(num_walks, walk_length, start_nodes=start_nodes), self.nodes)

    def simulate_walks(self, num_walks, walk_length, start_nodes=None):
        """Generate ``num_walks`` walks from every node (from every node of ``start_nodes`` when given, see
        ``simulate_walks_array``); returns ``List[List[str]]``."""
        mat = self.simulate_walks_array(num_walks, walk_length, start_nodes=start_nodes)
        return [self._map_walk(row) for row in mat]

    def _note_stats(self, stats):
        self.last_stats = stats
        if stats and stats.get("verify_mismatch", 0) > 0:
            import os
            import warnings

            if not os.environ.get("PECANPY_AMD_VERIFY_TIGHT"):
                warnings.warn(
                    f"{stats['verify_mismatch']} of {stats['verify_checked']} sampled interval decisions of the lane kernel disagreed "
                    "with the sequential float32 chain; the affected walks were generated again by the complete kernel.  This has "
                    "never been observed (DESIGN.md section 3) -- please report the graph and parameters.  "
                    "PECANPY_AMD_NO_LANES=1 avoids the lane kernel altogether.", RuntimeWarning, stacklevel=3)
        if stats and stats.get("stream_addressing") == 1:
            import warnings

            warnings.warn(
                "PECANPY_AMD_NOMINAL_STREAM is set: walks on this sink-heavy directed graph were generated with NOMINAL "
                "stream addressing (one fixed slot of walk_length draws per walk) after 32 re-addressing passes: "
                "reproducible under the seed, but not the reference's draw-for-draw assignment (unset it for the exact, "
                "block-wise repair; see DESIGN.md section 3)", RuntimeWarning, stacklevel=3)

    def _random_walks(self, starts, walk_length, gather=True):
        """GPU replacement of the reference's njit ``_random_walks`` (pecanpy.py:164-210)."""
        eng = self._get_engine()
        seed = self._run_seed if self.random_state is None else self.random_state
        if self._dist() is not None:
            if self._mode not in ("SparseOTF", "DenseOTF", "Node2vecPlusPlus", "SparseNode2vecPlusPlus"):
                raise NotImplementedError(
                    f"{self._mode} draws a variable number of random words per step; its seeded "
                    "stream cannot be sharded across GPUs -- run it in a single process")
            return self._random_walks_sharded(eng, starts, walk_length, seed, gather)
        multi = self._multi_engine(starts.size, walk_length)
        if multi is not None:
            eng = multi
        mat = eng.simulate(self._mode, self.p, self.q, self.extend, starts, walk_length, seed=seed)
        self._note_stats(eng.last_stats)
        return mat

    def _random_walks_sharded(self, eng, starts, walk_length, seed, gather=True):
        import torch
        import torch.distributed as dist

        from .sharding import sharded_walk_matrix, to_uint32_numpy

        dev = torch.device("cuda", eng.device)
        host_comm = dist.get_backend() == "gloo"  # gloo moves CPU tensors; nccl (= RCCL) device tensors

        def run_shard(sl, skip):
            d_starts = torch.from_numpy(np.ascontiguousarray(sl).view(np.int32)).to(dev)
            out = eng.simulate_device(self._mode, self.p, self.q, self.extend, d_starts,
                                      walk_length, seed=seed, stream_skip=skip)
            steps = eng.last_stats["total_steps"] if d_starts.numel() else 0
            if d_starts.numel() and eng.last_stats["stream_addressing"] == 1:
                # nominal slots: the shard owns walk_length draws per walk with neighbours, used or not
                steps = eng.count_stream_draws(sl, walk_length)
            return (out.cpu() if host_comm else out), steps

        full = sharded_walk_matrix(run_shard, lambda sl: eng.count_stream_draws(sl, walk_length),
                                   starts, walk_length, gather=gather)
        self._note_stats(eng.last_stats)
        if not gather:
            rows, bounds = full
            return to_uint32_numpy(rows), bounds
        return to_uint32_numpy(full)

    def get_move_forward(self):
        """``move_forward(cur_idx, prev_idx=None) -> next_idx`` of the on-the-fly modes (pecanpy.py:522-561, 576-614),
        evaluated on the GPU by the walk kernels' own step code (``pw_step``); the uniform draw comes from
        ``np.random.random()`` as in the reference.  One kernel launch per call: for API compatibility and
        inspection -- ``simulate_walks`` is the throughput path."""
        if self._mode not in ("SparseOTF", "DenseOTF", "Node2vecPlusPlus", "SparseNode2vecPlusPlus"):
            raise NotImplementedError(f"{self._mode}: single steps are provided for the on-the-fly modes")
        eng = self._get_engine()
        mode, p, q, extend = self._mode, self.p, self.q, self.extend

        def move_forward(cur_idx, prev_idx=None):
            return eng.step(mode, p, q, extend, cur_idx, prev_idx)

        return move_forward

    def setup_get_normalized_probs(self):
        """``(get_normalized_probs, noise_thresholds)`` as the reference returns them (pecanpy.py:212-229).  The
        callable keeps the reference's signature ``(data, indices, indptr, p, q, cur_idx, prev_idx=None,
        average_weight_ary=None)`` but computes on the GPU from the graph this object holds (``pw_probs``: the
        probabilities the walk kernels sample from, bit for bit)."""
        thr = self.get_noise_thresholds() if self.extend else None
        if self._mode == "DenseOTF":
            mode = "DenseOTF"
        else:
            mode = "SparseOTF"      # the alias modes precompute exactly these vectors (pecanpy.py:442-507)
        eng = self._get_engine()
        extend = self.extend

        def get_normalized_probs(data, indices, indptr, p, q, cur_idx, prev_idx=None, average_weight_ary=None):
            return eng.probs(mode, p, q, extend, cur_idx, prev_idx)

        return get_normalized_probs, thr

    def preprocess_transition_probs(self):
        """No-op for on-the-fly modes (pecanpy.py:231-233)."""

    def _preprocess_transition_probs(self):
        if not self._preprocessed:
            self.preprocess_transition_probs()
            self._preprocessed = True

    def _device_walks(self, num_walks, walk_length, start_nodes=None):
        """The walk matrix of ``simulate_walks_array`` as a device tensor (``WalkEngine.simulate_device``), or ``None`` where
        that call takes another route: under ``torch.distributed``, with the in-process multi-GPU engine, and for engines
        without a device entry."""
        starts = self._starts_for(num_walks, start_nodes)
        eng = self._get_engine()
        if self._dist() is not None or self._multi_engine(starts.size, walk_length) is not None or not hasattr(eng, "simulate_device"):
            return None
        import torch

        seed = self._run_seed if self.random_state is None else self.random_state
        d_starts = torch.from_numpy(starts.view(np.int32)).to(torch.device("cuda", eng.device))
        d_walks = eng.simulate_device(self._mode, self.p, self.q, self.extend, d_starts, walk_length, seed=seed)
        self._note_stats(eng.last_stats)
        return d_walks

    def _train_on_device(self, dim, num_walks, walk_length, window_size, epochs, workers):
        """Walks and trainer with the walk matrix in device memory: ``(d_vectors, walk_ms, sgns_call_ms)``, or ``None`` where
        ``_device_walks`` returns ``None``."""
        import time

        from .embed import train_sgns_device

        t0 = time.perf_counter()
        d_walks = self._device_walks(num_walks, walk_length)
        if d_walks is None:
            return None
        import torch

        torch.cuda.synchronize(d_walks.device)
        t1 = time.perf_counter()
        d_vec = train_sgns_device(d_walks, self.num_nodes, dim=dim, window=window_size, epochs=epochs, seed=self.random_state,
                                  workers=workers)
        t2 = time.perf_counter()
        return d_vec, (t1 - t0) * 1e3, (t2 - t1) * 1e3

    def _embed_through_host(self, t0, dim, num_walks, walk_length, window_size, epochs, workers):
        """The route of ``embed_array`` and ``embed_to_file`` once ``_train_on_device`` has returned ``None``:
        ``simulate_walks_array`` + ``train_sgns``, the walk matrix crossing to the host and back.  ``t0`` is when the caller
        began."""
        import time

        from .embed import train_sgns

        mat = self.simulate_walks_array(num_walks, walk_length)
        t1 = time.perf_counter()
        vec = train_sgns(mat, self.num_nodes, dim=dim, window=window_size, epochs=epochs, seed=self.random_state,
                         device=self._device_index(), workers=workers)
        t2 = time.perf_counter()
        self.last_embed_stats = {"walk_matrix_host_bytes": 2 * int(mat.nbytes), "walk_ms": (t1 - t0) * 1e3,
                                 "sgns_call_ms": (t2 - t1) * 1e3}
        return vec

    def embed_array(self, dim=128, num_walks=10, walk_length=80, window_size=10, epochs=1, workers=0):
        """Walks and skip-gram on the GPU, the walk matrix staying in device memory: start array -> ``simulate_device`` ->
        ``pecanpy_amd.embed.train_sgns_device`` -> ``float32[num_nodes, dim]`` in node order, copied to the host once.
        ``workers`` is the trainer's (0: hogwild, 1: one wavefront, deterministic under ``random_state``).

        ``self.last_embed_stats`` records the call: ``walk_matrix_host_bytes`` (0 on this route), ``walk_ms``, ``train_ms``
        (the training kernels), ``vocab_ms``, ``init_ms``, ``sgns_call_ms``, ``download_ms``, ``trained_pairs``,
        ``kept_occurrences``, ``wavefronts``.  Where the walks cannot stay on one device (see ``_device_walks``) the
        host-matrix route of ``simulate_walks_array`` + ``train_sgns`` runs instead and ``walk_matrix_host_bytes`` holds
        the bytes of the matrix that crossed to the host and back."""
        import time

        from .embed import train_sgns_device

        t0 = time.perf_counter()
        trained = self._train_on_device(dim, num_walks, walk_length, window_size, epochs, workers)
        if trained is None:
            return self._embed_through_host(t0, dim, num_walks, walk_length, window_size, epochs, workers)
        d_vec, walk_ms, sgns_call_ms = trained
        t2 = time.perf_counter()
        vec = d_vec.cpu().numpy()
        t3 = time.perf_counter()
        self.last_embed_stats = {"walk_matrix_host_bytes": 0, "walk_ms": walk_ms, "sgns_call_ms": sgns_call_ms,
                                 "download_ms": (t3 - t2) * 1e3, **train_sgns_device.last_stats}
        return vec

    def _session_walks(self, num_walks, walk_length, call_seed="own", start_nodes=None):
        """``_device_walks`` for a session, drawn with the call seed ``call_seed`` in place of ``random_state`` when one is
        given (``None``: a new OS seed); ``NotImplementedError`` where there is no device matrix."""
        saved = self.random_state
        if call_seed != "own":
            self.random_state = call_seed
        try:
            kw = {} if start_nodes is None else {"start_nodes": start_nodes}
            d_walks = self._device_walks(num_walks, walk_length, **kw)
        finally:
            self.random_state = saved
        if d_walks is None:
            raise NotImplementedError("embed_session needs the walk matrix on one device: not under torch.distributed or "
                                      "with the in-process multi-GPU engine")
        return d_walks

    def embed_session(self, dim=128, num_walks=10, walk_length=80, window_size=10, epochs=1, workers=0, compute_loss=False,
                      fresh_walks=False, holdout_walks=0):
        """The walks of ``embed_array`` generated in device memory and a ``pecanpy_amd.embed.SgnsSession`` on them, nothing
        trained yet: ``session.run()`` trains the schedule of ``epochs`` epochs in slices and reports every epoch (with
        ``compute_loss`` its loss), ``session.vectors()`` is ``float32[num_nodes, dim]`` in node order on the device.
        ``session.run(epochs)`` trains what ``embed_array`` trains.  Under ``torch.distributed`` and with the in-process
        multi-GPU engine there is no device matrix to hold a session on: ``NotImplementedError``.

        ``fresh_walks`` / ``holdout_walks``: the session is a ``GraphSgnsSession``, which knows this graph.  The corpus of
        epoch ``e`` is the walk matrix of this graph with call seed ``random_state + e`` (mod 2^32; ``random_state=None``: a
        new OS seed per epoch).  With ``fresh_walks`` every epoch after the first trains on its own corpus, drawn in device
        memory just before it (``set_walks``, the tables of the first corpus kept).  With ``holdout_walks = h > 0`` a
        matrix of ``h`` walks per node is drawn once, with call seed ``random_state - 1`` (2^32 - 1 for ``random_state=0``),
        and every epoch's record gains ``holdout_loss`` and ``holdout_evaluations``: ``evaluate`` on that matrix after the
        epoch, always with ``epoch=0`` -- the same evaluations every time, so the figures compare across epochs."""
        from .embed import SgnsSession

        params = dict(dim=dim, window=window_size, epochs=epochs, seed=self.random_state, workers=workers, compute_loss=compute_loss)
        if not fresh_walks and not holdout_walks:
            return SgnsSession(self._session_walks(num_walks, walk_length), self.num_nodes, **params)
        if int(holdout_walks) < 0:
            raise ValueError("holdout_walks must not be negative")
        return GraphSgnsSession(self, num_walks, walk_length, bool(fresh_walks), int(holdout_walks), **params)

    def extend_session(self, known_ids, vectors, context_vectors=None, starts="new", freeze=True, num_walks=10, walk_length=80,
                       window_size=10, epochs=1, workers=0, compute_loss=False, fresh_walks=False, holdout_walks=0):
        """Embed new vertices into old vectors: a ``GraphSgnsSession`` on this graph in which every vertex of ``known_ids``
        has its row of ``vectors`` (and, with ``context_vectors``, its row of ``syn1``) -- matched by ID; NumPy, a CPU tensor
        or a CUDA tensor, ``float32[len(known_ids), dim]``, ``dim`` taken from ``vectors`` -- and the other vertices the
        session's seeded initial ``syn0`` and a zero ``syn1``.  Nothing is trained yet; the other keywords are
        ``embed_session``'s.

        ``starts="new"``: the walks -- fresh and held-out ones too -- start from the vertices that are not in ``known_ids``,
        ``num_walks`` each; ``"all"``: from every vertex.  ``freeze=True``: the known rows of ``syn0`` are frozen
        (``SgnsSession.freeze``) and keep their bits however long the session trains; the known rows of ``syn1`` are frozen
        only when ``context_vectors`` was given -- without old context vectors there is nothing to preserve, and a zero row
        that cannot learn would teach the new vertices nothing.  The placement is a scatter on the device.

        The vocabulary tables -- word counts, the noise table negatives are drawn from, the keep probabilities of the
        subsampling -- come from the corpus the session is created on.  With ``starts="new"`` that is the neighbourhood of
        the new vertices, not the whole graph, deliberately: negatives are drawn from where the new vertices live.

        ``ValueError``: a known ID that is not in the graph, a repeated one, no new vertex with ``starts="new"``, a matrix
        of another shape or dtype.  ``NotImplementedError`` where ``embed_session`` raises one."""
        import torch

        if starts not in ("new", "all"):
            raise ValueError("starts must be 'new' or 'all'")
        if int(holdout_walks) < 0:
            raise ValueError("holdout_walks must not be negative")
        known = self._indices_of(known_ids, "known_ids")
        placed = []
        for name, m in (("vectors", vectors), ("context_vectors", context_vectors)):
            if m is None:
                placed.append(None)
                continue
            if not isinstance(m, torch.Tensor):
                m = torch.from_numpy(np.ascontiguousarray(m))
            if m.dtype != torch.float32 or m.dim() != 2 or m.shape[0] != known.size or m.shape[1] < 1:
                raise ValueError(f"{name} must be float32[{known.size}, dim], not {m.dtype}{list(m.shape)}")
            if placed and placed[0] is not None and m.shape[1] != placed[0].shape[1]:
                raise ValueError(f"context_vectors must have the dim of vectors ({placed[0].shape[1]}), not {m.shape[1]}")
            placed.append(m)
        if placed[0] is None:
            raise ValueError("vectors must be float32[len(known_ids), dim]")
        start_nodes = None
        if starts == "new":
            is_known = np.zeros(self.num_nodes, dtype=bool)
            is_known[known] = True
            ids = self.nodes
            start_nodes = [ids[i] for i in np.flatnonzero(~is_known).tolist()]
            if not start_nodes:
                raise ValueError("every vertex of the graph is in known_ids: there is no new vertex to walk from (starts='all'?)")
        s = GraphSgnsSession(self, num_walks, walk_length, bool(fresh_walks), int(holdout_walks), start_nodes=start_nodes,
                             dim=int(placed[0].shape[1]), window=window_size, epochs=epochs, seed=self.random_state, workers=workers,
                             compute_loss=compute_loss)
        try:
            dev = s.d_walks.device
            rows = torch.from_numpy(known.astype(np.int64)).to(dev)
            syn0 = s.vectors()
            syn0[rows] = placed[0].to(dev)
            syn1 = None
            if placed[1] is not None:
                syn1 = s.context_vectors()
                syn1[rows] = placed[1].to(dev)
            s.load(vectors=syn0, context_vectors=syn1)
            if freeze:
                s.freeze(rows, context=placed[1] is not None)
        except Exception:
            s.close()
            raise
        return s

    def extend_embedding(self, known_ids, vectors, context_vectors=None, starts="new", freeze=True, **kw):
        """``extend_session`` run through its whole schedule: ``float32[num_nodes, dim]`` in node order on the host, as
        ``embed_array`` returns it -- the rows of ``known_ids`` bitwise those of ``vectors`` when ``freeze`` is set."""
        with self.extend_session(known_ids, vectors, context_vectors=context_vectors, starts=starts, freeze=freeze, **kw) as s:
            s.run(s.state["sched_total"])
            return s.vectors().cpu().numpy()

    def embed_to_file(self, path, dim=128, num_walks=10, walk_length=80, window_size=10, epochs=1, workers=0):
        """``embed_array`` + ``save_word2vec_format`` without the vectors visiting the host: walks, trainer and the device
        writer (``pecanpy_amd.embed.save_word2vec_format_device``); only the text of the file leaves the device.  The file
        holds the bytes ``save_word2vec_format(path, self.nodes, self.embed_array(...))`` writes for the same vectors.

        ``self.last_embed_stats``: ``embed_array``'s keys without ``download_ms``, plus ``vectors_host_bytes`` (0 on this
        route), ``write_call_ms`` and the writer's ``format_ms``, ``copy_ms``, ``write_ms``, ``bytes``, ``chunks``.  Where
        the walks cannot stay on one device (see ``_device_walks``) ``embed_array`` + ``save_word2vec_format`` run instead
        and ``vectors_host_bytes`` holds the bytes of the matrix that came to the host."""
        import time

        from .embed import save_word2vec_format, save_word2vec_format_device, train_sgns_device

        t0 = time.perf_counter()
        trained = self._train_on_device(dim, num_walks, walk_length, window_size, epochs, workers)
        if trained is None:       # the route is decided once: what embed_array does from here on, not embed_array again
            vec = self._embed_through_host(t0, dim, num_walks, walk_length, window_size, epochs, workers)
            t0 = time.perf_counter()
            save_word2vec_format(path, self.nodes, vec)
            self.last_embed_stats = {**self.last_embed_stats, "vectors_host_bytes": int(vec.nbytes),
                                     "write_call_ms": (time.perf_counter() - t0) * 1e3}
            return
        d_vec, walk_ms, sgns_call_ms = trained
        trainer = train_sgns_device.last_stats
        t0 = time.perf_counter()
        save_word2vec_format_device(path, self.nodes, d_vec)
        self.last_embed_stats = {"walk_matrix_host_bytes": 0, "vectors_host_bytes": 0, "walk_ms": walk_ms,
                                 "sgns_call_ms": sgns_call_ms, "write_call_ms": (time.perf_counter() - t0) * 1e3, **trainer,
                                 **save_word2vec_format_device.last_stats}

    def walks_to_file(self, path, num_walks=10, walk_length=80, start_nodes=None):
        """The walks of ``simulate_walks(num_walks, walk_length, start_nodes)`` as a text file, one walk per line with the node IDs
        separated by single spaces (``pecanpy_amd.corpus``), without ``List[List[str]]``: ``_device_walks`` ->
        ``save_walks_device``; neither the walk matrix nor ID lists visit the host, only the text of the file leaves the
        device.  For a seeded object the file holds the bytes ``cli._dump_walks(path, self.simulate_walks(...))`` writes.

        ``self.last_corpus_stats``: ``walk_matrix_host_bytes`` (0 on this route), ``walk_ms``, ``write_call_ms`` and the
        writer's ``format_ms``, ``copy_ms``, ``write_ms``, ``bytes``, ``chunks``, ``rows``, ``tokens``.  Where the walks
        cannot stay on one device (see ``_device_walks``) ``simulate_walks_array`` + ``save_walks`` run instead and
        ``walk_matrix_host_bytes`` holds the bytes of the matrix that came to the host."""
        import time

        from .corpus import save_walks, save_walks_device

        t0 = time.perf_counter()
        d_walks = self._device_walks(num_walks, walk_length, start_nodes)
        if d_walks is None:
            mat = self.simulate_walks_array(num_walks, walk_length, start_nodes=start_nodes)
            t1 = time.perf_counter()
            save_walks(path, self.nodes, mat)
            self.last_corpus_stats = {"walk_matrix_host_bytes": int(mat.nbytes), "walk_ms": (t1 - t0) * 1e3,
                                      "write_call_ms": (time.perf_counter() - t1) * 1e3}
            return
        import torch

        torch.cuda.synchronize(d_walks.device)
        t1 = time.perf_counter()
        save_walks_device(path, self.nodes, d_walks)
        self.last_corpus_stats = {"walk_matrix_host_bytes": 0, "walk_ms": (t1 - t0) * 1e3,
                                  "write_call_ms": (time.perf_counter() - t1) * 1e3, **save_walks_device.last_stats}

    def sample_non_edges(self, m, seed, first_candidate=0):
        """``(u, v, candidates_used)``: ``m`` pairs of node indices that are neither a loop nor an edge of this graph, drawn
        on the GPU from ``seed``'s stream (``linkpred.sample_non_edges``; ``linkpred.sample_non_edges_host`` states the rule):
        negatives for link prediction.  Accepted pairs may repeat.  ``candidates_used`` added to ``first_candidate``
        continues the sequence in a later call.  Sparse classes only: a dense one raises ``NotImplementedError``."""
        if not isinstance(self, SparseGraph):
            raise NotImplementedError("sample_non_edges needs a sparse (CSR) graph")
        from . import linkpred

        return linkpred.sample_non_edges(self, m, seed, first_candidate)

    def holdout_edges(self, fraction, seed, directed=False, protect=True, first_word=0):
        """``(train_graph, (u, v, weight), words_used)``: a seeded split of this graph's edges on the GPU into a train graph --
        an object of this class with the same parameters, device and node IDs, its walk handle installed -- and the held-out
        pairs as tensors on the graph's device (``linkpred.holdout_edges``; ``linkpred.holdout_edges_host`` states the rule).
        With ``protect`` no vertex that had an edge loses all of them.  Negatives for the held-out pairs come from
        ``sample_non_edges`` of THIS graph, the original: the train graph's non-edges include the held-out edges.  Sparse
        classes only: a dense one raises ``NotImplementedError``."""
        if not isinstance(self, SparseGraph):
            raise NotImplementedError("holdout_edges needs a sparse (CSR) graph")
        from . import linkpred

        return linkpred.holdout_edges(self, fraction, seed, directed, protect, first_word)

    def neighbour_scores(self, u, v, kind, table=None):
        """The neighbourhood heuristic ``kind`` -- ``common_neighbours``, ``jaccard``, ``preferential_attachment``,
        ``adamic_adar``, ``resource_allocation``, or ``weighted`` with ``table=`` -- of every pair ``(u[i], v[i])`` of node
        indices, computed on the GPU: a float64 tensor on the graph's device, what ``linkpred.auc`` takes
        (``linkpred.neighbour_scores``; ``linkpred.neighbour_scores_host`` states the rule).  The baselines of link prediction:
        call it on the TRAIN graph of ``holdout_edges``.  Sparse classes only: a dense one raises ``NotImplementedError``."""
        if not isinstance(self, SparseGraph):
            raise NotImplementedError("neighbour_scores needs a sparse (CSR) graph")
        from . import linkpred

        return linkpred.neighbour_scores(self, u, v, kind, table=table)

    def embed(self, dim=128, num_walks=10, walk_length=80, window_size=10, epochs=1, verbose=False):
        """``simulate_walks`` + skip-gram (pecanpy.py:240-290): returns ``float32[num_nodes, dim]`` in node order.

        With gensim installed the reference's call is made (``Word2Vec(walks, sg=1, min_count=0, ...)``); without
        it the GPU pipeline of this package runs (``embed_array``: same model and defaults, the walk matrix stays in
        device memory, no string corpus)."""
        try:
            from gensim.models import Word2Vec
        except ImportError:
            Word2Vec = None
        if Word2Vec is None:
            return Timer("generate walks + train embeddings", verbose)(self.embed_array)(
                dim=dim, num_walks=num_walks, walk_length=walk_length, window_size=window_size, epochs=epochs)
        walks = Timer("generate walks", verbose)(self.simulate_walks)(num_walks, walk_length)
        w2v = Timer("train embeddings", verbose)(Word2Vec)(
            walks, vector_size=dim, window=window_size, sg=1, min_count=0, workers=self.workers,
            epochs=epochs, seed=self.random_state)
        return w2v.wv[self.nodes]


class _SparseBase(Base, SparseGraph):
    """CSR-backed modes (reference ``SparseRWGraph`` mixin, rw/sparse_rw.py:9-35)."""

    def __init__(self, *args, **kwargs):
        Base.__init__(self, *args, **kwargs)
        self.data = None
        self.indptr = None
        self.indices = None

    def _graph_key(self):
        return (id(self.indptr), id(self.indices), id(self.data))

    def _make_engine(self, device):
        return WalkEngine.from_csr(self.indptr, self.indices, self.data, device=device)

    @classmethod
    def from_edge_index(cls, edge_index, edge_weight=None, num_nodes=None, directed=False, node_ids=None, **kwargs):
        """Graph from an edge list held as arrays, the CSR built ON THE DEVICE (``pw_coo_to_csr_device``).

        ``edge_index``: integer ``[2, m]`` torch tensor (a CUDA tensor is used where it is; a CPU tensor or a NumPy
        array is uploaded first and takes the same path); ``edge_weight``: float ``[m]`` or ``None`` (unweighted);
        ``num_nodes``: ``None`` = largest id listed + 1; ``node_ids``: as in ``from_csr``; ``kwargs``: the constructor's.

        Vertex ``i`` IS id ``i``: there is no renumbering by first appearance, which is how ``read_edg`` numbers the
        vertices of an edge-list file.  Otherwise the semantics are the reference's ``AdjlstGraph.add_edge`` /
        ``to_csr`` (graph.py:238-268, 323-341): an edge with a non-positive weight is dropped (one ``RuntimeWarning``
        with the count), every kept edge is inserted in both directions unless ``directed``, the last insertion of an
        ordered pair wins, rows come out ascending.  NaN or infinite weights and ids outside ``[0, num_nodes)`` raise.

        The object's host ``indptr`` / ``indices`` / ``data`` are filled from the device CSR (``data`` all ones when
        unweighted, as ``from_csr`` does) and the walk handle created from it is installed as the object's engine: the
        first ``simulate_walks`` / ``embed_array`` does not upload the graph again.  ``last_build_stats`` records the
        call (``edge_list_host_bytes``: 0 for a CUDA ``edge_index``; sizes, ``dropped``, ``build_ms``, stage times)."""
        from .engine import check_edge_index

        check_edge_index(edge_index, edge_weight, num_nodes)   # ValueError before the library or a device is touched
        g = cls(**kwargs)
        device = edge_index.device.index if getattr(edge_index, "is_cuda", False) else g._device_index()
        eng = WalkEngine.from_edge_index(edge_index, edge_weight, num_nodes=num_nodes, directed=directed, device=device)
        try:
            if node_ids is not None and len(node_ids) != eng.n_nodes:
                raise ValueError(f"node_ids has {len(node_ids)} entries, the graph has {eng.n_nodes} vertices")
        except Exception:
            eng.close()
            raise
        if device != g._device_index():
            g.device = device   # (a CUDA edge_index decides where the graph lives)
        g.indptr, g.indices, g.data = eng.csr
        g.set_node_ids(node_ids, implicit_ids=node_ids is None, num_nodes=eng.n_nodes)
        g._engine = eng
        g._engine_key = (g._graph_key(), g._device_index())
        g.last_build_stats = dict(eng.build_stats)
        if eng.build_stats["dropped"]:
            import warnings

            warnings.warn(f"{eng.build_stats['dropped']} non-positive edge(s) ignored", RuntimeWarning, stacklevel=2)
        return g

    def read_edg_device(self, path, weighted, directed, delimiter="\t"):
        """``read_edg`` with the file parsed ON THE DEVICE (``WalkEngine.from_edgelist_file``): the text is uploaded,
        tokenised, numbered by first appearance and turned into the CSR in device memory.  ``nodes``, ``indptr``,
        ``indices`` and ``data`` (all ones when unweighted) come out as ``read_edg`` fills them, bit for bit, and the walk
        handle created from the device CSR is installed as the object's engine: the first ``simulate_walks`` /
        ``embed_array`` uploads nothing.

        The device reader takes a subset of the files the native host reader takes; for everything else -- whatever makes
        the reference warn or raise, weight literals it does not parse exactly, a file that cannot be opened, no GPU or no
        library -- this method calls ``read_edg``, so warnings and exceptions are the reference's in every case.
        ``last_build_stats["reader"]`` says which ran: ``"device"`` (with the stage times and sizes of
        ``from_edgelist_file``) or ``"host"``."""
        from . import _lib

        try:   # without the library or a GPU there is nothing to read on: the host reader needs neither (the walks will say so)
            have_device = int(_lib.load().pw_device_count()) > 0
        except (_lib.PwError, OSError, AttributeError):
            have_device = False
        eng = None
        if have_device:   # (a device error in the reader itself is raised, not papered over)
            eng = WalkEngine.from_edgelist_file(path, weighted, directed, delimiter, device=self._device_index())
        if eng is None:
            self.read_edg(path, weighted, directed, delimiter)
            self.last_build_stats = {"reader": "host"}
            return
        if self._multi is not None:
            for rep in self._multi.engines[1:]:
                rep.close()
            self._multi = None
        if self._engine is not None:
            self._engine.close()
        self.set_node_ids(eng.ids)
        self.indptr, self.indices, self.data = eng.csr
        self._engine = eng
        self._engine_key = (self._graph_key(), self._device_index())
        self._thr_key = None
        self.last_build_stats = {"reader": "device", **eng.build_stats}

    def get_has_nbrs(self):
        """``has_nbrs(idx)`` callback (sparse_rw.py:12-20); host-side helper, not used by the GPU path."""
        indptr = self.indptr
        return lambda idx: indptr[idx] != indptr[idx + 1]

    def get_noise_thresholds(self):
        """Per-node noisy-edge threshold ``max(mean + gamma * std, 0)`` (sparse_rw.py:22-35), bit for bit
        what the reference's row-by-row NumPy expression gives: evaluated by the native restatement of
        NumPy's pairwise reductions (``pw_noise_thresholds_csr``), by the NumPy loop itself when the
        library is not built."""
        data = np.ascontiguousarray(self.data, dtype=np.float32)
        indptr = np.ascontiguousarray(self.indptr, dtype=np.uint32)
        n = self.num_nodes
        thr = np.zeros(n, dtype=np.float32)
        try:
            from . import _lib

            lib = _lib.load()
        except Exception:  # library not built
            lib = None
        if lib is not None:
            # the promotion rule of the installed NumPy (NEP 50 from 2.0 on), so that the native path equals the
            # row-by-row NumPy expression below in the same environment
            fn = lib.pw_noise_thresholds_csr if int(np.__version__.split(".")[0]) >= 2 else lib.pw_noise_thresholds_csr_numpy1
            _lib.check(fn(indptr.ctypes.data, data.ctypes.data, n, float(self.gamma), thr.ctypes.data))
            return thr
        for i in range(n):
            row = data[indptr[i]:indptr[i + 1]]
            thr[i] = row.mean() + self.gamma * row.std()
        return np.maximum(thr, 0)


class SparseOTF(_SparseBase):
    """Sparse graph, transition probabilities on the fly (reference pecanpy.py:510-561)."""

    _mode = "SparseOTF"


class FirstOrderUnweighted(_SparseBase):
    """Uniform neighbour pick, p = q = 1, unweighted (reference pecanpy.py:293-309)."""

    _mode = "FirstOrderUnweighted"


class PreCompFirstOrder(_SparseBase):
    """First-order alias tables (reference pecanpy.py:312-361)."""

    _mode = "PreCompFirstOrder"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.alias_j = self.alias_q = None

    def preprocess_transition_probs(self):
        """Build the per-node alias tables on the GPU (reference pecanpy.py:336-361)."""
        eng = self._get_engine()
        eng.precomp_build(1, 1, False, True)
        _, self.alias_j, self.alias_q = eng.precomp_export(True)


class PreComp(_SparseBase):
    """Second-order alias tables (reference pecanpy.py:364-507)."""

    _mode = "PreComp"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.alias_dim = None
        self.alias_j = None
        self.alias_q = None
        self.alias_indptr = None

    def preprocess_transition_probs(self):
        """Build the sum(deg^2) second-order alias tables on the GPU (reference pecanpy.py:442-507)
        and mirror them into ``alias_dim / alias_indptr / alias_j / alias_q``."""
        eng = self._get_engine()
        eng.precomp_build(self.p, self.q, self.extend, False)
        self.alias_indptr, self.alias_j, self.alias_q = eng.precomp_export(False)
        self.alias_dim = self.indptr[1:] - self.indptr[:-1]


class _DenseBase(Base, DenseGraph):
    """Dense-matrix-backed modes (reference ``DenseRWGraph`` mixin, rw/dense_rw.py:8-31)."""

    def __init__(self, *args, **kwargs):
        Base.__init__(self, *args, **kwargs)
        self._data = None
        self._nonzero = None
        self._device_built = None   # from_tensor / from_edge_index: token of the graph the installed engine was built from

    def _graph_key(self):
        if self._device_built is not None:   # (survives the lazy fill of `data`: the engine keeps walking)
            return ("device-built", id(self._device_built))
        return (id(self._data),)

    def _make_engine(self, device):
        return WalkEngine.from_dense(self.data, device=device)

    def _get_engine(self):
        if (self._device_built is not None and self._data is None and self._engine is not None
                and self._engine_key != (self._graph_key(), self._device_index())):
            self._materialize()   # the object moves to another device: the matrix comes down before its engine goes
        return super()._get_engine()

    # ---- graphs built on the device: the host matrix is filled on first read -------------------------------------------
    def _materialize(self):
        """``data`` / ``nonzero`` of an object made by ``from_tensor`` / ``from_edge_index``, rebuilt on the host from the
        handle's compressed rows (``WalkEngine.dense_arrays``): the values the reference's attributes would hold."""
        if self._data is not None or self._device_built is None or self._engine is None:
            return
        a = self._engine.dense_arrays()
        n = self._engine.n_nodes
        rows = np.repeat(np.arange(n), np.diff(a["indptr"].astype(np.int64)))
        mat = np.zeros((n, n))
        mat[rows, a["indices"]] = a["data"]
        nonzero = np.zeros((n, n), dtype=bool)
        nonzero[rows, a["indices"]] = True
        self._data, self._nonzero = mat, nonzero

    @property
    def data(self):
        self._materialize()
        return self._data

    @data.setter
    def data(self, data):
        self._device_built = None   # a matrix assigned by the caller replaces a graph built on the device
        DenseGraph.data.fset(self, data)

    @property
    def nonzero(self):
        self._materialize()
        return self._nonzero

    @property
    def num_edges(self):
        """``nonzero.sum()`` (graph.py:524-528).  While the graph is built on the device and its host matrix has not been
        read, the same count comes from the handle (``pw_dense_shape``) and no ``N * N`` array is made for it -- ``density``,
        and thereby ``check_mode``, goes through here."""
        if self._device_built is not None and self._data is None and self._engine is not None:
            return np.int64(self._engine._dense_shape()["nnz"])
        return DenseGraph.num_edges.fget(self)

    def _install_device_engine(self, eng, device, node_ids):
        try:
            if node_ids is not None and len(node_ids) != eng.n_nodes:
                raise ValueError(f"node_ids has {len(node_ids)} entries, the graph has {eng.n_nodes} vertices")
        except Exception:
            eng.close()
            raise
        if device != self._device_index():
            self.device = device   # (a CUDA input decides where the graph lives)
        self.set_node_ids(node_ids, implicit_ids=node_ids is None, num_nodes=eng.n_nodes)
        self._data = self._nonzero = None
        self._device_built = object()
        self._engine = eng
        self._engine_key = (self._graph_key(), self._device_index())
        self.last_build_stats = dict(eng.build_stats)

    @classmethod
    def from_tensor(cls, adj, node_ids=None, **kwargs):
        """Graph from a dense adjacency matrix, the walk handle built ON THE DEVICE (``pw_dense_create_device``).

        ``adj``: square 2-d torch tensor or NumPy array (float64 / float32 as they are, other real dtypes converted to
        float64).  A CUDA tensor is used where it is and decides the device; a CPU tensor or a NumPy array is uploaded
        first and takes the same path.  ``node_ids``: as in ``from_mat`` (``None``: ``"0" .. "N-1"``); ``kwargs``: the
        constructor's.

        The handle is installed as the object's engine and equals the one ``from_mat`` would create from the same values,
        so the walks are the same.  The object keeps no reference to ``adj`` and does not download the matrix: ``data`` and
        ``nonzero`` are rebuilt on the host from the handle's compressed rows when they are first read, and until then
        ``get_noise_thresholds`` computes on the device (``pw_dense_noise_thresholds``).  ``last_build_stats`` records the
        call (``matrix_host_bytes``: 0 for a CUDA tensor; ``n_nodes``, ``nnz``, ``unit``, ``build_ms``, stage times)."""
        from .engine import check_dense_matrix

        check_dense_matrix(adj)   # ValueError before the library or a device is touched
        g = cls(**kwargs)
        device = adj.device.index if getattr(adj, "is_cuda", False) else g._device_index()
        g._install_device_engine(WalkEngine.from_dense_tensor(adj, device=device), device, node_ids)
        return g

    @classmethod
    def from_edge_index(cls, edge_index, edge_weight=None, num_nodes=None, directed=False, node_ids=None, **kwargs):
        """Dense graph from an edge list held as arrays, built ON THE DEVICE (``pw_coo_to_csr_device``, then
        ``pw_dense_create_from_csr``).  Arguments, checks and the warning for dropped edges are those of the sparse classes'
        ``from_edge_index``; ``last_build_stats`` has the same keys.

        Semantics: the reference's ``AdjlstGraph.add_edge`` + ``to_dense()`` (graph.py:238-268, 343-362) with vertex ``i``
        = id ``i``: non-positive weights dropped, the reverse edge inserted unless ``directed``, the last insertion of an
        ordered pair wins.  Weights are taken as float32, as the sparse route takes them: the matrix this object stands for
        holds those float32 values widened to float64 (an edge-list FILE read by ``read_edg`` keeps its float64 literals).
        ``data`` / ``nonzero`` are filled on first read, as after ``from_tensor``."""
        from .engine import check_edge_index

        check_edge_index(edge_index, edge_weight, num_nodes)   # ValueError before the library or a device is touched
        g = cls(**kwargs)
        device = edge_index.device.index if getattr(edge_index, "is_cuda", False) else g._device_index()
        eng = WalkEngine.dense_from_edge_index(edge_index, edge_weight, num_nodes=num_nodes, directed=directed, device=device)
        g._install_device_engine(eng, device, node_ids)
        if eng.build_stats["dropped"]:
            import warnings

            warnings.warn(f"{eng.build_stats['dropped']} non-positive edge(s) ignored", RuntimeWarning, stacklevel=2)
        return g

    def read_edg_device(self, path, weighted, directed, delimiter="\t"):
        """``read_edg`` with the file parsed and the dense handle built ON THE DEVICE
        (``WalkEngine.dense_from_edgelist_file``): the text is uploaded, tokenised, numbered by first appearance and sorted
        in device memory as for the sparse classes, the CSR keeps the float64 weights as parsed, and
        ``pw_dense_create_from_csr`` makes the handle of the matrix ``read_edg`` would assign to ``data`` -- float64
        literals, not their float32 roundings.  No ``N * N`` host array is made: ``nodes`` are set from the reader's names,
        the handle is installed as the object's engine, ``data`` / ``nonzero`` are filled on first read as after
        ``from_tensor``, ``num_edges`` / ``density`` come from the handle and ``get_noise_thresholds`` computes on the device.

        The contract is the sparse method's: for every file the device reader declines, without a GPU and without the
        library this method calls ``read_edg``, so warnings and exceptions are the reference's in every case.
        ``last_build_stats["reader"]`` says which ran: ``"device"`` (with the keys of ``dense_from_edgelist_file``) or
        ``"host"``."""
        from . import _lib

        try:   # without the library or a GPU there is nothing to read on: the host reader needs neither (the walks will say so)
            have_device = int(_lib.load().pw_device_count()) > 0
        except (_lib.PwError, OSError, AttributeError):
            have_device = False
        eng = None
        if have_device:   # (a device error in the reader itself is raised, not papered over)
            eng = WalkEngine.dense_from_edgelist_file(path, weighted, directed, delimiter, device=self._device_index())
        if eng is None:
            self.read_edg(path, weighted, directed, delimiter)
            self.last_build_stats = {"reader": "host"}
            return
        if self._multi is not None:
            for rep in self._multi.engines[1:]:
                rep.close()
            self._multi = None
        if self._engine is not None:
            self._engine.close()
        self._install_device_engine(eng, self._device_index(), eng.ids)
        self._thr_key = None
        self.last_build_stats = {"reader": "device", **eng.build_stats}

    def get_has_nbrs(self):
        nonzero = self.nonzero
        return lambda idx: bool(nonzero[idx].any())

    def get_noise_thresholds(self):
        """Dense variant (rw/dense_rw.py:11-19): float64 rows, non-zero entries only; native restatement
        of NumPy's reductions (``pw_noise_thresholds_dense``) with the NumPy loop as fallback.  For a graph built on the
        device whose host matrix has not been read yet the same values come from the handle's compressed rows
        (``pw_dense_noise_thresholds``)."""
        if self._device_built is not None and self._data is None and self._engine is not None:
            return self._engine.compute_thresholds(self.gamma)
        n = self.num_nodes
        thr = np.zeros(n, dtype=np.float32)
        try:
            from . import _lib

            lib = _lib.load()
        except Exception:  # library not built
            lib = None
        if lib is not None:
            mat = np.ascontiguousarray(self.data, dtype=np.float64)
            _lib.check(lib.pw_noise_thresholds_dense(mat.ctypes.data, n, float(self.gamma), thr.ctypes.data))
            return thr
        for i in range(n):
            w = self.data[i, self.nonzero[i]]
            thr[i] = w.mean() + self.gamma * w.std()
        return np.maximum(thr, 0)


class DenseOTF(_DenseBase):
    """Dense graph, transition probabilities on the fly (reference pecanpy.py:564-614)."""

    _mode = "DenseOTF"
