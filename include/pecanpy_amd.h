/*
 * pecanpy_amd.h -- C ABI of the MI355X-native node2vec walk engine (libpecanpy_amd.so).
 *
 * The reference (krishnanlab/PecanPy) has no FFI: its operator boundary for walk generation is
 * the njit function
 *     Base._random_walks(tot_num_jobs, walk_length, random_state, start_node_idx_ary,
 *                        has_nbrs, move_forward, progress_proxy) -> uint32[tot_num_jobs, L+2]
 * (reference src/pecanpy/pecanpy.py:164-210) whose callbacks are built from the graph arrays by
 * get_has_nbrs()/get_move_forward() (pecanpy.py:522-561, 576-614; rw/sparse_rw.py:12-20).
 * The entry points below are what a ctypes/cffi binding of that boundary binds to: the graph
 * arrays become a device-resident handle (pw_csr_create / pw_dense_create), and one call
 * (pw_simulate*) replaces _random_walks + the two callbacks.  Plain pointers and sizes only.
 *
 * Conventions
 *   - every function returns 0 on success, a negative pw_status on failure; pw_last_error()
 *     returns a thread-local human-readable message.  Nothing prints or aborts.
 *   - host buffers are borrowed for the duration of a call; device copies of the graph are owned
 *     by the handle until pw_graph_destroy().
 *   - one in-flight pw_simulate* per handle.
 *   - walk matrix layout = the reference's: row i = [start, n_1 .. n_L, len_i], unused cells 0,
 *     len_i = L+1 normally, 1 for a start without neighbours, j for a dead end before step j
 *     (pecanpy.py:182-206).
 *   - random stream = ONE MT19937 stream seeded like the reference (np.random.seed(random_state)
 *     inside _random_walks, pecanpy.py:177-178); walk i step j consumes double #(S_i + j),
 *     S_i = sum of (len-1) over earlier walks.  stream_skip shifts S_0 (multi-GPU shards).
 */
#ifndef PECANPY_AMD_H
#define PECANPY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pw_graph pw_graph; /* opaque, device resident */

typedef enum {
    PW_OK = 0,
    PW_ERR_INVALID = -1,     /* bad argument */
    PW_ERR_HIP = -2,         /* HIP runtime error (message has the hipError string) */
    PW_ERR_NO_DEVICE = -3,   /* no usable GPU */
    PW_ERR_UNSUPPORTED = -4, /* mode/option not available for this graph kind */
    PW_ERR_NOMEM = -5
} pw_status;

/* walk modes = the reference's mode classes (pecanpy.py:293-614) */
typedef enum {
    PW_MODE_SPARSE_OTF = 0,            /* SparseOTF.move_forward, pecanpy.py:543-559 */
    PW_MODE_DENSE_OTF = 1,             /* DenseOTF.move_forward,  pecanpy.py:597-612 */
    PW_MODE_PRECOMP = 2,               /* PreComp.move_forward,   pecanpy.py:409-438 */
    PW_MODE_FIRST_ORDER_UNWEIGHTED = 3,/* FirstOrderUnweighted,   pecanpy.py:299-309 */
    PW_MODE_PRECOMP_FIRST_ORDER = 4,   /* PreCompFirstOrder,      pecanpy.py:319-334 */
    PW_MODE_NODE2VEC_PLUSPLUS = 5,     /* experimental.Node2vecPlusPlus, experimental.py:31-102 (see below) */
    PW_MODE_SPARSE_NODE2VEC_PLUSPLUS = 6 /* experimental.SparseNode2vecPlusPlus: node2vec++ on CSR handles (see below) */
} pw_mode;

/* PW_MODE_NODE2VEC_PLUSPLUS: node2vec++, the reference's continuous form of node2vec+, on dense handles.  A column x of cur's
 * row with data[prev, x] < thr[x], x != prev, is weighted by ((t * b) / (1 + (b - 1))) * |1 - 1/q| + min(1, 1/q), with
 * t = data[prev, x] / thr[x] (1 - t when q < 1) and b = data[cur, x] / thr[x]; prev's weight is divided by p; the first step is
 * unbiased.  Like DenseOTF it draws one double per step (stream_skip, shards and pw_count_stream_draws apply unchanged).
 *   - the thresholds of pw_graph_set_thresholds() are always used (extend is ignored); without them: PW_ERR_INVALID.
 *   - PW_ERR_UNSUPPORTED for CSR handles, pw_dense_create_bits handles and matrices with negative or non-finite weights.
 *   - legal weights can make the reference's probabilities NaN (b < 2^-54 and q > 1) or inf / NaN (q < 1); the step then
 *     follows NumPy's searchsorted (the first k with !(cdf[k] < r)); a draw no partial sum reaches takes the last neighbour
 *     and counts as an overflow + clamped read.  pw_stats.ambiguous_steps counts the steps the reference's loops decided. */

/* PW_MODE_SPARSE_NODE2VEC_PLUSPLUS: node2vec++ on CSR handles.  Walks, steps and probabilities equal mode 5 on the dense
 * float64 form of the graph (A.toarray().astype(np.float64)), bit for bit, for any number of nodes; no row length limit.
 *   - the thresholds must be the DENSE formula's (pw_noise_thresholds_csr_f64); without any: PW_ERR_INVALID.
 *   - PW_ERR_UNSUPPORTED for dense handles and for CSR handles with a stored weight of 0 (the dense form has no such entry).
 *   - pw_probs writes float64[degree(cur)]; one double per step, so stream_skip, shards and pw_count_stream_draws apply. */

typedef struct {
    uint64_t total_steps;     /* sampled transitions = sum_i (len_i - 1) */
    uint64_t overflow_reads;  /* steps where the float CDF never reached r (choice == degree,
                                 SURVEY.md App. D quirk 1; mirrored from the reference) */
    uint64_t clamped_reads;   /* of those, reads that would have left the index buffer */
    uint64_t dead_end_walks;  /* walks that stopped early at a vertex without out-edges */
    uint64_t repair_rounds;   /* extra passes needed to re-address the stream after dead ends */
    double walk_kernel_ms;    /* HIP-event time of the walk kernel launches of this call */
    double rng_kernel_ms;     /* HIP-event time of the MT19937 expansion kernels */
    uint32_t walk_kernel_launches;
    uint32_t stream_addressing; /* 0: the reference's exact draw assignment (also on sink-heavy directed graphs: block-wise
                                   repair); 1: nominal per-walk slots -- only with the explicit opt-in
                                   PECANPY_AMD_NOMINAL_STREAM=1 in the environment, after 32 re-addressing passes */
    /* lane kernel (one walk per lane, csrc/walk_lanes.hip.h): unit-weight CSR graphs, 1/p and 1/q powers of two */
    uint32_t lane_kernel;       /* 1: the call ran on the lane kernel; 2: on its float-chain form (1/p or 1/q not a power of two);
                                   3: on its weighted form (weighted CSR graphs: float64-bounded decision, eager_steps = the steps
                                   the wave-per-walk scan decided) */
    uint32_t lane_rounds;       /* lane kernel launches of the call: walks whose step needs the float32 chain are parked,
                                   the chains of a whole queue run in one launch, the next round resumes the walks */
    uint64_t redo_walks;        /* walks a fast kernel handed to the complete one: lane kernel -> wave-per-walk kernel
                                   (tie budget, rows outside the exact range, overflow reads without a line), register-only
                                   dense kernel -> column-space kernel with the float64 chain (undecided steps) */
    uint64_t list_entries_read; /* common-neighbour list entries the lane kernel read (uint16 positions: 2 bytes each; uint32 for
                                   rows of more than 65536 entries) */
    uint64_t ambiguous_steps;   /* steps the a-priori rounding bound left open (settled by the interval decision or the chain) */
    double lane_kernel_ms;      /* HIP-event time of the lane kernel launches alone */
    uint64_t wave_chain_steps;  /* of the ambiguous steps, those that needed the float32 chain itself */
    double param_index_ms;      /* device time spent in THIS call building an index that depends on (p, q, extend):
                                   per-edge normalisers of weighted graphs, hint tables; 0 when cached in the handle */
    /* PECANPY_AMD_VERIFY_TIGHT=1 (test mode of the lane kernel): every step the interval decision settled is decided
     * again by the sequential float32 chain on the device */
    uint64_t verify_checked;    /* steps re-decided */
    uint64_t verify_mismatch;   /* of those, steps where the chain picked a different neighbour (must be 0) */
    uint64_t verify_dropped;    /* steps not recorded because the record buffer was full */
    uint64_t verify_ties;       /* steps the chain declined (rounding-tie budget): not compared */
    /* partial lane index (the byte budget left the longest common-neighbour lists out, see pw_csr_create) */
    uint64_t eager_steps;       /* lane-kernel steps that arrived by an entry without a stored list: decided by one wavefront each
                                   (lanes_eager_kernel: membership searched), the walk resumed in the lane kernel */
    uint32_t index_max_list;    /* longest list the index stores beyond the edge lines (0xffffffff: all of them; 0: no lane index) */
    uint32_t reserved0;
} pw_stats;

/* ---- introspection ------------------------------------------------------------------- */
const char *pw_version(void);
const char *pw_last_error(void);
int pw_device_count(void);
/* One-time start-up of this library on `device` (the first stream a process creates through the library costs ~140 ms on an
 * MI355X box -- code objects, queues -- whatever torch or another library has initialised before): a caller with host work in front
 * of its first handle (reading an edge list: cli.py:328-337, graph.py:270-341) runs this on a helper thread beside that work and
 * pw_csr_create / pw_dense_create find the runtime warm.  *ms (optional) receives the wall clock of the call.  No reference
 * counterpart (Numba's JIT compilation at the first call is the reference's start-up cost, pecanpy.py:164). */
int pw_warmup(int device, double *ms);

/* ---- graph handles --------------------------------------------------------------------- */
/* CSR in the reference's SparseGraph layout (graph.py:409-413): indptr uint32[n_nodes+1],
 * indices uint32[nnz] ascending and duplicate-free per row, data float32[nnz].
 * data may be NULL: all weights 1.0 (the reference's unweighted graphs, graph.py:170,480).
 * Besides the three arrays the handle owns the membership index built here on the device (per-row
 * Bloom filters, adjacency hash index, key stream, vertex records and the lane index: one 64-byte edge line per CSR entry
 * with the common-neighbour list of the edge, longer lists in an overflow array; weighted graphs WITH self loops get
 * none): about 180 bytes per CSR entry at RMAT-22.
 * Limits: the 32-bit offsets of the index allow about 2^33 hash slots, i.e. graphs up to ~2 * 10^9 CSR
 * entries (PW_ERR_INVALID "graph too large" beyond that; the reference's own limit is nnz < 2^32).
 * Environment: PECANPY_AMD_NO_LAZY=1 skips the per-edge records (every step then takes the eager path;
 * used by the test-suite to cross-check the two step implementations).  PECANPY_AMD_INDEX_BUDGET=<bytes> bounds the
 * overflow array of the common-neighbour lists (default: half of the free device memory): beyond it the index is
 * PARTIAL -- edge lines always, the longest lists left out -- and steps that arrive by an entry without its list are
 * decided by one wavefront each (pw_stats.eager_steps) while the walk stays in the lane kernel. */
int pw_csr_create(const uint32_t *indptr, const uint32_t *indices, const float *data,
                  uint32_t n_nodes, uint32_t nnz, int device, pw_graph **out);

/* ---- CSR built on the device from an edge list (COO) that is already in device memory ------------------------------------
 * The sparse counterpart of pw_dense_create_bits(on_device = 1): a caller that holds a graph as edge arrays on the GPU (a
 * PyTorch edge_index, a COO buffer) gets the reference's CSR without sorting, symmetrising and deduplicating on the host.
 * Semantics = AdjlstGraph.add_edge / to_csr of the reference (graph.py:238-268, 323-341) with IMPLICIT INTEGER IDS: vertex i
 * is id i -- no renumbering by first appearance, unlike pw_edgelist_read.
 *   d_src, d_dst  int64[m] on `device` (two pointers: the rows of a [2, m] tensor work without a copy)
 *   d_weight      float32[m] on `device`, or NULL: unweighted (the result then has no data array: the unit-weight case of
 *                 pw_csr_create's data == NULL)
 *   n_nodes       0: largest id listed + 1 (edges that are dropped count too)
 *   - an edge with weight <= 0 is dropped and counted (the reference's "Non-positive edge ignored");
 *   - kept edge i inserts (src, dst) and, when directed == 0, then (dst, src) with the same weight; insertion order is edge
 *     order, forward before reverse; for every ordered pair the LAST insertion's weight wins;
 *   - rows ascending and duplicate-free; vertices without a kept edge are empty rows;
 *   - PW_ERR_INVALID, nothing kept allocated: a NaN or infinite weight (pw_csr_create's rule), a negative id, an id >= n_nodes,
 *     n_nodes > 2^32 - 2, or 2^32 or more insertions; PW_ERR_NOMEM with the sizes in the message when the scratch (two
 *     key arrays of 8 bytes and, with weights, two of 4 bytes per insertion, 1/8 of that again for histograms) does not fit.
 * The result is a function of the input alone (a stable radix sort on (src, dst) keeps equal pairs in insertion order; no
 * result depends on the order atomics arrive in).  Work runs on the device's default stream; the call returns when it is done.
 *   pw_csr_dev_shape    n_nodes, nnz, insertions (the reference's num_edges counter: insertions, not distinct edges),
 *                       dropped, build_ms (HIP-event time of the build's kernels: the allocations and the two small
 *                       device-to-host reads between them are not in it); NULL = skip
 *   pw_csr_dev_export   copies to host arrays of the caller: indptr uint32[n_nodes + 1], indices uint32[nnz], data
 *                       float32[nnz] (all 1.0 when no weights were given); NULL = skip
 *   pw_csr_create_device  a walk handle on the same device: the same validation, membership index and lane index, hence the
 *                       same walks, as pw_csr_create on the exported arrays.  The host passes of the index build (work items,
 *                       degrees) read host arrays: h_indptr / h_indices / h_data = what pw_csr_dev_export wrote (h_data is
 *                       ignored when no weights were given), so a caller that exported anyway pays no second download; all
 *                       three NULL = the CSR comes down once inside the call.  Arrays that differ from the device CSR give
 *                       an inconsistent handle.  The handle's device copy is made device to device; the pw_csr_dev stays
 *                       valid and owns its arrays until pw_csr_dev_destroy, so the device holds the CSR twice while the handle
 *                       is built.  pw_csr_create builds the lane index only when it fits in half of the free device memory:
 *                       within one CSR's size of that limit this handle can come without the lane index that pw_csr_create
 *                       on the exported arrays, with the pw_csr_dev destroyed first, would build. */
typedef struct pw_csr_dev pw_csr_dev;
int pw_coo_to_csr_device(int device, const int64_t *d_src, const int64_t *d_dst, const float *d_weight, uint64_t m,
                         uint64_t n_nodes, int directed, pw_csr_dev **out);
int pw_csr_dev_shape(const pw_csr_dev *c, uint64_t *n_nodes, uint64_t *nnz, uint64_t *insertions, uint64_t *dropped,
                     double *build_ms);
int pw_csr_dev_export(const pw_csr_dev *c, uint32_t *indptr, uint32_t *indices, float *data);
void pw_csr_dev_destroy(pw_csr_dev *c);
int pw_csr_create_device(const pw_csr_dev *c, const uint32_t *h_indptr, const uint32_t *h_indices, const float *h_data,
                         pw_graph **out);

/* Device time (ms) of the index kernels pw_csr_create ran, device bytes of the index, and the number of entries
 * of the lane kernel's common-neighbour lists (0: lane index not built).  Any pointer may be NULL. */
int pw_graph_index_info(const pw_graph *g, double *build_ms, uint64_t *index_bytes, uint64_t *lane_list_entries);
/* Test hook: the lane index decoded to flat arrays (any pointer may be NULL).  For every CSR entry e = (u -> v):
 * n_in[e] = |N(u) & N(v)| (less u itself when u has a self loop: the reference takes prev out of the common neighbours,
 * sparse_rw.py:79-87), rev_pos[e] = position of u in row v (0xffffffff: v -> u is not an edge); entries = the
 * positions in row v of those common neighbours, ascending, concatenated in entry order (lane_list_entries values,
 * pw_graph_index_info).  PW_ERR_UNSUPPORTED when the graph has no lane index (weighted graphs with self loops). */
int pw_lane_index_export(pw_graph *g, uint32_t *n_in, uint32_t *rev_pos, uint32_t *entries);

/* Dense adjacency in the reference's DenseGraph layout (graph.py:576-580): float64[n, n]
 * row-major; nonzero mask = (data != 0). */
int pw_dense_create(const double *data, uint32_t n_nodes, int device, pw_graph **out);

/* Unweighted dense graph from its bit-packed adjacency: row u = ceil(n/64) uint64 words, bit x of the
 * row set <=> nonzero[u, x] (the reference's bool mask, graph.py:580, one bit per entry).  The
 * pointer may be a host pointer (on_device = 0) or a device pointer on `device` (on_device = 1);
 * lets a 100k-node dense graph be created without materialising the 80 GB float64 matrix. */
int pw_dense_create_bits(const uint64_t *adjbits, uint32_t n_nodes, int on_device, int device,
                         pw_graph **out);

/* ---- dense handles built on the device ------------------------------------------------------------------------------------
 * pw_dense_create is one host thread over all n^2 values; these entries make the same handle from data that is already in
 * device memory (csrc/dense_build.hip.h): two passes over the matrix, or one over a device CSR.
 *   pw_dense_create_device    d_data: row-major [n_nodes, n_nodes] matrix on `device`, float64 (is_f32 = 0) or float32 (is_f32
 *                             != 0: every value widened to float64, which is exact).  The handle equals pw_dense_create's on the
 *                             same values: packed adjacency rows (tail bits zero), rows compressed in ascending column order,
 *                             values dropped when they are all 1.0, degrees, the same 2^32 - 1 edge limit.  A NaN is a non-zero
 *                             entry, -0.0 is none.  n_nodes == 0: PW_ERR_INVALID.  The matrix is only read, and not referenced
 *                             after the call.  Work runs on the handle's stream; the call returns when it is done.
 *   pw_dense_create_from_csr  the same handle from a pw_csr_dev (pw_coo_to_csr_device): the dense float64 form of that CSR --
 *                             float32 weights widened, every weight 1.0 when the CSR has none.  A pw_csr_dev that carries float64
 *                             weights (pw_edgelist_read_device_ex, PW_EDGELIST_KEEP_F64) gives them as they are, and unit /
 *                             dense_nonneg are judged on them: weights that are all 1.00000001 are 1.0 in float32 and still make
 *                             no unit handle; weights that are all exactly 1.0 do, values dropped.  The pw_csr_dev stays valid.
 *   build_ms (optional)       HIP-event time of the build's kernels; allocations and the small device-to-host reads between
 *                             them are outside it (as pw_csr_dev_shape's build_ms).
 *   pw_dense_noise_thresholds the node2vec+ thresholds pw_noise_thresholds_dense computes from the matrix, computed on the device
 *                             from the handle's compressed rows (all ones for a unit handle; NaN for an empty row), bit for bit;
 *                             installed in the handle as pw_graph_set_thresholds installs them and copied to thr[n_nodes] when
 *                             thr is not NULL.  PW_ERR_UNSUPPORTED for CSR handles and pw_dense_create_bits handles.
 *   pw_dense_shape            n_nodes, nnz, words per adjacency row, maximum degree of a dense handle; NULL = skip
 *   pw_dense_export           test hook and host read-back: copies to host arrays of the caller indptr uint32[n + 1], indices
 *                             uint32[nnz], data float64[nnz] (all 1.0 for a unit handle), adjbits uint64[n * words_per_row], deg
 *                             uint32[n]; *flags: bit 0 = unit, bit 1 = dense_nonneg; NULL = skip.  indices / data:
 *                             PW_ERR_UNSUPPORTED for pw_dense_create_bits handles. */
int pw_dense_create_device(int device, const void *d_data, int is_f32, uint32_t n_nodes, pw_graph **out, double *build_ms);
int pw_dense_create_from_csr(const pw_csr_dev *c, pw_graph **out, double *build_ms);
int pw_dense_noise_thresholds(pw_graph *g, double gamma, float *thr);
int pw_dense_shape(const pw_graph *g, uint32_t *n_nodes, uint32_t *nnz, uint32_t *words_per_row, uint32_t *max_degree);
int pw_dense_export(pw_graph *g, uint32_t *indptr, uint32_t *indices, double *data, uint64_t *adjbits, uint32_t *deg,
                    uint32_t *flags);

/* node2vec+ noise thresholds, float32[n_nodes] (sparse_rw.py:22-35 / dense_rw.py:11-19);
 * required before a call with extend != 0. */
int pw_graph_set_thresholds(pw_graph *g, const float *thr);

void pw_graph_destroy(pw_graph *g);

/* ---- the walk operator ----------------------------------------------------------------- */
/*
 * Replaces Base._random_walks + has_nbrs + move_forward.
 *   starts      uint32[n_jobs]  (already shuffled by the caller, pecanpy.py:135-141)
 *   out         uint32[n_jobs * (walk_length + 2)]
 *   has_seed=0  -> seed taken from the OS (reference: random_state=None)
 *   stream_skip doubles of the stream consumed by earlier shards (0 for a whole job array)
 * pw_simulate takes host pointers (copies in/out); pw_simulate_device takes device pointers on
 * the handle's GPU (nothing crosses PCIe) and is what bench.py times.
 */
int pw_simulate(pw_graph *g, int mode, double p, double q, int extend, const uint32_t *starts,
                uint64_t n_jobs, uint32_t walk_length, int has_seed, uint32_t seed,
                uint64_t stream_skip, uint32_t *out, pw_stats *stats);

int pw_simulate_device(pw_graph *g, int mode, double p, double q, int extend,
                       const uint32_t *d_starts, uint64_t n_jobs, uint32_t walk_length,
                       int has_seed, uint32_t seed, uint64_t stream_skip, uint32_t *d_out,
                       pw_stats *stats);

/* ---- several GPUs from ONE process -------------------------------------------------------
 * The reference is one process: `pecanpy` reads a graph, calls simulate_walks() once and writes the result
 * (src/pecanpy/cli.py:328-351); its parallelism is Numba's thread pool inside _random_walks (pecanpy.py:165, 189).  The
 * counterpart here is one host thread per device inside one call -- no launcher, no torch.distributed:
 *   pw_csr_create_multi   builds the handle on devices[0] and REPLICATES it to the other devices (pw_graph_replicate:
 *                         CSR + the whole per-graph index copied device to device over xGMI, not rebuilt); a device may
 *                         be named more than once (every entry is a replica with its own streams and scratch).
 *                         out_handles[n_devices] receives the handles (destroy each with pw_graph_destroy).
 *   pw_device_mask_to_list  bit d of device_mask set <=> device d; returns how many devices the mask names (negative
 *                         pw_status when it names one that is not visible) and writes the first `cap` of them.
 *   pw_simulate_multi     the walk operator over replicas of one graph: the job array is split into contiguous shards
 *                         (the prange static chunking of pecanpy.py:189), shard i starts in the ONE random stream where
 *                         the earlier shards' draws end (announced as by pw_count_stream_draws; on directed graphs with
 *                         dead ends the later shards are walked again with the draws actually consumed), so the matrix
 *                         is bit-identical to pw_simulate on one handle.  starts: host pointer.  out_on_device = 0: out
 *                         is host memory, every device copies its rows out itself (its own PCIe link); 1: out is device
 *                         memory on handles[0]'s GPU, the other devices' rows arrive by peer copies (xGMI).
 *                         Alias / first-order modes (sequential stream) run on handles[0] alone.  pw_stats: sums; the
 *                         kernel times are the maximum over the shards (they run side by side).
 * Thresholds for extend != 0 are set per handle (pw_graph_set_thresholds; a replica inherits what its source had). */
int pw_graph_replicate(const pw_graph *src, int device, pw_graph **out);
int pw_device_mask_to_list(uint64_t device_mask, int *devices, int cap);
int pw_csr_create_multi(const uint32_t *indptr, const uint32_t *indices, const float *data, uint32_t n_nodes, uint32_t nnz,
                        const int *devices, int n_devices, pw_graph **out_handles);
int pw_simulate_multi(pw_graph *const *handles, int n_handles, int mode, double p, double q, int extend,
                      const uint32_t *starts, uint64_t n_jobs, uint32_t walk_length, int has_seed, uint32_t seed,
                      uint64_t stream_skip, uint32_t *out, int out_on_device, pw_stats *stats);

/* One transition of the on-the-fly modes for a given (cur, prev) -- the operator boundary of the reference's
 * callbacks: move_forward(cur, prev) (pecanpy.py:543-559 / 597-612) with the uniform draw r in [0, 1) supplied by the
 * caller (the reference draws it with np.random.random() inside), and get_normalized_probs(cur, prev)
 * (rw/sparse_rw.py:51-130, rw/dense_rw.py:34-118).  has_prev = 0: first step of a walk (prev ignored).
 *   pw_step : *next = sampled neighbour, *position (may be NULL) = its index in cur's row (== degree when the float
 *             CDF never reached r: the reference's overflow read, mirrored)
 *   pw_probs: probs = float32[degree(cur)] for CSR handles, float64[degree(cur)] for dense handles and mode 6 (room for the
 *             maximum degree of the graph), *n = degree(cur)
 * The same device code as the walk kernels' eager step; one launch per call (API compatibility and tests, not a
 * throughput path). */
int pw_step(pw_graph *g, int mode, double p, double q, int extend, uint32_t cur, int has_prev, uint32_t prev, double r,
            uint32_t *next, uint32_t *position);
int pw_probs(pw_graph *g, int mode, double p, double q, int extend, uint32_t cur, int has_prev, uint32_t prev, void *probs,
             uint32_t *n);

/* Alias tables of the PreComp modes, built on the device and kept in the handle.
 *   first_order = 0: PreComp.preprocess_transition_probs (pecanpy.py:442-507): sum(deg^2) entries,
 *                    table of (v, k-th neighbour as prev) at alias_indptr[v] + deg(v) * k
 *   first_order = 1: PreCompFirstOrder.preprocess_transition_probs (pecanpy.py:336-361): nnz entries
 * pw_simulate* with PW_MODE_PRECOMP / PW_MODE_PRECOMP_FIRST_ORDER builds them on demand.
 * pw_precomp_export copies them to host arrays (alias_indptr uint64[n_nodes+1] may be NULL for
 * first_order); *n_entries receives the table length (call with NULL arrays to query it).
 * Tables built with extend name the threshold upload they were built from: after pw_graph_set_thresholds the
 * next build (or PreComp call) builds them again, and pw_precomp_export returns PW_ERR_INVALID until it has. */
int pw_precomp_build(pw_graph *g, double p, double q, int extend, int first_order);
int pw_precomp_export(pw_graph *g, uint64_t *alias_indptr, uint32_t *alias_j, float *alias_q,
                      uint64_t *n_entries);

/* Number of stream doubles the jobs starts[0..n_jobs) consume when no walk dead-ends mid-way
 * (= walk_length x number of starts with at least one neighbour).  Lets a multi-GPU driver
 * compute each shard's stream_skip without running the walks. */
int pw_count_stream_draws(pw_graph *g, const uint32_t *starts, uint64_t n_jobs,
                          uint32_t walk_length, uint64_t *out_draws);

/* The draws [stream_skip, stream_skip + n_draws) of `seed`'s MT19937 stream, expanded once and KEPT in the handle:
 * pw_simulate_device calls with that seed whose draws lie inside use them in place (no jump-ahead, no expansion) until
 * pw_stream_release, the next pw_stream_hold or a pw_simulate call that walks in parts.  For a shard walked in several
 * calls (chunks that travel while the next is walked): one jump tree per shard instead of one per chunk. */
int pw_stream_hold(pw_graph *g, uint32_t seed, uint64_t stream_skip, uint64_t n_draws);
int pw_stream_release(pw_graph *g);

/* ---- skip-gram training over a walk matrix (the stage after the walks) ------------------- */
/* Word2Vec(walks, sg=1, negative, window, epochs) of Base.embed / cli.learn_embeddings (pecanpy.py:276-290,
 * cli.py:307-325) as a HIP kernel: skip-gram with negative sampling, word2vec.c's update rule, unigram^0.75 negative
 * table, walks thinned by the subsampling of frequent nodes (sample, 0 = off) before the windows are taken, window
 * shrunk at random, learning rate alpha -> min_alpha linearly over the run.  Every random choice is a hash of (seed,
 * epoch, walk, position, ...): the SET of updates depends on the seed only, their order on `workers`:
 *   workers = 1  one wavefront, sentence order: deterministic; equals the sequential restatement oracle/sgns_ref.c
 *                within float tolerance (tests/test_gpu_sgns.py) -- what gensim's workers=1 is to gensim;
 *   workers = 0  as many wavefronts as the corpus feeds (hogwild, unsynchronised updates, like gensim's threads);
 *   workers > 1  that many wavefronts.
 * Not bit-comparable with gensim itself (its own random streams; not installed here).
 *   walks   host uint32[n_walks, walk_length + 2] as pw_simulate returns it (indices into 0..n_nodes-1; a node id
 *           >= n_nodes or a length cell > walk_length + 1 is rejected with PW_ERR_INVALID)
 *   vectors host float32[n_nodes, dim] (out), dim <= 512
 * walk_length must be below 8192 (the thinned walk of a wavefront lives in LDS).  pw_sgns_train is upload ->
 * pw_sgns_train_device -> download: one preparation path, one kernel. */
int pw_sgns_train(int device, const uint32_t *walks, uint64_t n_walks, uint32_t walk_length, uint32_t n_nodes,
                  uint32_t dim, uint32_t window, uint32_t negative, uint32_t epochs, float alpha, float min_alpha,
                  float sample, uint32_t seed, uint32_t workers, float *vectors);

/* What a training call did.  vocab_ms: counting pass, noise table, keep probabilities and their upload (host clock);
 * init_ms: syn0 initialisation and upload (host clock); train_ms: the training kernels of all epochs (hipEvent). */
typedef struct pw_sgns_stats {
    double vocab_ms, init_ms, train_ms;
    uint64_t kept_occurrences; /* occurrences that survived the subsampling, summed over the epochs */
    uint64_t trained_pairs;    /* (centre, context) pairs, each updating negative + 1 target rows at most */
    uint64_t wavefronts;       /* wavefronts of one training launch */
} pw_sgns_stats;

/* The same trainer on a walk matrix that is already in device memory, where pw_simulate_device leaves it: no copy of
 * the matrix in either direction (the word counts come down and the tables go up: tens of MB).
 *   d_walks   device uint32[n_walks, walk_length + 2] on `device` (same checks and error texts as pw_sgns_train)
 *   d_vectors device float32[n_nodes, dim] on `device` (out; trained in place)
 *   stats     may be NULL
 * Work is queued on the device's default stream; the call returns after it has finished. */
int pw_sgns_train_device(int device, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint32_t n_nodes,
                         uint32_t dim, uint32_t window, uint32_t negative, uint32_t epochs, float alpha, float min_alpha,
                         float sample, uint32_t seed, uint32_t workers, float *d_vectors, pw_sgns_stats *stats);

/* ---- the trainer as a session: epochs in slices, a loss, both matrices (csrc/sgns.hip.h) ------------------------------------
 * pw_sgns_train_device is create -> run(epochs) -> vectors_get(0) -> destroy on this handle: one preparation path.
 *   pw_sgns_create_device  the preparation of pw_sgns_train_device -- the same checks and error texts, the word counts, the
 *                          noise table, the keep probabilities, the seeded syn0, a zeroed syn1, the wavefront count from
 *                          `workers` -- and no training.  The handle owns syn0, syn1 and the tables.  d_walks is BORROWED, not
 *                          copied: the matrix must stay allocated and unchanged until pw_sgns_destroy.  `epochs` is the length of
 *                          the learning-rate schedule.  flags: PW_SGNS_LOSS = every launch also computes the epoch's loss.
 *   pw_sgns_run            the next n_epochs epochs of the schedule, one launch each; returns when they are done.  per_epoch
 *                          (n_epochs cells, may be NULL): kept_occurrences and trained_pairs of that epoch; with PW_SGNS_LOSS
 *                          loss = the sum over its trained evaluations of softplus(-dot) for the centre and softplus(dot) for a
 *                          negative (gensim's skip-gram / negative-sampling loss), in float64 from the float32 dot product the
 *                          update used, taken before the update; evaluations = their number.  Both 0 without the flag.  The sum
 *                          is made without floating-point atomics, in an order fixed by the number of walks: per-walk sums in
 *                          evaluation order, then blocks of 4096 walks, then the block sums.  With workers = 1 it is a function
 *                          of the seed.  stats (may be NULL): vocab_ms / init_ms of the create call, train_ms and the counters of
 *                          this run.  More epochs than the schedule has left: PW_ERR_INVALID before any launch.
 *   pw_sgns_get_state / pw_sgns_set_state
 *                          epoch: the global epoch index, which every hash of (seed, epoch, walk, position) uses; pw_sgns_run
 *                          only ever grows it.  sched_pos / sched_total: epochs of the schedule done / in all; the learning rate
 *                          of an item is alpha - (alpha - min_alpha) * (items before it in the schedule / items of the schedule),
 *                          at least min_alpha.  set_state restores a checkpoint (with pw_sgns_vectors_set for both matrices)
 *                          and starts a new schedule on the trained vectors (sched_pos = 0, another sched_total / alpha /
 *                          min_alpha; epoch left as it is).  sched_total = 0 or sched_pos > sched_total: PW_ERR_INVALID.
 *   pw_sgns_vectors_get / pw_sgns_vectors_set
 *                          a device-to-device copy of syn0 (which = 0: the input vectors, the embedding) or syn1 (which = 1: the
 *                          context vectors, gensim's syn1neg) out of / into the handle; d_ptr = float32[n_nodes, dim],
 *                          contiguous, on the handle's device.
 *   pw_sgns_evaluate       scores, trains nothing: the evaluations a PW_SGNS_LOSS launch of global epoch index `epoch` performs on
 *                          the matrix -- the same subsampling, windows and negatives, hashes of (seed, epoch, walk, position)
 *                          with item base n_walks * (walk_length + 1) * epoch of THAT matrix -- against syn0 / syn1 as they are,
 *                          by a kernel of its own that writes no vector (sgns_eval_kernel).  d_walks = NULL: the session's own
 *                          matrix (n_walks / walk_length ignored); any other device matrix may have its own shape and gets the
 *                          checks and error texts of the create call (a node id >= n_nodes, a length cell > walk_length + 1,
 *                          walk_length >= 8192).  out: loss, evaluations, kept_occurrences, trained_pairs (the pairs scored);
 *                          PW_SGNS_LOSS is not needed on the handle.  The sum is made as pw_sgns_run makes it; nothing is
 *                          written, so nothing races: the launch takes as many wavefronts as the matrix feeds whatever
 *                          `workers` is, and the record is a function of (seed, epoch, matrix, vectors), bit for bit.  syn0,
 *                          syn1, the tables and the state are unchanged.
 *   pw_sgns_set_walks      another matrix under the session, BORROWED like the first (the old one is no longer used).  It must
 *                          have the session's (n_walks, walk_length) -- the schedule arithmetic stays; another shape is
 *                          PW_ERR_INVALID -- and gets the content checks of the create call.  flags = 0: the noise table and
 *                          the keep probabilities stay those of the create call; PW_SGNS_RECOUNT: they are rebuilt from the new
 *                          matrix by the create call's own path.  The state and both matrices are not touched.  On any error
 *                          the session keeps the old matrix and all its tables.
 *   pw_sgns_set_locks / pw_sgns_get_locks
 *                          frozen rows.  d_lock0 / d_lock1: device uint8[n_nodes] on the handle's device, non-zero = the row of
 *                          syn0 / syn1 is frozen; NULL = no row of that matrix.  The masks are COPIED (packed to bits by a small
 *                          kernel, one ballot per 64 rows: bit r % 32 of word r / 32 covers row r, the bits at and beyond n_nodes
 *                          in the last word are zero), not borrowed, and the handle owns the bit arrays.  A call replaces the
 *                          locks of BOTH matrices; a mask without a non-zero byte counts as NULL.  A frozen row is read by every
 *                          pair that names it and never written: pw_sgns_run then launches the LOCK instances of the kernel, which
 *                          evaluate exactly what the others evaluate -- the same pairs, draws, dot products, loss terms, counters
 *                          -- skip the store of a frozen row, and still let a free context row learn from a frozen target.  With no
 *                          row frozen in either matrix pw_sgns_run launches the kernel without locks, bit for bit what a handle
 *                          that never had locks runs.  Locks survive pw_sgns_run, pw_sgns_set_state, pw_sgns_vectors_set,
 *                          pw_sgns_set_walks (with and without PW_SGNS_RECOUNT) and pw_sgns_evaluate; they do NOT protect against
 *                          pw_sgns_vectors_set, which replaces a matrix wholesale as before.  On any error the handle keeps the
 *                          locks it had.  get_locks writes them back as uint8[n_nodes] 0 / 1, zeros where none; either pointer
 *                          may be NULL.
 *   pw_sgns_lock_info      out[0] / out[1]: frozen rows of syn0 / syn1; out[2]: 1 when the last pw_sgns_run launched the LOCK
 *                          instances, 0 when it launched the kernel without locks (or nothing ran yet).
 *   pw_sgns_destroy        frees what the handle owns; NULL is allowed. */
enum { PW_SGNS_LOSS = 1 };
enum { PW_SGNS_RECOUNT = 1 };
typedef struct pw_sgns pw_sgns;
typedef struct pw_sgns_epoch {
    double loss;
    uint64_t kept_occurrences, trained_pairs, evaluations;
} pw_sgns_epoch;
typedef struct pw_sgns_state {
    uint64_t epoch;
    uint64_t sched_pos, sched_total;
    float alpha, min_alpha;
} pw_sgns_state;
int pw_sgns_create_device(int device, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint32_t n_nodes,
                          uint32_t dim, uint32_t window, uint32_t negative, uint32_t epochs, float alpha, float min_alpha,
                          float sample, uint32_t seed, uint32_t workers, uint32_t flags, pw_sgns **out);
int pw_sgns_run(pw_sgns *s, uint32_t n_epochs, pw_sgns_epoch *per_epoch, pw_sgns_stats *stats);
int pw_sgns_get_state(const pw_sgns *s, pw_sgns_state *st);
int pw_sgns_set_state(pw_sgns *s, const pw_sgns_state *st);
int pw_sgns_vectors_get(pw_sgns *s, int which, float *d_ptr);
int pw_sgns_vectors_set(pw_sgns *s, int which, const float *d_ptr);
int pw_sgns_evaluate(pw_sgns *s, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint64_t epoch, pw_sgns_epoch *out);
int pw_sgns_set_walks(pw_sgns *s, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint32_t flags);
int pw_sgns_set_locks(pw_sgns *s, const uint8_t *d_lock0, const uint8_t *d_lock1);
int pw_sgns_get_locks(const pw_sgns *s, uint8_t *d_lock0, uint8_t *d_lock1);
int pw_sgns_lock_info(const pw_sgns *s, uint64_t out[3]);
void pw_sgns_destroy(pw_sgns *s);

/* ---- the embedding file written from device memory (csrc/emb_text.hip.h) --------------------------------------------------
 * The text format of gensim's KeyedVectors.save_word2vec_format, the output of `pecanpy --output G.emb` (cli.py:323-325), made
 * on the device from the vectors where pw_sgns_train_device leaves them: only the text crosses to the host.
 *   file       "<n_rows> <dim>\n", then per row its name, " " + the component for every component, "\n".  A component is
 *              written as printf("%.6f", (double)x) writes it -- Python's "%.6f" % float(x) -- byte for byte: rounded to six
 *              decimals exactly, ties to even on the binary value (integer arithmetic on mantissa and exponent); -0.0 and
 *              negative values that round to zero give "-0.000000"; "nan" for a NaN of either sign; "inf" / "-inf"; at most
 *              47 characters (-FLT_MAX).  The bytes are a function of the input alone.
 *   d_vectors  device float32[n_rows, dim] on `device`, row-major and contiguous; only read.  Any n_rows >= 1, dim >= 1.
 *   id_chars, id_offsets   host: the names as one byte blob (UTF-8 as given, not inspected) and uint64[n_rows + 1] offsets,
 *              row i's name = id_chars[id_offsets[i] : id_offsets[i + 1]] (pw_edgelist_export's layout); uploaded by the call.
 *   path       created or truncated; the library writes it itself (fwrite of whole chunks).
 *   chunks     the rows are taken in consecutive blocks, each the longest run of rows whose text fits a byte budget: 32 MiB, or
 *              PECANPY_AMD_EMB_CHUNK_BYTES; a budget below what one row can take (its name, dim times 48 bytes, the newline,
 *              with the longest name) is raised to that.  One device buffer of the budget (of the whole text when that is
 *              less) and two pinned host buffers: chunk k + 1 is formatted and copied while chunk k is written.
 *   stats      optional.
 * PW_ERR_INVALID: n_rows == 0, dim == 0, offsets that do not ascend, a path that cannot be opened or written (strerror in
 * the message).  A failed call may leave a partial file.  Work runs on the device's default stream; the call returns when
 * the file is closed.  pw_vectors_write_text is the same for a matrix in host memory: upload, then the same path. */
typedef struct pw_emb_write_stats {
    double format_ms;   /* HIP-event time of the kernels: count pass, scan, the fill pass of every chunk */
    double copy_ms;     /* HIP-event time of the device-to-host copies of the chunks */
    double write_ms;    /* host clock of the fwrite calls and the fclose */
    uint64_t bytes;     /* size of the file */
    uint64_t chunks;
} pw_emb_write_stats;
int pw_vectors_write_text_device(int device, const float *d_vectors, uint64_t n_rows, uint32_t dim, const char *id_chars,
                                 const uint64_t *id_offsets, const char *path, pw_emb_write_stats *stats);
int pw_vectors_write_text(int device, const float *vectors, uint64_t n_rows, uint32_t dim, const char *id_chars,
                          const uint64_t *id_offsets, const char *path, pw_emb_write_stats *stats);
/* Test hook: x[i] as the writer formats it, at chars[48 i ..) (the rest of the slot zero), lens[i] = the number of characters
 * (0xffffffff if the writer's count pass would disagree with its fill pass).  on_device = 0: the host build of the routine
 * (csrc/emb_text.hip.h: format_f6), usable without a GPU; on_device != 0: one thread per value of a kernel on `device`. */
int pw_selftest_format_f6(int on_device, int device, const float *x, uint64_t n, char *chars, uint32_t *lens);
/* Test hook: the device's exclusive prefix sum (csrc/scan.hip.h), the one behind every offset table of the library.  x = n
 * values of uint32 (width 32) or uint64 (width 64) in host memory, replaced by x'[i] = x[0] + ... + x[i - 1] in that width;
 * *total = their sum.  n == 0 launches nothing and gives 0. */
int pw_selftest_exclusive_scan(int device, int width, void *x, uint64_t n, uint64_t *total);

/* ---- the walk corpus file written from device memory (csrc/walk_text.hip.h) ------------------------------------------------
 * One walk per line, the names of its nodes separated by single spaces: what gensim's LineSentence / Word2Vec(corpus_file=),
 * fastText and word2vec.c read, and what `pecanpy --task walks` writes -- made on the device from the walk matrix where
 * pw_simulate_device leaves it: only the text crosses to the host.
 *   file       no header.  Row r with len = r[walk_length + 1] gives the names of r[0] .. r[len - 1] joined by " ", then "\n"
 *              (len == 0: just "\n").  Cells at positions >= len are never read.  The bytes are a function of the input alone.
 *   d_walks    device uint32[n_walks, walk_length + 2] on `device`, row-major and contiguous; only read.  walk_length < 2^31.
 *   id_chars, id_offsets, n_names   host: the names as one byte blob (UTF-8 as given, not inspected) and uint64[n_names + 1]
 *              offsets, node i's name = id_chars[id_offsets[i] : id_offsets[i + 1]] (at most 2^25 - 1 bytes, may be empty);
 *              uploaded by the call.  The names are looked up by node index.
 *   path       created or truncated; the library writes it itself (fwrite of whole chunks).
 *   chunks     as pw_vectors_write_text_device: consecutive rows while their text fits a byte budget of 32 MiB, or
 *              PECANPY_AMD_WALKS_CHUNK_BYTES; a budget below the longest possible row, (walk_length + 1) * (longest name + 1),
 *              is raised to that.  One device buffer, two pinned host buffers.
 *   stats      optional.
 * n_walks == 0 writes an empty file; walk_length == 0 is a corpus of start nodes; n_names may exceed what a node index can
 * address (the names beyond are never looked up).  PW_ERR_INVALID: offsets that do not ascend, a name that is too long, a path that
 * cannot be opened or written (strerror in the message), and what the matrix itself holds: a row length above
 * walk_length + 1 ("row length ...") or, among the first len cells of a row, a node index >= n_names ("node index ...
 * outside the ... names").  The matrix is checked on the device before any text is made -- such a value is compared, never
 * used as an index -- and the file is left empty.  Any other failed call may leave a partial file.  Work runs on the
 * device's default stream; the call returns when the file is closed.  pw_walks_write_text is the same for a matrix in host
 * memory: upload, then the same path. */
typedef struct pw_walks_write_stats {
    double format_ms;   /* HIP-event time of the kernels: count pass, scan, the fill pass of every chunk */
    double copy_ms;     /* HIP-event time of the device-to-host copies of the chunks */
    double write_ms;    /* host clock of the fwrite calls and the fclose */
    uint64_t bytes;     /* size of the file */
    uint64_t chunks;
    uint64_t rows;      /* lines written = n_walks */
    uint64_t tokens;    /* names written = the sum of the row lengths */
} pw_walks_write_stats;
int pw_walks_write_text_device(int device, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, const char *id_chars,
                               const uint64_t *id_offsets, uint64_t n_names, const char *path, pw_walks_write_stats *stats);
int pw_walks_write_text(int device, const uint32_t *walks, uint64_t n_walks, uint32_t walk_length, const char *id_chars,
                        const uint64_t *id_offsets, uint64_t n_names, const char *path, pw_walks_write_stats *stats);

/* ---- nearest neighbours of embedding vectors, exact and ordered (csrc/knn.hip.h) ---------------------------------------------
 * What gensim's wv.most_similar answers, on the vectors where the trainer leaves them, by one written definition whose
 * answer is unique -- the device kernels are held to it bit for bit (the full text stands at the top of csrc/knn.hip.h):
 *   dot(a, b)  = (((0.0 + a[0] b[0]) + a[1] b[1]) + ...), k ascending, in float64 on the float32 values widened (the products
 *                are exact, the dim additions the only roundings; fma and multiply-add give the same bits);
 *   norm(x)    = sqrt(dot(x, x)), correctly rounded;
 *   score      PW_KNN_DOT: dot(q, x).  PW_KNN_COSINE: dot(q, x) / (norm(q) * norm(x)), +0.0 when that product is 0;
 *   order      descending score, equal scores by ascending row number: total, so the top topn are unique;
 *   exclude_self   a query given as a row number leaves that one row out (a different row with the same contents stays); a
 *                query given as a vector excludes nothing;
 *   output     idx uint32[nq, topn], score float64[nq, topn]; slots beyond the number of candidates hold 0xFFFFFFFF / -inf.
 * Limits: 1 <= topn <= PW_KNN_MAX_TOPN, 1 <= dim <= 4096, 1 <= n_rows < 2^32; nq = 0 is a valid call that does nothing.
 * PW_ERR_INVALID, nothing written: a NaN or an infinity in the matrix ("row <i> ...") or in a query vector ("query <i> ..."),
 * naming the first; a row number >= n_rows; both or neither of d_queries and d_rows; a limit exceeded.
 *   pw_knn_create_device   COPIES the matrix (device float32[n_rows, dim], contiguous): the index is a snapshot, a session that
 *                goes on training does not change it.  Computes the norms and refuses non-finite rows.  pw_knn_create: the same
 *                from host memory.
 *   pw_knn_query_device    d_queries (device float32[nq, dim]) or d_rows (device uint32[nq]) -- exactly one; d_idx, d_score on the
 *                index's device.  Runs on the device's default stream and returns when the results are written.  stats is
 *                optional.
 *   pw_knn_info, pw_knn_norms_get (device float64[n_rows]), pw_knn_destroy (NULL is harmless). */
#define PW_KNN_MAX_TOPN 128
enum { PW_KNN_DOT = 0, PW_KNN_COSINE = 1 };
typedef struct pw_knn pw_knn;
typedef struct pw_knn_stats {
    double score_ms, merge_ms;   /* HIP-event time of the score kernel and of the merge kernel, summed over the batches */
    double total_ms;             /* host clock of the call */
    uint32_t grid;               /* workgroups of the score kernel = row_parts * tile_parts (the first batch's) */
    uint32_t row_parts;          /* parts the row blocks are dealt to: a query has row_parts * rows_per_block / 64 partial lists */
    uint32_t rows_per_block, queries_per_tile, col_chunk;   /* the tile actually used (pw_knn_tiles) */
    uint32_t batches;            /* query batches (the widened queries of a batch stay within 256 MiB) */
} pw_knn_stats;
typedef struct pw_knn_tiles {    /* test configuration of pw_selftest_knn; 0 in a field = the default */
    uint32_t rows_per_block;     /* rows a workgroup stages at a time: 64, 128 or 256 (default: by nq) */
    uint32_t queries_per_tile;   /* queries a wavefront keeps accumulators for: 1 .. 8 (default 8) */
    uint32_t grid;               /* workgroups of the score kernel, at most 65536 (default: what the device holds at once) */
    uint32_t col_chunk;          /* columns staged at a time: a multiple of 4, at most 32 (default 32) */
} pw_knn_tiles;
int pw_knn_create_device(int device, const float *d_vectors, uint64_t n_rows, uint32_t dim, pw_knn **out);
int pw_knn_create(int device, const float *vectors, uint64_t n_rows, uint32_t dim, pw_knn **out);
int pw_knn_query_device(pw_knn *k, const float *d_queries, const uint32_t *d_rows, uint64_t nq, uint32_t topn, int metric,
                        int exclude_self, uint32_t *d_idx, double *d_score, pw_knn_stats *stats);
int pw_knn_info(const pw_knn *k, uint64_t *n_rows, uint32_t *dim, uint64_t *bytes);
int pw_knn_norms_get(pw_knn *k, double *d_norms);
void pw_knn_destroy(pw_knn *k);
/* Test hook: the whole query on HOST pointers.  on_device = 0: the host build of the definition (plain loops), usable
 * without a GPU; otherwise upload, the kernels with the forced tiles (NULL: the defaults), download.  Same refusals. */
int pw_selftest_knn(int on_device, int device, const float *vectors, uint64_t n, uint32_t dim, const float *queries,
                    const uint32_t *rows, uint64_t nq, uint32_t topn, int metric, int exclude_self, const pw_knn_tiles *tiles,
                    uint32_t *idx, double *score);

/* ---- link prediction in device memory: pair scores, exact AUC, non-edges from the seeded stream --------------------------
 * The three definitions are written at the top of csrc/linkpred.hip.h (DESIGN.md 4.9 repeats them); host and device answer
 * them identically, whatever the grid, the tiling or the batch size.  Refusals: PW_ERR_INVALID with a message that names the
 * first offending element, nothing written.
 *   pw_knn_score_pairs_device   d_score[i] = the score (pw_knn's dot / norm / score, the stored norms) of row d_u[i] of `a` and row
 *                d_v[i] of `b` (NULL: of `a`).  `b` must have a's dim and device; row numbers are checked against each index's
 *                n_rows.  m = 0 is a valid call that does nothing; u[i] == v[i] and repeated pairs are allowed.  d_u, d_v
 *                (uint32[m]) and d_score (float64[m]) on the indexes' device.
 *   pw_auc_device   out[0] = wins = #{(i, j): pos[i] > neg[j]}, out[1] = ties = #{(i, j): pos[i] == neg[j]}, IEEE comparison
 *                (-0.0 == +0.0, infinities ordinary); the AUC is (2 wins + ties) / (2 m n).  d_pos float64[m], d_neg float64[n]
 *                on `device`; m, n >= 1, m * n < 2^62, n < 2^32.  A NaN in either array is refused ("pos[i]" before "neg[j]").
 *   pw_sample_non_edges_device   candidate c, counted from first_candidate, of the words w of RandomState(seed) (pw_mt_words):
 *                u = (w[2c] * n_nodes) >> 32, v = (w[2c+1] * n_nodes) >> 32, accepted when u != v and v is not in row u.  d_u,
 *                d_v (device uint32[m]) receive the first m accepted candidates in candidate order (pairs may repeat);
 *                *candidates_used = one past the last candidate examined, minus first_candidate: a call at first_candidate +
 *                *candidates_used continues the sequence.  PW_ERR_UNSUPPORTED on dense handles; refused when the graph has no
 *                off-diagonal non-edge, and once 16 * ceil(m * n_nodes^2 / acceptable pairs) + 64 candidates have been examined
 *                (the message names the count).  m < 2^32.
 * Test hooks on HOST pointers (on_device = 0: the host build of the definitions, plain loops, usable without a GPU; otherwise
 * upload, the kernels, download): pw_selftest_score_pairs (b == NULL: a against itself; dim_b: b's row length),
 * pw_selftest_auc, pw_selftest_sample_non_edges (the CSR as host arrays, rows ascending; batch: candidates per batch of the
 * device form, 0 = the default). */
int pw_knn_score_pairs_device(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int metric,
                              double *d_score);
int pw_auc_device(int device, const double *d_pos, uint64_t m, const double *d_neg, uint64_t n, uint64_t out[2]);
int pw_sample_non_edges_device(pw_graph *g, uint32_t seed, uint64_t first_candidate, uint64_t m, uint32_t *d_u, uint32_t *d_v,
                               uint64_t *candidates_used);
int pw_selftest_score_pairs(int on_device, int device, const float *a, uint64_t na, const float *b, uint64_t nb, uint32_t dim,
                            uint32_t dim_b, const uint32_t *u, const uint32_t *v, uint64_t m, int metric, double *score);
int pw_selftest_auc(int on_device, int device, const double *pos, uint64_t m, const double *neg, uint64_t n, uint64_t out[2]);
int pw_selftest_sample_non_edges(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes,
                                 uint32_t seed, uint64_t first_candidate, uint64_t m, uint64_t batch, uint32_t *u, uint32_t *v,
                                 uint64_t *candidates_used);

/* ---- neighbourhood link-prediction baselines in device memory: common neighbours, Jaccard, preferential attachment, table sums ----
 * The definition is written at the top of csrc/nbr_scores.hip.h (DESIGN.md 4.11 repeats it); host and device answer it
 * identically, whatever the grid, the tile or the cut between the kernel's two forms.  N(x) = the entries of row x other than x
 * itself (weights are not looked at; a directed graph's out-row), d(x) = |N(x)|, C(u, v) = N(u) n N(v), cn = |C|.  Refusals:
 * PW_ERR_INVALID with a message that names the first offending element, nothing written; dense handles: PW_ERR_UNSUPPORTED.
 *   pw_nbr_degrees_device   d_deg (device uint32[n_nodes]) receives d(x).
 *   pw_nbr_scores_device    d_score[i] (device float64[m]) = the score of the pair (d_u[i], d_v[i]) (device uint32[m]) by `kind`:
 *                PW_NBR_COMMON    double(cn)
 *                PW_NBR_JACCARD   double(cn) / double(d(u) + d(v) - cn): one IEEE division, +0.0 when the denominator is 0
 *                PW_NBR_PREF      double(uint64(d(u)) * uint64(d(v))): the product exact, one rounding in the conversion
 *                PW_NBR_WEIGHTED  (((+0.0 + t[z0]) + t[z1]) + ...) over z in C ascending, one rounding per addition; t = d_table,
 *                                 device float64[n_nodes], a NaN or an infinity in it an ordinary value.  Adamic-Adar and
 *                                 resource allocation are this kind with t[z] = 1 / ln d(z) and 1 / d(z) (0.0 for d(z) < 2),
 *                                 a table the caller builds: the library evaluates no log.
 *                d_table is read by PW_NBR_WEIGHTED only (NULL there: refused) and may be NULL otherwise.  u[i] == v[i], repeated
 *                pairs and pairs that are edges are pairs like any other; m = 0 is a valid call that does nothing.  A row number
 *                >= n_nodes is refused ("u[i]" before "v[i]" at one position); an unknown kind is refused.
 * Test hooks on HOST pointers (the CSR as host arrays, rows ascending and duplicate-free; on_device = 0: the host build of the
 * definition, plain loops, usable without a GPU; otherwise upload, the kernels, download): pw_selftest_nbr_degrees and
 * pw_selftest_nbr_scores.  short_max forces the cut between the kernel's forms: a pair whose shorter row has at most short_max
 * entries is settled by one lane, the others by the whole wavefront -- 0 sends every pair to the wavefront, 0xFFFFFFFF leaves
 * every pair with its lane, -1 selects the library's default.  No result depends on it.
 * pw_nbr_scores_device_cut is pw_nbr_scores_device with that cut forced and, when kernel_ms is not NULL, the device time of the
 * score kernel alone (two events around it) in ms: the measurement hook of tools/nbr_bench.py. */
enum { PW_NBR_COMMON = 0, PW_NBR_JACCARD = 1, PW_NBR_PREF = 2, PW_NBR_WEIGHTED = 3 };
int pw_nbr_degrees_device(pw_graph *g, uint32_t *d_deg);
int pw_nbr_scores_device(pw_graph *g, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int kind, const double *d_table,
                         double *d_score);
int pw_nbr_scores_device_cut(pw_graph *g, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int kind, const double *d_table,
                             double *d_score, int64_t short_max, float *kernel_ms);
int pw_selftest_nbr_scores(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes,
                           const uint32_t *u, const uint32_t *v, uint64_t m, int kind, const double *table, int64_t short_max,
                           double *score);
int pw_selftest_nbr_degrees(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes,
                            uint32_t *deg);

/* ---- exact binary logistic regression on embedding rows and pair operators: one evaluation, in device memory ------------
 * The definition is written at the top of csrc/logit.hip.h (DESIGN.md 4.12 repeats it); host and device answer it identically,
 * bit for bit, whatever the grid.  a, b: two pw_knn indexes of one dim <= 512 on one device (b == NULL: a against itself).
 * Sample i has the feature f = feat(op, a[d_u[i]], b[d_v[i]]) in float64:
 *                PW_LOGIT_ROW       a's row as it is (d_v is not read and may be NULL): node classification
 *                PW_LOGIT_AVERAGE   (a + b) * 0.5
 *                PW_LOGIT_HADAMARD  a * b
 *                PW_LOGIT_L1        fabs(a - b)
 *                PW_LOGIT_L2        (a - b) * (a - b)
 * and the decision value z[i] = (((bias + w[0] f[0]) + w[1] f[1]) + ...), theta = (w[0] .. w[dim - 1], bias) float64[dim + 1] in
 * HOST memory, every product and sum rounded on its own.
 *   pw_logit_eval_device   d_u, d_v device uint32[m], d_y device uint8[m] of 0 / 1, 1 <= m < 2^40, l2 finite and >= 0.
 *                *loss = mean log-loss + (0.5 l2) |w|^2 and grad[dim + 1] (HOST memory) = its gradient (the bias is not
 *                penalised), summed in the definition's order: 1024-sample chunks, ascending.  d_z (device float64[m], may be
 *                NULL) receives the decision values.  With d_y == NULL the call computes d_z alone (loss and grad are not
 *                touched): scoring with a trained model.  The library evaluates no libm exp or log: the definition carries its
 *                own two functions, built from + - * / alone.
 *                Refused with PW_ERR_INVALID and a message naming the first offending element, NOTHING written: an unknown op,
 *                dims or devices of a and b that differ, m out of range, l2 negative / NaN / infinite, a non-finite theta entry,
 *                a row number out of range ("u[i]" before "v[i]" at one position), a label other than 0 / 1, a z that is not
 *                finite.  dim > 512: PW_ERR_UNSUPPORTED.
 *   pw_logit_eval_device_grid   the same with the grid of both kernels forced to `blocks` workgroups (-1: the default) and, when
 *                kernel_ms is not NULL, the device time of the kernels (two events around them) in ms: the hook of the tests
 *                and of tools/logit_bench.py.  No result depends on blocks.
 * Test hooks on HOST pointers: pw_selftest_logit (a float32[na, dim], b float32[nb, dim] or NULL; y == NULL: z alone; on_device = 0:
 * the host build of the definition, plain loops, usable without a GPU; otherwise upload, the kernels, download) and
 * pw_selftest_logit_math (the host build of the definition's lg_exp (which = 0) or lg_log1p (which = 1) on an array). */
enum { PW_LOGIT_ROW = 0, PW_LOGIT_AVERAGE = 1, PW_LOGIT_HADAMARD = 2, PW_LOGIT_L1 = 3, PW_LOGIT_L2 = 4 };
int pw_logit_eval_device(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, const uint8_t *d_y, uint64_t m, int op,
                         const double *theta, double l2, double *loss, double *grad, double *d_z);
int pw_logit_eval_device_grid(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, const uint8_t *d_y, uint64_t m,
                              int op, const double *theta, double l2, double *loss, double *grad, double *d_z, int blocks,
                              float *kernel_ms);
int pw_selftest_logit(int on_device, int device, const float *a, uint64_t na, const float *b, uint64_t nb, uint32_t dim,
                      const uint32_t *u, const uint32_t *v, const uint8_t *y, uint64_t m, int op, const double *theta, double l2,
                      int blocks, double *loss, double *grad, double *z);
int pw_selftest_logit_math(int which, const double *x, uint64_t n, double *out);

/* ---- edges held out by the seeded stream: the train graph and the held-out pairs, in device memory ----------------------
 * The definition is written at the top of csrc/holdout.hip.h (DESIGN.md 4.10 repeats it); host and device answer it
 * identically, whatever the grid or the batch of words expanded at a time.
 *   pw_holdout_edges_device   g: a CSR handle (dense: PW_ERR_UNSUPPORTED), not modified.  w = the words of RandomState(seed)
 *                (pw_mt_words).  directed = 1: every entry r -> c, r != c, is a unit; directed = 0: the CSR must be symmetric
 *                (the first entry position without its mate c -> r is refused with PW_ERR_INVALID naming it, nothing written
 *                or allocated), a unit is an entry with r < c and its mate shares its fate.  Self loops always stay.  With
 *                protect = 1 the unit at the first non-loop entry of a row -- for an undirected unit, of either of its two
 *                rows -- is protected: every row that had a non-loop entry keeps one.  The unit at entry position e is held
 *                out iff w[first_word + e] < threshold and it is not protected; first_word < 2^60.
 *                *train = the CSR of the entries not held out, in order, data carried over (pw_csr_dev_shape / _export /
 *                pw_csr_create_device / pw_csr_dev_destroy apply; insertions, dropped and build_ms are 0); *held = the held-out
 *                list in ascending unit position.  A later call at first_word + nnz draws an independent split.  stage_ms
 *                (may be NULL; its synchronisations make the call a little slower): the wall clock of the word expansion, the
 *                flag kernels, and the scans with the compactions, in ms.
 *   pw_holdout_dev_shape    held units, units, protected units (any may be NULL)
 *   pw_holdout_dev_fill     u, v (u < v when undirected, (r, c) when directed) and weight (the float32 of the unit's own entry,
 *                1.0 for a graph without data) into device arrays of the handle's device with room for `held` elements
 * Test hook on HOST pointers: pw_selftest_holdout_edges (on_device = 0: the host build of the definition, plain loops, usable
 * without a GPU; otherwise upload, the kernels with `batch` words per expansion -- 0 = the default --, download).  data may be
 * NULL (every weight 1.0).  out_indptr: n_nodes + 1 cells; out_indices, out_data (may be NULL), u, v, weight: room for nnz.
 * counts = {train entries, held units, units, protected units}. */
typedef struct pw_holdout_dev pw_holdout_dev;
int pw_holdout_edges_device(pw_graph *g, int directed, uint32_t seed, uint64_t first_word, uint32_t threshold, int protect,
                            pw_csr_dev **train, pw_holdout_dev **held, double stage_ms[3]);
int pw_holdout_dev_shape(const pw_holdout_dev *h, uint64_t *held, uint64_t *units, uint64_t *protected_units);
int pw_holdout_dev_fill(const pw_holdout_dev *h, uint32_t *d_u, uint32_t *d_v, float *d_weight);
void pw_holdout_dev_destroy(pw_holdout_dev *h);
int pw_selftest_holdout_edges(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, const float *data,
                              uint32_t n_nodes, int directed, uint32_t seed, uint64_t first_word, uint32_t threshold, int protect,
                              uint64_t batch, uint32_t *out_indptr, uint32_t *out_indices, float *out_data, uint32_t *u,
                              uint32_t *v, float *weight, uint64_t counts[4]);

/* ---- random stream service (host side; usable without a GPU) ---------------------------- */
/* doubles #offset.. of RandomState(seed).random_sample, produced with MT19937 jump-ahead. */
int pw_mt_random_sample(uint32_t seed, uint64_t offset, uint64_t n, double *out);

/* Test hook: the same doubles as the DEVICE produces them for a walk call (jump-ahead tree + expansion kernels on the
 * handle's GPU), copied to the host -- lets the tests compare the device stream with pw_mt_random_sample / NumPy at
 * the offsets the last shards of a multi-GPU run start from. */
int pw_stream_sample_device(pw_graph *g, uint32_t seed, uint64_t offset, uint64_t n, double *out);
/* The tempered 32-bit words #offset.. of the same stream (random_sample takes them two at a time:
 * ((w[2i] >> 5) * 2^26 + (w[2i+1] >> 6)) / 2^53; RandomState(seed).randint(0, 2**32, size=n, dtype=np.uint64) hands them
 * out one by one), with jump-ahead: what the seeded alias / first-order modes draw from.  Host side, no GPU needed. */
int pw_mt_words(uint32_t seed, uint64_t offset, uint64_t n, uint32_t *out);
/* Test hook: the same words as the DEVICE expands them (jump-ahead tree + mt_words_kernel on the handle's GPU). */
int pw_stream_words_device(pw_graph *g, uint32_t seed, uint64_t offset, uint64_t n, uint32_t *out);

/* ---- seeded alias / first-order modes: the word offsets of the jobs, by speculation rounds (host form) -------------------- */
/* With a seed PW_MODE_PRECOMP, _FIRST_ORDER_UNWEIGHTED and _PRECOMP_FIRST_ORDER reproduce the reference's ONE stream, which
 * hands every step a variable number of words: the word offset at which a job starts depends on every earlier draw, and that
 * one integer per job is all that is sequential.  csrc/seq_spec.h finds the offsets of many jobs per round: it walks
 * candidate (job, offset) pairs in windows around the expected offsets, resolves the chain that starts at the round's exact
 * base by pointer doubling and commits the jobs on it -- exact by construction, whatever the fields below say.  The rounds
 * have a host form only (pw_selftest_seq_offsets, pw_selftest_seq_walks); on the device seeded calls of these modes walk on
 * one lane (walk_seq_kernel). */
typedef struct pw_seq_config {  /* 0 in a field = the default */
    uint32_t jobs_per_round;     /* windows planned per round (default 512, at most 4096) */
    uint32_t max_candidates;     /* cap on the candidates of a round (default 2^19); the round plans the jobs that fit */
    uint32_t word_buffer_blocks; /* size of the word buffer in blocks of 624 words (default 65536); raised to the smallest
                                    legal size, which holds one job of 3 * walk_length + 4096 words */
    uint64_t min_jobs;           /* calls with fewer jobs take the plain sequential loop; UINT64_MAX: always */
    float window_sigmas;         /* half width of a window in deviations of the words per job (default 3); negative: the
                                    centre candidate alone, nearly every window misses (tests) */
    float force_mean;            /* > 0: words per job the windows are centred with, in place of the running mean (tests) */
    float force_sigma;           /* > 0: in place of the running deviation */
} pw_seq_config;
typedef struct pw_seq_info {
    uint32_t path;               /* 0 sequential loop, 1 speculative, 2 speculative then fell back (a job that did not finish
                                    inside a full word buffer starting at its own block) */
    uint64_t rounds;             /* rounds that committed jobs */
    uint64_t candidate_walks, committed_jobs;
    uint64_t window_misses;      /* rounds whose chain ended at an offset outside the next window */
    uint64_t unfinished_retries; /* rounds repeated behind a larger expansion: their first job had run out of words */
    uint64_t words_consumed;     /* by the whole call: where job n_jobs would start */
    uint64_t words_expanded;
    double plan_ms;              /* host clock of the planning */
    double candidate_ms, resolve_ms, commit_ms, expand_ms;   /* device time of the phases: 0 in the host form */
} pw_seq_info;
/* Test hook (host, no GPU): the plan, candidate, resolve and commit logic of the rounds for FirstOrderUnweighted on a host
 * CSR, the same headers built for the host with the words of pw_mt_words.  offsets[i] = the word job i starts at,
 * offsets[n_jobs] = the words consumed.  cfg->min_jobs = UINT64_MAX: a plain sequential loop instead. */
int pw_selftest_seq_offsets(const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, const uint32_t *starts,
                            uint64_t n_jobs, uint32_t walk_length, uint32_t seed, const pw_seq_config *cfg, uint64_t *offsets,
                            pw_seq_info *info);
/* Test hook (host, no GPU): the same rounds for any of the three modes on a host CSR (data NULL: all 1.0) and, for PW_MODE_PRECOMP
 * and PW_MODE_PRECOMP_FIRST_ORDER, caller-built alias tables in pw_precomp_export's layout (first order: alias_indptr = indptr
 * widened).  out (optional): uint32[n_jobs][walk_length + 2], the walk matrix of pw_simulate; counts (optional): total_steps,
 * overflow_reads, clamped_reads, dead_end_walks of pw_stats.  cfg->min_jobs = UINT64_MAX: the plain sequential loop. */
int pw_selftest_seq_walks(int mode, const uint32_t *indptr, const uint32_t *indices, const float *data, uint32_t n_nodes,
                          const uint64_t *alias_indptr, const uint32_t *alias_j, const float *alias_q, uint64_t n_alias,
                          const uint32_t *starts, uint64_t n_jobs, uint32_t walk_length, uint32_t seed, const pw_seq_config *cfg,
                          uint64_t *offsets, uint32_t *out, uint64_t *counts, pw_seq_info *info);

/* ---- node2vec+ noisy-edge thresholds (host side; usable without a GPU) --------------------- */
/* thr[i] = max(mean(row i) + gamma * std(row i), 0) exactly as the reference's NumPy expression evaluates it
 * (rw/sparse_rw.py:22-35 on float32 CSR rows; rw/dense_rw.py:11-19 on the non-zero entries of float64 rows):
 * NumPy's pairwise summation, every step in the array's precision.  Rows without entries give NaN, as there.
 * The result is what pw_graph_set_thresholds() expects. */
int pw_noise_thresholds_csr(const uint32_t *indptr, const float *data, uint32_t n_nodes, double gamma, float *thr);
int pw_noise_thresholds_dense(const double *data, uint32_t n_nodes, double gamma, float *thr);
/* The dense formula over a float32 CSR (data NULL: every weight 1.0): what pw_noise_thresholds_dense gives for its float64
 * dense form -- the row's non-zeros widened to float64 in column order.  The thresholds of PW_MODE_SPARSE_NODE2VEC_PLUSPLUS. */
int pw_noise_thresholds_csr_f64(const uint32_t *indptr, const float *data, uint32_t n_nodes, double gamma, float *thr);
/* pw_noise_thresholds_csr evaluates mean + gamma * std as NumPy >= 2 does (float32 throughout); this variant as NumPy
 * 1.x does (the reference pins numpy==1.23.2: float32 scalar * Python float -> float64, one rounding on store).  They
 * differ by an ulp when gamma * std is not exact in float32 (gamma = 0.1, ...); the Python layer picks the one that
 * matches the installed NumPy, i.e. what the reference's expression would give in the same environment. */
int pw_noise_thresholds_csr_numpy1(const uint32_t *indptr, const float *data, uint32_t n_nodes, double gamma, float *thr);
/* Test hook: the dense formula for ONE row of n values (a row's non-zeros in column order) as the device computes it in
 * pw_dense_noise_thresholds -- the host build of the same routine (csrc/dense_build.hip.h: threshold_row). */
int pw_selftest_thresholds_row(const double *row, uint64_t n, double gamma, float *thr);

/* ---- edge-list ingestion (host side; usable without a GPU) -------------------------------- */
/* Fast path of AdjlstGraph.read + to_csr (reference src/pecanpy/graph.py:270-341): parses a 2- or
 * 3-column edge list into the reference's CSR (vertices numbered by first appearance, rows ascending,
 * float32 weights, last duplicate wins) and the vertex-ID table.
 * Returns PW_OK, PW_ERR_INVALID (file cannot be read), or PW_ERR_UNSUPPORTED when the file needs the
 * statement-by-statement reader to reproduce Python-level behaviour (malformed line, non-positive or
 * exotic weight literal, conflicting duplicate edge -- the cases where the reference warns or raises --
 * or non-ASCII bytes); the caller then falls back to it.  The handle owns the arrays until destroyed. */
typedef struct pw_edgelist pw_edgelist;
int pw_edgelist_read(const char *path, int weighted, int directed, const char *delimiter, pw_edgelist **out);
/* n_nodes, nnz (distinct directed edges), insertions (the reference's num_edges counter), id_bytes */
int pw_edgelist_shape(const pw_edgelist *e, uint64_t *n_nodes, uint64_t *nnz, uint64_t *insertions,
                      uint64_t *id_bytes);
/* indptr uint32[n_nodes+1], indices uint32[nnz], data float32[nnz] (the CSR of to_csr), data64
 * float64[nnz] (the weights as parsed: AdjlstGraph.to_dense keeps float64), id_offsets uint64[n_nodes+1],
 * id_chars char[id_bytes] (vertex i's ID = id_chars[id_offsets[i] : id_offsets[i+1]]); NULL = skip */
int pw_edgelist_export(const pw_edgelist *e, uint32_t *indptr, uint32_t *indices, float *data,
                       double *data64, uint64_t *id_offsets, char *id_chars);
void pw_edgelist_destroy(pw_edgelist *e);

/* ---- edge-list ingestion on the device (csrc/edgelist_dev.hip.h) ------------------------------------------------------------
 * pw_edgelist_read's result -- the reference's CSR, vertices numbered by first appearance -- with the text of the file
 * uploaded, tokenised and numbered in device memory and the CSR built there (pw_coo_to_csr_device's build; the float64 weights
 * as parsed decide whether a repeated pair conflicts, the entries hold them rounded once to float32).  The reader accepts a
 * SUBSET of what pw_edgelist_read accepts.  Return value:
 *   PW_EDGELIST_OK                 *csr = the CSR (pw_csr_dev_shape / _export / _destroy, pw_csr_create_device), *ids = the names
 *   PW_EDGELIST_NEEDS_HOST_READER  no error: the caller takes pw_edgelist_read's route.  Everything pw_edgelist_read declines
 *                                  (see there), and: a weight literal outside  [+-]digits[.digits][e[+-]digits]  with at most 15
 *                                  significand digits behind the leading zeros and a power of ten, fraction digits taken off,
 *                                  within +-22 (the class one correctly rounded float64 operation evaluates); a delimiter of
 *                                  more than 16 bytes; an empty file; a file of 4 GiB or more; 2^32 - 1 or more insertions;
 *                                  scratch that does not fit in device (or host) memory
 *   PW_EDGELIST_IO                 the file cannot be opened or read (the caller's own open then raises what Python raises)
 *   < 0                            PW_ERR_*: no device, a HIP error
 * Nothing stays allocated unless PW_EDGELIST_OK is returned.  stats (may be NULL; zeroed unless OK): wall clock of the stages,
 * each ended by a wait for the device -- upload_ms (file -> pinned staging -> device text), scan_ms (byte classes, line
 * starts, per-line records), ids_ms (id table, numbering, the names' spans), build_ms (the CSR build, allocations included;
 * pw_csr_dev_shape has its kernels' time) -- and lines, n_nodes, file_bytes.
 *   pw_edgelist_ids_shape   n_nodes, id_bytes (the names' characters in all)
 *   pw_edgelist_ids_export  pw_edgelist_export's layout: id_offsets uint64[n_nodes + 1], id_chars char[id_bytes], vertex v's
 *                           name = id_chars[id_offsets[v] : id_offsets[v + 1]], sliced from the bytes the call read
 * pw_edgelist_read_device_ex is the same call with a flags word (unknown bits: PW_ERR_INVALID); pw_edgelist_read_device is
 * flags = 0.
 *   PW_EDGELIST_KEEP_F64    a weighted file's CSR also keeps, per entry, the winning line's float64 weight exactly as parsed (8
 *                           more bytes per entry, written by the launch that writes the float32 data, which stays bit for bit).
 *                           pw_dense_create_from_csr then stores those values instead of the widened float32 ones: the handle of
 *                           the reference's to_dense(), which keeps the Python float.  Without the bit, and for an unweighted
 *                           file, nothing more is allocated.
 *   pw_csr_dev_export_f64   test hook: data64 float64[nnz] = those weights; PW_ERR_UNSUPPORTED when the CSR holds none (built by
 *                           pw_coo_to_csr_device, read without the bit, or from an unweighted file) */
enum { PW_EDGELIST_OK = 0, PW_EDGELIST_NEEDS_HOST_READER = 1, PW_EDGELIST_IO = 2 };
enum { PW_EDGELIST_KEEP_F64 = 1 };
typedef struct pw_edgelist_dev_stats {
    double upload_ms, scan_ms, ids_ms, build_ms;
    uint64_t lines, n_nodes, file_bytes;
} pw_edgelist_dev_stats;
typedef struct pw_edgelist_ids pw_edgelist_ids;
int pw_edgelist_read_device(const char *path, int weighted, int directed, const char *delimiter, int device, pw_csr_dev **csr,
                            pw_edgelist_ids **ids, pw_edgelist_dev_stats *stats);
int pw_edgelist_read_device_ex(const char *path, int weighted, int directed, const char *delimiter, int device, uint32_t flags,
                               pw_csr_dev **csr, pw_edgelist_ids **ids, pw_edgelist_dev_stats *stats);
int pw_csr_dev_export_f64(const pw_csr_dev *c, double *data64);
int pw_edgelist_ids_shape(const pw_edgelist_ids *ids, uint64_t *n_nodes, uint64_t *id_bytes);
int pw_edgelist_ids_export(const pw_edgelist_ids *ids, uint64_t *id_offsets, char *id_chars);
void pw_edgelist_ids_destroy(pw_edgelist_ids *ids);
/* Host builds of the reader's text routines, no GPU needed.  Both return 1 (accepted), 0 (declined) or PW_ERR_INVALID.
 *   pw_selftest_edgelist_weight  el_parse_weight on text[0, n): *value = the float64 (sign applied; the reader itself
 *                                declines what is not > 0)
 *   pw_selftest_edgelist_line    el_tokenize_line on the line text[lo, hi) (without its newline): *n_terms =
 *                                len(line.strip().split(delimiter)); spans uint32[10] = (offset, length) of the first three
 *                                terms, then of terms[0].strip() and terms[1].strip(); *weight (1.0 when unweighted) */
int pw_selftest_edgelist_weight(const char *text, uint64_t n, double *value);
int pw_selftest_edgelist_line(const char *text, uint64_t lo, uint64_t hi, const char *delimiter, int weighted, uint32_t *n_terms,
                              uint32_t *spans, double *weight);

/* ---- a walk corpus file read on the device (csrc/corpus_dev.hip.h) -----------------------------------------------------------
 * The inverse of pw_walks_write_text_device: the text of a corpus file (one walk per line, names separated by white space) is
 * uploaded and tokenised in device memory, the names are numbered by first appearance with the edge-list reader's id table,
 * and the walk matrix uint32[n_rows, width] is laid out as pw_sgns_train_device and pw_walks_write_text_device take it: row r =
 * the numbers of line r's tokens, zeros, and in the last cell the token count; width = the most tokens in a line (at least 1)
 * + 1, i.e. walk_length = width - 2.  The byte definition is pecanpy_amd.corpus.read_walks.  Return value:
 *   PW_EDGELIST_OK                 *out = the matrix (pw_corpus_dev_shape / _fill / _export / _destroy), *ids = the names in
 *                                  first-appearance order (pw_edgelist_ids_shape / _export / _destroy)
 *   PW_EDGELIST_NEEDS_HOST_READER  no error: the caller reads the file on the host.  A byte outside {\t, \n, \r, 0x20 .. 0x7E}
 *                                  (\v, \f, 0x1C .. 0x1F, NUL, 0x7F, everything from 0x80 up); an empty file; a file of 4 GiB or
 *                                  more; scratch or a matrix that does not fit in device (or host) memory
 *   PW_EDGELIST_IO                 the file cannot be opened or read
 *   < 0                            PW_ERR_*: no device, a HIP error
 * Space, \t and \r separate tokens, \n ends a line; a last line without a newline counts, an empty line is a row of count 0.
 * Nothing stays allocated unless PW_EDGELIST_OK is returned.  stats (may be NULL; zeroed unless OK): wall clock of the stages,
 * each ended by a wait for the device -- upload_ms (file -> pinned staging -> device text), scan_ms (byte classes, newline and
 * token-start counts, their scans, token offsets / lines, the width), tokens_ms (token records, id table, numbering), fill_ms
 * (the matrix, the names' spans) -- and file_bytes, lines, tokens, names.
 *   pw_corpus_dev_shape    n_rows, width, n_tokens (any may be NULL)
 *   pw_corpus_dev_fill     the matrix into d_out, a device buffer of the handle's device with room for n_rows * width words
 *                          (a torch tensor's storage); complete when the call returns
 *   pw_corpus_dev_export   the same words to host memory */
typedef struct pw_corpus_dev_stats {
    double upload_ms, scan_ms, tokens_ms, fill_ms;
    uint64_t file_bytes, lines, tokens, names;
} pw_corpus_dev_stats;
typedef struct pw_corpus_dev pw_corpus_dev;
int pw_corpus_read_device(const char *path, int device, pw_corpus_dev **out, pw_edgelist_ids **ids, pw_corpus_dev_stats *stats);
int pw_corpus_dev_shape(const pw_corpus_dev *c, uint64_t *n_rows, uint64_t *width, uint64_t *n_tokens);
int pw_corpus_dev_fill(const pw_corpus_dev *c, uint32_t *d_out);
int pw_corpus_dev_export(const pw_corpus_dev *c, uint32_t *h_out);
void pw_corpus_dev_destroy(pw_corpus_dev *c);

/* ---- self test hooks (host only, no GPU needed -- except pw_selftest_lane with on_device) -- */
/* Runs the binade-scan emulation of csrc/seqscan.h on a host array: returns through *index the
 * position np.searchsorted(np.cumsum(x), r) would return under sequential float32 semantics
 * (n if never reached) and through *sum the sequential float32 sum.  chunk = elements per pass. */
int pw_selftest_seqscan_f32(const float *x, uint32_t n, double r, int use_target, uint32_t chunk,
                            uint32_t *index, float *sum);
int pw_selftest_seqscan_f64(const double *x, uint32_t n, double r, int use_target, uint32_t chunk,
                            uint32_t *index, double *sum);

/* Exact-arithmetic decision of the float32 CDF search used by the unit-weight walk step (csrc/seqscan.h:
 * exact_thresholds_f32), on a host row: cls[k] = 0 (other neighbour, weight w_out), 1 (common neighbour,
 * weight 1) or 2 (prev, weight w_prev); w_out, w_prev powers of two.  For every r[i]: chain[i] = what the
 * reference's np.searchsorted(np.cumsum(w / w.sum()), r) returns under sequential float32 semantics
 * (pecanpy.py:556-557; n if never reached), exact[i] = the index decided in integer arithmetic, or
 * 0xffffffff when a partial sum lies inside the drift bound (the kernel then runs the float chain). */
int pw_selftest_exact_decision(const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r,
                               uint32_t n_r, uint32_t *chain, uint32_t *exact);
/* The same decision as one thread of the lane kernel takes it, from the ascending positions of the common neighbours
 * (csrc/seqscan.h: lane_decide -> lane_tight -> lane_chain), beside the sequential float32 chain:
 *   chain[i]      = np.searchsorted(np.cumsum(float32 probs), r[i]) (n if never reached),
 *   lane[i]       = lane_decide: decided index, 0xfffffffd when a partial sum of the exact CDF lies inside the a-priori
 *                   drift bound (then kmax[i] = number of leading positions the chain may need: chain[i] < kmax[i] or
 *                   chain[i] == n), 0xfffffffc when the row is outside the exact range,
 *   tight[i]      = lane[i] when that is decided, else the list-free interval decision (lane_tight: the chain's
 *                   systematic drift bounded from the class counts lane_decide already knows): index or 0xfffffffd,
 *   chain_lane[i] = (may be NULL) the float32 chain as ONE thread evaluates it (lane_chain) over the first kmax[i]
 *                   positions (the whole row when lane[i] is decided): position, 0xfffffffb when that prefix never
 *                   reaches r[i], 0xfffffffa on a rounding tie the thread cannot afford.
 * on_device != 0: every target is decided by one thread of a kernel on `device` (the sequential chain included), i.e.
 * by the code the walk kernels run -- device code generation, v_rcp_f32 -- instead of the host build of the same
 * routines.  Rows of more than 65536 entries use uint32 positions, shorter ones uint16 (the lane index's formats). */
int pw_selftest_lane(int on_device, int device, const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r,
                     uint32_t n_r, uint32_t *chain, uint32_t *lane, uint32_t *kmax, uint32_t *tight, uint32_t *chain_lane);
/* The step of the lane kernel's FLOATS form (unit weights, 1/p or 1/q NOT a power of two: w_out, w_prev arbitrary
 * positive float32): chain[i] = the reference's position (sequential float32 w.sum(), w / tot, cumsum, searchsorted),
 * lane[i] = the same from two closed-form chains of one thread (lane_chain with r = +inf for the total, then the
 * search; 0xfffffffb never reached, 0xfffffffa rounding-tie budget), tots[2 i] / tots[2 i + 1] = the sequential row
 * total / the thread's.  on_device: one GPU thread per target. */
int pw_selftest_lane_floats(int on_device, int device, const uint8_t *cls, uint32_t n, float w_out, float w_prev,
                            const double *r, uint32_t n_r, uint32_t *chain, uint32_t *lane, float *tots);
/* The bounded decision of that step alone (csrc/seqscan.h: lane_decide_unit_bounded, round 5 -- the real prefix sums of the
 * three row values in closed form + a rigorous bound on the float32 chain's drift), host only, given the row's sequential
 * float32 total: lane[i] = the position, n (never reached) or 0xfffffffd (left open: the chain decides); chain[i] = the
 * reference's position (n: never reached).  Fails when a k_safe lies beyond the reference's position. */
int pw_selftest_lane_unit_bounded(const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r, uint32_t n_r,
                                  uint32_t *chain, uint32_t *lane);
/* ... with the interval decision of round 6 in front of the chain (csrc/seqscan.h: lane_tight_values -- the float32 chain's
 * systematic drift bounded from the class counts the bounded decision already has, for arbitrary float32 values):
 * tight[i] = lane[i] when that is a verdict, else the interval decision's position or 0xfffffffd (left to the float chain). */
int pw_selftest_lane_unit_tight(const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r, uint32_t n_r,
                                uint32_t *chain, uint32_t *lane, uint32_t *tight);
/* The lane kernel's decision for WEIGHTED rows (csrc/seqscan.h: lane_decide_weighted: float64 prefix sums of the step's
 * values with a rigorous bound on the float32 chain's drift), host only.  vals[k] = the step's value of neighbour k
 * before normalisation (what get_normalized_probs holds at sparse_rw.py:87 / :126), base[k] = its value as a plain
 * "out" neighbour, cls[k] = 0 other (vals == base) / 1 common neighbour of prev and cur / 2 prev.  chain[i] = the
 * reference's position for draw r[i] (sequential float32 w.sum(), w / tot, cumsum, searchsorted; n: never reached),
 * lane[i] = the decision: the same position, or 0xfffffffd when a partial sum lies within the bound of the draw (the
 * step then takes the wave-per-walk scan). */
int pw_selftest_lane_weighted(const float *vals, const float *base, const uint8_t *cls, uint32_t n, const double *r,
                              uint32_t n_r, uint32_t *chain, uint32_t *lane);
/* float64 flavour (DenseOTF column-space kernel, dense_rw.py:34-72 semantics; exact_thresholds_f64). */
int pw_selftest_exact_decision_f64(const uint8_t *cls, uint32_t n, double w_out, double w_prev, const double *r,
                                   uint32_t n_r, uint32_t *chain, uint32_t *exact);

#ifdef __cplusplus
}
#endif
#endif
