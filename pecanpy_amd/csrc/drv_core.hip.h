#pragma once
// Host driver, core: what every other piece stands on -- PW_EXPORT, the error text (fail, HIP_TRY), the switches of a call
// (LaneSwitches), grow, check_device, the evaluation drivers' helpers (dev_alloc .. download), the handles (GraphDesc / GraphData /
// pw_graph, pw_csr_dev) and their owners, csr_dev, graph_common_init, the declaration of stream_words_window (pecanpy_amd.hip).
// Exports pw_version, pw_last_error, pw_device_count, pw_warmup, pw_graph_destroy.  The system includes of the whole driver
// are here and nowhere else.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <unistd.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <random>
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pecanpy_amd.h"
#include "counters.h"
#include "devmem.hpp"
#include "seqscan.h"            // PrefixPair in GraphData; Binade for seqscan_emulate
#include "walk_sparse.hip.h"    // ELine in GraphData; CsrDev for csr_dev
#include "walk_lanes.hip.h"     // SuspRec, VerRec: the queues and records of pw_graph

#define PW_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_err;

using pw::N_COUNTERS;   // (pw_graph::counters: counters.h)

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// opt-in switches documented as NAME=1: on when set to a non-zero number (NAME=0 and an empty value leave them off)
bool env_on(const char *name) {
    const char *v = getenv(name);
    return v != nullptr && atoi(v) != 0;
}

// Behaviour switches of the lane path and the call driver.  read_lane_switches() is the one place that reads them, once at
// the top of a call (pw_simulate_device; pw_csr_create for NO_LANES) -- never kept across calls: tests set and clear them
// between the calls of one process -- and the struct is passed down.
struct LaneSwitches {
    bool has_chain_tail; uint64_t chain_tail;   // PECANPY_AMD_CHAIN_TAIL=<walks>: set at all, its number
    bool no_chain_queue;                     // PECANPY_AMD_NO_CHAIN_QUEUE (set at all)
    int lane_chains;                         // PECANPY_AMD_LANE_CHAINS=0/1: -1 when unset
    uint64_t late_chains;                    // PECANPY_AMD_LATE_CHAINS=<resumed walks per resident lane> (default 16; 0: never)
    bool verify_tight, verify_tight_poison;  // PECANPY_AMD_VERIFY_TIGHT (set at all), =poison
    uint32_t verify_sample;                  // PECANPY_AMD_VERIFY_SAMPLE=N as given (default 1024; 0: off)
    bool verify_sample_poison;               // PECANPY_AMD_VERIFY_SAMPLE_POISON (set at all)
    bool has_verify_cap; uint64_t verify_cap;   // PECANPY_AMD_VERIFY_CAP=<records>: set at all, its number
    bool no_lanes, no_wlanes, no_twin, force_tot;   // PECANPY_AMD_NO_LANES / _NO_WLANES / _NO_TWIN / _FORCE_TOT (set at all)
    bool debug_rounds;                       // PW_DEBUG_ROUNDS (set at all)
};

LaneSwitches read_lane_switches() {
    const char *tail = getenv("PECANPY_AMD_CHAIN_TAIL"), *chains = getenv("PECANPY_AMD_LANE_CHAINS"), *late = getenv("PECANPY_AMD_LATE_CHAINS");
    const char *tight = getenv("PECANPY_AMD_VERIFY_TIGHT"), *sample = getenv("PECANPY_AMD_VERIFY_SAMPLE"), *cap = getenv("PECANPY_AMD_VERIFY_CAP");
    LaneSwitches sw;
    sw.has_chain_tail = tail != nullptr;   sw.chain_tail = tail ? (uint64_t)strtoull(tail, nullptr, 10) : 0;
    sw.no_chain_queue = getenv("PECANPY_AMD_NO_CHAIN_QUEUE") != nullptr;
    sw.lane_chains = chains ? (atoi(chains) != 0 ? 1 : 0) : -1;
    sw.late_chains = late ? (uint64_t)strtoull(late, nullptr, 10) : 16ull;
    sw.verify_tight = tight != nullptr;    sw.verify_tight_poison = tight && strcmp(tight, "poison") == 0;
    sw.verify_sample = sample ? (uint32_t)strtoul(sample, nullptr, 10) : 1024u;
    sw.verify_sample_poison = getenv("PECANPY_AMD_VERIFY_SAMPLE_POISON") != nullptr;
    sw.has_verify_cap = cap != nullptr;    sw.verify_cap = cap ? (uint64_t)strtoull(cap, nullptr, 10) : 0;
    sw.no_lanes = getenv("PECANPY_AMD_NO_LANES") != nullptr;   sw.no_wlanes = getenv("PECANPY_AMD_NO_WLANES") != nullptr;
    sw.no_twin = getenv("PECANPY_AMD_NO_TWIN") != nullptr;     sw.force_tot = getenv("PECANPY_AMD_FORCE_TOT") != nullptr;
    sw.debug_rounds = getenv("PW_DEBUG_ROUNDS") != nullptr;
    return sw;
}

// The weighted lane form takes a job array only when its rounds have a queue -- the in-place form can do nothing with a
// step it cannot decide (first steps included) but hand the walk to walk_kernel: more walks than the tail at which its
// rounds stop queueing (PECANPY_AMD_CHAIN_TAIL, or WLANES_TAIL: plan_lane_call), and not with PECANPY_AMD_NO_CHAIN_QUEUE.
constexpr uint64_t WLANES_TAIL = 8192;
bool wlanes_worth(const LaneSwitches &sw, uint64_t n_jobs) {
    return n_jobs > (sw.has_chain_tail ? sw.chain_tail : WLANES_TAIL) && !sw.no_chain_queue;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(PW_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
    } while (0)

using pw::DevBuf;      // (devmem.hpp: every device allocation of the host driver lives in one, pinned host memory in a PinnedBuf)
using pw::PinnedBuf;

// scratch that is reused across calls: grown on demand, PW_ERR_NOMEM when the device has no room for it
template <typename T> int grow(DevBuf<T> &b, size_t n) {
    const hipError_t e = b.ensure(n);
    return e == hipSuccess ? 0 : fail(PW_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
}

// the one device check of every entry that takes a device index
int check_device(int device) {
    const int n = pw_device_count();
    if (n <= 0) return fail(PW_ERR_NO_DEVICE, "no HIP device visible (libpecanpy_amd needs a GPU; there is no CPU fallback)");
    if (device < 0 || device >= n) return fail(PW_ERR_INVALID, "device index out of range");
    return 0;
}

// ---- what the evaluation drivers (drv_knn, drv_linkpred, drv_nbr, drv_logit, drv_holdout) share --------------------------------
// a fresh allocation of a call.  ("pw_knn:" whichever family asks: where the function began; a known wart)
template <typename T> int dev_alloc(DevBuf<T> &b, size_t n) {
    const hipError_t e = b.alloc(n);
    return e == hipSuccess ? 0 : fail(PW_ERR_NOMEM, "pw_knn: " + std::to_string(n * sizeof(T)) + " bytes do not fit in device memory: " + hipGetErrorString(e));
}

// the grid of a 256-thread kernel whose threads stride over n items: a thread per item up to 16 workgroups per CU
unsigned strided_grid(uint64_t n, int n_cu) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)std::max(1, n_cu) * 16)); }

// the grid of a persistent kernel whose wavefronts take tiles from a counter: what the device holds at once, no idle workgroup
int persistent_tile_grid(const void *kernel, int threads, uint32_t waves, uint64_t n_tiles, int n_cu, size_t lds, uint64_t *blocks) {
    int occ = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds));
    *blocks = std::min<uint64_t>((n_tiles + waves - 1) / waves, (uint64_t)std::max(1, occ) * std::max(1, n_cu));
    return 0;
}

// the total of an exclusive scan launched on `stream`, behind it (scan.hip.h: [0] = the total of its scratch array)
int scan_total(hipStream_t stream, const uint32_t *scan_tmp, uint32_t *total) {
    HIP_TRY(hipMemcpyAsync(total, scan_tmp, sizeof(*total), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

// the self tests' staging: a host array into a fresh device buffer, and a device buffer back into a host array
template <typename T> int upload(DevBuf<T> &b, const T *host, size_t n) {
    if (int rc = dev_alloc(b, n)) return rc;
    HIP_TRY(hipMemcpy(b.p, host, sizeof(T) * n, hipMemcpyHostToDevice));
    return 0;
}
template <typename T> int download(T *host, const DevBuf<T> &b, size_t n) { HIP_TRY(hipMemcpy(host, b.p, sizeof(T) * n, hipMemcpyDeviceToHost)); return 0; }

}  // namespace

// The scalar description of a graph: pw_graph_replicate copies it in one assignment.
struct GraphDesc {
    int kind = 0;  // 0 = CSR, 1 = dense
    uint32_t n_nodes = 0, nnz = 0;
    bool unit = false;  // all weights are 1.0f (data not stored)
    uint32_t max_degree = 0;
    bool bits_only = false;          // dense graph created from packed bits: no compressed rows
    bool dense_nonneg = false;       // weighted dense graph: every stored value is finite and > 0 (walk_dense_w.hip.h)
    uint32_t words_per_row = 0;
    bool has_loop = false;                              // the CSR has a self loop (unit graphs: lists fixed up, wave kernel's lazy step off)
    bool lanes_off = false;                             // PECANPY_AMD_NO_LANES was set when the handle was created: the index is
                                                        // built (the wave kernel's lazy step reads it) but the lane kernel is not used
    bool vlines = false;                                // lines[nnz + v]: the line of vertex v's mirrored overflow read
    uint64_t clist_bytes = 0, line_bytes = 0;
    uint64_t n_clist = 0;
    uint32_t list_max_len = 0xffffffffu;                // partial index: lists longer than this were left out (EL_NO_LIST)
    uint64_t index_bytes = 0;                           // device bytes of the membership / lane index
};

// A graph on one device: its arrays, index and per-(p, q) tables, shared by the call contexts (pw_graph) that walk it.
// Written only by handle creation (pw_csr_create, pw_dense_create*, pw_graph_replicate), pw_graph_set_thresholds,
// pw_precomp_build and the lazy builders -- d_hasnbr in compute_offsets, ensure_tot_table, ensure_unit_tot,
// ensure_wlane_tables, spp_check -- each of which writes nothing when its keys already match.  A twin context reads it
// from another thread while the primary walks: its calls use the primary's (p, q, extend) and thresholds, so they find
// every table in place -- or build, under those keys, one that the primary's smaller half declined and does not read.
// Every table that reads the thresholds records the upload it was built from (*_thr_version against thr_version).
struct GraphData : GraphDesc {
    int device = 0;
    DevBuf<uint32_t> d_indptr, d_indices;
    DevBuf<uint32_t> d_hasnbr;                          // bit v: vertex v has neighbours (stream offsets; built by the first call)
    DevBuf<void> d_data;             // float32 (CSR graphs) or float64 (dense graphs); null when unit
    DevBuf<float> d_thr;
    DevBuf<uint64_t> d_adjbits;      // dense graphs: bit-packed adjacency rows
    DevBuf<uint32_t> d_deg;          // dense graphs: row degrees
    DevBuf<uint32_t> d_foff;         // CSR graphs: per-row membership filters (offsets, bits)
    DevBuf<uint64_t> d_fbits;
    DevBuf<uint2> d_kf;              // CSR graphs: (neighbour id, filter word) per CSR entry
    DevBuf<uint64_t> d_tab_off, d_slots;                // CSR graphs: adjacency index (exact lookups)
    DevBuf<uint4> d_vrec;                               // CSR graphs: per-vertex record (row start, degree, filter, index)
    DevBuf<pw::ELine> d_lines;                          // lane index (walk_lanes.hip.h): 64-byte edge line per CSR entry; its first 16 bytes
                                                        // {neighbour, common-neighbour count, reverse position, degree} also serve walk_kernel's lazy step
    DevBuf<uint8_t> d_clist;                            // lane index: the lists too long for their edge line
    double index_build_ms = 0;                          // device time of all index KERNELS of pw_csr_create (event pairs around them)
    double create_wall_ms = 0;                          // wall clock of pw_csr_create: runtime start-up, host passes, H2D, allocations, kernels
    uint64_t thr_version = 0;                           // thresholds uploaded (pw_graph_set_thresholds calls)
    DevBuf<float> d_tot_e, d_tot_v;                     // weighted CSR graphs: per-edge / per-vertex normalisers
    double tot_p = 0, tot_q = 0;                        // ... built for these parameters
    int tot_extend = -1;                                // -1: none yet
    uint64_t tot_thr_version = 0;                       // thresholds uploaded since the table was built?
    bool tot_failed = false;
    double tot_build_ms = 0;
    DevBuf<float> d_utot;                               // unit graphs, 1/p or 1/q not a power of two: row total per arriving line
    float utot_wo = 0, utot_wp = 0;                     // ... built for these biases (0: none)
    bool utot_failed = false;
    // weighted lane form (walk_lanes.hip.h: WEIGHTED): base values, their per-row float64 prefix sums, per-entry delta prefix sums
    DevBuf<float> d_wb;
    DevBuf<pw::PrefixPair> d_wpq;
    DevBuf<double> d_wdl, d_wl_dprev;
    DevBuf<unsigned long long> d_wl_off;
    DevBuf<uint32_t> d_wedge_row;                       // ... source vertex of every CSR entry
    DevBuf<pw::PrefixPair> d_wp1;                       // ... per-row prefix sums of the raw weights (first steps; graph-static)
    DevBuf<unsigned long long> d_wck_off;               // ... recorded chain values (wckpt_kernel): first record of entry e
    DevBuf<float> d_wck;
    double wl_p = 0, wl_q = 0;
    int wl_extend = -1;
    uint64_t wl_thr_version = 0;
    bool wl_failed = false;
    int spp_zero = -1;                                  // CSR: some stored weight is 0.0f (-1: not checked yet)
    // alias tables (PreComp modes)
    DevBuf<uint64_t> alias_indptr;
    DevBuf<uint32_t> alias_j, alias_s, alias_l, edge_row;
    DevBuf<float> alias_q;
    uint64_t n_alias = 0;
    int alias_kind = -1;  // -1 none, 0 second order, 1 first order
    double alias_p = 0, alias_q_param = 0;
    int alias_extend = 0;
    uint64_t alias_thr_version = 0;                     // ... from this threshold upload (read by the extend tables only)

    explicit GraphData(int dev) : device(dev) {}
    GraphData(const GraphData &) = delete;
    GraphData &operator=(const GraphData &) = delete;
    ~GraphData() { (void)hipSetDevice(device); }   // (the members free themselves behind this body: on their own device)
};

// blocks of 312 draws from `first_block` on that cover the draws up to stream_skip + total (at least one): the one rounding
// of expand_stream's range and of the range a hold keeps
static uint64_t stream_blocks_from(uint64_t first_block, uint64_t stream_skip, uint64_t total) {
    const uint64_t end_block = (stream_skip + total + 311) / 312;
    return end_block > first_block ? end_block - first_block : 1;
}

// A call context over a graph: streams, events, counters, random stream and scratch buffers, and the state of the
// current call.  The graph itself (gd) may be shared with a twin context.
struct pw_graph {
    int device = 0;
    std::shared_ptr<GraphData> gd;
    // TWIN (round 6): a second call context on the SAME device over the same GraphData (own streams, counters, queues, stream
    // buffers): the weighted lane form walks the two halves of a job array on the two contexts side by side, so that one half's
    // eager kernel runs beside the other half's lane round (simulate_twin)
    pw_graph *twin = nullptr;
    // INPUTS of a call, set around it by simulate_twin: not part of `call`, the driver's reset leaves them alone
    bool twin_active = false;                           // the current call runs on both contexts: each takes a share of the GPU
    std::function<void()> on_tables_ready;              // simulate_twin: called once the call's per-(p, q) tables are in place
    // What one call of the driver (simulate_device_impl) keeps for its launchers and its statistics: reset by ONE assignment
    // there, behind the validation, and read and written through this name only.
    struct Call {
        bool n2vpp = false;                             // the current call walks node2vec++ (walk_dense_w.hip.h)
        bool spp = false;                               // ... node2vec++ on this CSR handle (walk_sparse_pp.hip.h)
        bool wl_active = false;                         // the current call may run the weighted lane form (tables are there)
        bool wl_used = false;                           // ... and did
        double param_ms = 0;                            // (p, q)-dependent index time of the current call
        double lane_ms = 0;                             // lane kernel time of the current call
        uint32_t lane_rounds = 0;                       // lane kernel launches of the current call
        uint64_t runnable = 0;                          // whole-array call: jobs whose start has neighbours (the stream's nominal draws / walk_length)
        uint64_t ver_checked = 0, ver_mismatch = 0, ver_dropped = 0, ver_ties = 0;   // verification counts of the current call
    } call;
    // pw_simulate() walks a large job array in parts: the stream of the WHOLE array is expanded once, and while this is
    // set expand_stream() serves the parts' sub-ranges from g->rng as it stands (never kept across API calls)
    struct { bool valid = false, user = false; uint32_t seed = 0; uint64_t first_block = 0, n_blocks = 0; } rng_hold;   // (user: pw_stream_hold)
    void drop_hold() { rng_hold.valid = false; rng_hold.user = false; }
    // g->rng holds the draws [stream_skip, stream_skip + n_draws) of `seed`, expanded from draw `base` (expand_stream's *rng_base) on
    void set_hold(uint32_t seed, uint64_t base, uint64_t stream_skip, uint64_t n_draws, bool user) {
        rng_hold.valid = true;
        rng_hold.user = user;
        rng_hold.seed = seed;
        rng_hold.first_block = base / 312;
        rng_hold.n_blocks = stream_blocks_from(base / 312, stream_skip, n_draws);
    }
    static constexpr int N_STAGE = 12;
    PinnedBuf<void> stage[N_STAGE];        // pinned staging buffers of pw_simulate's copy out
    PinnedBuf<uint32_t> seed_state;        // pinned: the seed's MT19937 state on its way to the device
    int n_cu = 0;
    // scratch reused across calls
    DevBuf<uint64_t> stream_off, tile_sums;
    DevBuf<double> rng;
    DevBuf<uint32_t> mt_state, changed, redo;
    DevBuf<pw::SuspRec> susp[2];      // lane kernel: walks parked for the float chain (two queues, swapped per round)
    // generator states of recent calls, keyed by (seed, first block, blocks per generator, generators): a repeated
    // call (every pass of a benchmark, every chunk of a sharded run) skips the ~20 sequential jump-ahead launches
    struct MtCache { bool valid = false; uint32_t seed = 0, n_gen = 0; uint64_t first_block = 0; int per_gen_log = 0; uint64_t stamp = 0;
                     DevBuf<uint32_t> states; } mt_cache[8];
    uint64_t mt_stamp = 0;
    // verification mode of the lane kernel (PECANPY_AMD_VERIFY_TIGHT=1): steps the interval decision settled
    DevBuf<pw::VerRec> ver, ver_bad;
    DevBuf<uint32_t> ver_jobs;        // sampled verification (production): walks of mismatching records, redone by walk_kernel
    DevBuf<uint64_t> jump_table;  // MtJump::pow2_table() on the device
    DevBuf<uint32_t> jump_tmp;    // partial results of jumps whose taps are split over several workgroups (kept zeroed)
    bool jump_table_ready = false;
    DevBuf<unsigned long long> counters;  // N_COUNTERS device counters: counters.h names the slots
    DevBuf<float> probs_scratch;
    DevBuf<uint32_t> stream_words;   // pw_stream_words_device: raw stream words (624 per block)
    // Streams and events LAST: members go in reverse order behind the destructor's body, so the events are destroyed first, then
    // the streams, then the buffers above -- on this context's device (graph_common_init creates them; one that fails half way
    // leaves what it made to this destructor)
    pw::Stream stream;
    pw::Stream stream2;              // side stream: the zero-fill of the walk matrix runs under the stream expansion
    pw::Stream copy_stream;          // pw_simulate: the D2H of one part of the walk matrix runs here, under the walks of the next
    pw::Event ev_copy[N_STAGE];
    pw::Event ev_side;
    std::vector<pw::Event> round_ev;       // lane rounds: a pair of events per round, read once behind the last round (no sync per round)
    pw::Event ev[8];

    ~pw_graph() { (void)hipSetDevice(device); }   // (the members release themselves behind this body: on their own device)
};

// A CSR in device memory (pw_coo_to_csr_device, the edge-list reader, pw_holdout_edges): handles are made from it.
struct pw_csr_dev {
    int device = 0;
    uint64_t n_nodes = 0, nnz = 0, insertions = 0, dropped = 0;
    double build_ms = 0;
    DevBuf<uint32_t> d_indptr, d_indices;
    DevBuf<float> d_data;      // empty: no weights were given (every weight 1.0)
    DevBuf<double> d_data64;   // the edge-list reader with PW_EDGELIST_KEEP_F64: every entry's weight as parsed; empty otherwise
};

namespace {

// The owner of a call context under construction: every way out of a creator but the release() into *out destroys it (a twin
// with it).  A creator's locals go in reverse order of declaration, so where the owner stands among them decides what the
// handle outlives: each creator says so where it declares it.
template <typename T, void (*Destroy)(T *)> struct Closes { void operator()(T *p) const { Destroy(p); } };   // (KnnOwner, HoldoutOwner too)
using GraphOwner = std::unique_ptr<pw_graph, Closes<pw_graph, pw_graph_destroy>>;
using CsrDevOwner = std::unique_ptr<pw_csr_dev, Closes<pw_csr_dev, pw_csr_dev_destroy>>;

int set_device(const pw_graph *g) {
    HIP_TRY(hipSetDevice(g->device));
    return 0;
}

uint32_t os_seed() {
    std::random_device rd;
    return (uint32_t)rd();
}

// host emulation of seq_scan (walk_sparse.hip.h) used by the self test: identical arithmetic,
// `chunk` elements per pass instead of one wavefront pass.
template <typename T>
uint32_t seqscan_emulate(const T *x, uint32_t n, double r, bool use_target, uint32_t chunk, T *sum) {
    using B = pw::Binade<T>;
    using U = typename B::UInt;
    T c = (T)0;
    uint32_t k = 0;
    std::vector<pw::Inc<T>> f(chunk);
    while (k < n) {
        const int eb = B::eb_of(c);
        const U C = B::sig_of(c);
        const U Tt = use_target ? B::threshold(r, eb) : B::TOP;
        uint32_t m = n - k < chunk ? n - k : chunk;
        pw::Inc<T> run = {0, 0};
        uint32_t first = m;
        U Cprev = C, Cn = C;
        for (uint32_t l = 0; l < m; l++) {
            f[l] = B::quantize(x[k + l], eb);
            pw::Inc<T> incl = l ? B::compose(run, f[l]) : f[l];
            U Ci = B::apply(C, incl);
            if (Ci >= Tt) { first = l; Cn = Ci; break; }
            Cprev = Ci;
            run = incl;
        }
        if (first == m) {
            c = B::make(Cprev, eb);
            k += m;
            continue;
        }
        uint32_t kf = k + first;
        if (Cn < B::TOP) { c = B::make(Cn, eb); *sum = c; return kf; }
        c = B::make(Cprev, eb) + x[kf];
        if (use_target && (double)c >= r) { *sum = c; return kf; }
        k = kf + 1;
    }
    *sum = c;
    return n;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
PW_EXPORT const char *pw_version(void) { return "pecanpy_amd 0.1.0 (gfx950)"; }
PW_EXPORT const char *pw_last_error(void) { return g_err.c_str(); }

PW_EXPORT int pw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

PW_EXPORT int pw_warmup(int device, double *ms) {
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    HIP_TRY(hipStreamDestroy(s));
    if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PW_OK;
}

PW_EXPORT void pw_graph_destroy(pw_graph *g) {
    if (!g) return;
    if (g->twin) { pw_graph_destroy(g->twin); g->twin = nullptr; }
    delete g;        // (its events, streams and buffers with it, and the graph with the last context that walks it)
}

// a call context on `device` over `gd` (a twin's: the primary's graph) or over a new, empty graph
static int graph_common_init(pw_graph *g, int device, std::shared_ptr<GraphData> gd = nullptr) {
    const bool dbg = getenv("PECANPY_AMD_CREATE_DEBUG") != nullptr;
    auto nowms = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = nowms();
    auto lap = [&](const char *what) { if (dbg) { const double t = nowms(); fprintf(stderr, "[create]   init: %-28s %8.2f ms\n", what, t - t0); t0 = t; } };
    if (int rc = check_device(device)) return rc;
    g->device = device;
    g->gd = gd ? std::move(gd) : std::make_shared<GraphData>(device);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    g->n_cu = prop.multiProcessorCount;
    lap("device count / properties");
    HIP_TRY(g->stream.create(hipStreamNonBlocking));
    lap("stream");
    HIP_TRY(g->stream2.create(hipStreamNonBlocking));
    lap("stream2");
    HIP_TRY(g->ev_side.create(hipEventDisableTiming));
    for (auto &e : g->ev) HIP_TRY(e.create(hipEventDefault));
    lap("events");
    HIP_TRY(g->copy_stream.create(hipStreamNonBlocking));
    for (auto &e : g->ev_copy) HIP_TRY(e.create(hipEventDisableTiming));
    lap("copy stream + events");
    return 0;
}

// Defined in pecanpy_amd.hip beside expand_stream, declared here for drv_linkpred and drv_holdout: *words = word w0 of [w0, w0 + n)
static int stream_words_window(pw_graph *g, uint32_t seed, uint64_t w0, uint64_t n, const uint32_t **words);

static pw::CsrDev csr_dev(const pw_graph *g) {
    pw::CsrDev c;
    c.indptr = g->gd->d_indptr.p;
    c.indices = g->gd->d_indices.p;
    c.data = g->gd->d_data.p;
    c.thr = g->gd->d_thr.p;
    c.adjbits = g->gd->d_adjbits.p;
    c.foff = g->gd->d_foff.p;
    c.fbits = g->gd->d_fbits.p;
    c.kf = g->gd->d_kf.p;
    c.tab_off = g->gd->d_tab_off.p;
    c.slots = g->gd->d_slots.p;
    c.tri = (const uint4 *)g->gd->d_lines.p;   // (stride: one 64-byte line per CSR entry)
    c.clist = g->gd->d_clist.p;
    c.step_edge = 0xffffffffu;
    c.vrec = g->gd->d_vrec.p;
    c.words_per_row = g->gd->words_per_row;
    c.n_nodes = g->gd->n_nodes;
    c.nnz = g->gd->nnz;
    return c;
}
