#pragma once
// Host driver, skip-gram with negative sampling (sgns.hip.h, sgns_locks.hpp): the session (pw_sgns), its vocabulary, epochs,
// evaluation, state, vectors and row locks, and the one-call trainers over it.  Exports pw_sgns_*.
#include "drv_core.hip.h"
#include "sgns.hip.h"
#include "sgns_locks.hpp"

// ---- skip-gram with negative sampling over a walk matrix (sgns.hip.h) -------------------------
template <int PER, bool LOSS, bool LOCK>
static void sgns_launch(unsigned blocks, unsigned threads, size_t lds, const pw::SgnsArgs &a) {
    if constexpr (LOCK)
        hipLaunchKernelGGL((pw::sgns_walk_kernel<PER, LOSS, true, uint32_t, uint32_t>), dim3(blocks), dim3(threads), lds, 0, a, a.walks,
                           a.table, a.keep, a.lock0, a.lock1);
    else
        hipLaunchKernelGGL((pw::sgns_walk_kernel<PER, LOSS>), dim3(blocks), dim3(threads), lds, 0, a, a.walks, a.table, a.keep);
}
template <bool LOSS, bool LOCK>
static void sgns_launch_per(int per, unsigned blocks, unsigned threads, size_t lds, const pw::SgnsArgs &a) {
    switch (per) {   // one instance per count of components per lane: only the last component needs a lane guard
    case 1: sgns_launch<1, LOSS, LOCK>(blocks, threads, lds, a); break;
    case 2: sgns_launch<2, LOSS, LOCK>(blocks, threads, lds, a); break;
    case 3: sgns_launch<3, LOSS, LOCK>(blocks, threads, lds, a); break;
    case 4: sgns_launch<4, LOSS, LOCK>(blocks, threads, lds, a); break;
    case 5: sgns_launch<5, LOSS, LOCK>(blocks, threads, lds, a); break;
    case 6: sgns_launch<6, LOSS, LOCK>(blocks, threads, lds, a); break;
    case 7: sgns_launch<7, LOSS, LOCK>(blocks, threads, lds, a); break;
    default: sgns_launch<8, LOSS, LOCK>(blocks, threads, lds, a); break;
    }
}
// (the LOCK instances only when a row of either matrix is frozen: without locks a run is the LOCK = false kernel)
template <bool LOSS>
static void sgns_launch_lock(bool lock, int per, unsigned blocks, unsigned threads, size_t lds, const pw::SgnsArgs &a) {
    if (lock) sgns_launch_per<LOSS, true>(per, blocks, threads, lds, a);
    else sgns_launch_per<LOSS, false>(per, blocks, threads, lds, a);
}

// A trainer between launches: the two matrices, the tables of the vocabulary stage, the launch geometry, and where the run
// stands (pw_sgns_state).  The walk matrix is the caller's.
struct pw_sgns {
    int device = 0;
    pw::SgnsArgs a;                          // everything of a launch but item_base / lr_base / lr_total / alpha / min_alpha / counters
    uint64_t n_items = 0;                    // n_walks * (walk_length + 1): the items of one epoch
    uint32_t n_nodes = 0;
    bool loss = false;
    unsigned blocks = 1, threads = 64;
    size_t lds = 0;
    pw_sgns_state st;
    double vocab_ms = 0, init_ms = 0;
    DevBuf<float> syn0, syn1, keep;
    DevBuf<uint32_t> table;
    DevBuf<pw_sgns_epoch> epoch_out;         // what the launches of one pw_sgns_run leave, one cell per epoch
    DevBuf<double> walk_loss, block_loss;    // PW_SGNS_LOSS: per walk, per SGNS_LOSS_CHUNK walks
    DevBuf<unsigned long long> walk_evals, block_evals;
    pw::Event ev0, ev1;                      // the pair around the training launches of a run
    float sample = 0;                        // of the create call: what PW_SGNS_RECOUNT rebuilds the keep probabilities with
    unsigned n_cus = 1;
    // pw_sgns_evaluate: its own per-walk and per-block cells (sized by the matrix it scores) and its record
    DevBuf<double> eval_walk_loss, eval_block_loss;
    DevBuf<unsigned long long> eval_walk_evals, eval_block_evals;
    DevBuf<pw_sgns_epoch> eval_out;
    // pw_sgns_set_locks: the frozen rows of syn0 / syn1 as bits (a.lock0 / a.lock1 point here); not allocated = no row frozen
    DevBuf<uint32_t> lock0, lock1;
    uint64_t n_locked[2] = {0, 0};
    bool ran_locked = false;                 // the last pw_sgns_run launched the LOCK instances
};
static_assert(offsetof(pw_sgns_epoch, kept_occurrences) + sizeof(uint64_t) == offsetof(pw_sgns_epoch, trained_pairs),
              "the kernel's two counters are consecutive cells of an epoch's record");

// The vocabulary stage of a walk matrix.  The device check first: a node id >= n_nodes or a length cell > walk_length + 1 is
// PW_ERR_INVALID with the text every entry that takes a matrix shares.  With `out`, word2vec's unigram^0.75 table and the
// subsampling probabilities from the word counts of that pass, uploaded; without it the check alone.
struct SgnsVocab {
    DevBuf<uint32_t> table;
    DevBuf<float> keep;                      // (not allocated with sample = 0)
    uint32_t table_size = 0;
};
static int sgns_vocabulary(const uint32_t *d_walks, uint64_t n_walks, uint32_t L, uint32_t n_nodes, float sample, SgnsVocab *out) {
    DevBuf<unsigned long long> cnt_buf;
    // d_cnt: [0, n_nodes) word counts, [n_nodes] first bad walk
    hipError_t e = cnt_buf.alloc((size_t)n_nodes + 1);
    unsigned long long *const d_cnt = cnt_buf.p;
    if (e == hipSuccess) e = hipMemset(d_cnt, 0, sizeof(unsigned long long) * (size_t)n_nodes);
    if (e == hipSuccess) e = hipMemset(d_cnt + n_nodes, 0xff, sizeof(unsigned long long));
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    // vocabulary statistics (and the check that the matrix only names nodes of the vocabulary)
    const uint64_t n_items = n_walks * (uint64_t)(L + 1);
    hipLaunchKernelGGL(pw::sgns_count_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, 0, d_walks, n_walks, L, n_nodes, d_cnt,
                       d_cnt + n_nodes);
    std::vector<unsigned long long> cnt((size_t)n_nodes + 1);
    const size_t first = out ? 0 : n_nodes;   // (the check alone: only its cell comes down)
    e = hipMemcpy(cnt.data() + first, d_cnt + first, sizeof(unsigned long long) * ((size_t)n_nodes + 1 - first), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    if (cnt[n_nodes] != ~0ull)
        return fail(PW_ERR_INVALID, "walk " + std::to_string(cnt[n_nodes]) + ": node id >= n_nodes or length cell > walk_length + 1");
    if (!out) return PW_OK;
    double total = 0, pow_total = 0;
    for (uint32_t i = 0; i < n_nodes; i++) { total += (double)cnt[i]; pow_total += std::pow((double)cnt[i], 0.75); }
    if (!(total > 0)) return fail(PW_ERR_INVALID, "the walk matrix holds no nodes");
    // word2vec's unigram^0.75 table (a word that never occurs owns no slot) and subsampling probabilities
    const uint32_t table_size = (uint32_t)std::min<uint64_t>(1ull << 26, std::max<uint64_t>(1ull << 16, 16ull * n_nodes));
    std::vector<uint32_t> table(table_size);
    {
        uint32_t t = 0, last = 0;
        double cum = 0;
        for (uint32_t w = 0; w < n_nodes; w++) {
            if (!cnt[w]) continue;
            last = w;
            cum += std::pow((double)cnt[w], 0.75) / pow_total;
            while (t < table_size && (double)(t + 1) / table_size <= cum) table[t++] = w;
        }
        while (t < table_size) table[t++] = last;   // (rounding of the last share)
    }
    std::vector<float> keep;
    if (sample > 0) {
        keep.resize(n_nodes);
        const double thr = (double)sample * total;
        for (uint32_t i = 0; i < n_nodes; i++)
            keep[i] = cnt[i] ? (float)std::min(1.0, (std::sqrt((double)cnt[i] / thr) + 1.0) * thr / (double)cnt[i]) : 1.0f;
    }
    e = out->table.alloc(table_size);
    if (e == hipSuccess) e = hipMemcpy(out->table.p, table.data(), sizeof(uint32_t) * (size_t)table_size, hipMemcpyHostToDevice);
    if (e == hipSuccess && sample > 0) {
        e = out->keep.alloc(n_nodes);
        if (e == hipSuccess) e = hipMemcpy(out->keep.p, keep.data(), sizeof(float) * (size_t)n_nodes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    out->table_size = table_size;
    return PW_OK;
}

PW_EXPORT int pw_sgns_create_device(int device, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint32_t n_nodes,
                                    uint32_t dim, uint32_t window, uint32_t negative, uint32_t epochs, float alpha, float min_alpha,
                                    float sample, uint32_t seed, uint32_t workers, uint32_t flags, pw_sgns **out) {
    if (!out) return fail(PW_ERR_INVALID, "null pointer / empty corpus");
    *out = nullptr;
    if (!d_walks || !n_walks || !n_nodes) return fail(PW_ERR_INVALID, "null pointer / empty corpus");
    if (dim == 0 || dim > 64 * pw::SGNS_MAX_PER_LANE) return fail(PW_ERR_INVALID, "dim must be in 1..512");
    if (window == 0 || epochs == 0) return fail(PW_ERR_INVALID, "window and epochs must be positive");
    if (flags & ~(uint32_t)PW_SGNS_LOSS) return fail(PW_ERR_INVALID, "unknown flag");
    const uint32_t L = walk_length;
    // the survivors of a walk live in the wavefront's LDS: four wavefronts to a workgroup while that fits, else one
    const size_t lds_limit = 64 << 10, lds_wave = pw::sgns_lds_bytes_per_wave(L);
    if (lds_wave > lds_limit) return fail(PW_ERR_INVALID, "walk_length must be below 8192");
    const unsigned waves_per_block = 4 * lds_wave <= lds_limit ? 4 : 1;
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    const size_t vbytes = sizeof(float) * (size_t)n_nodes * dim;
    std::unique_ptr<pw_sgns> s(new pw_sgns);
    s->device = device; s->n_nodes = n_nodes; s->loss = (flags & PW_SGNS_LOSS) != 0; s->sample = sample;
    auto t_vocab = clk::now();
    hipError_t e = s->syn0.alloc((size_t)n_nodes * dim);
    if (e == hipSuccess) e = s->syn1.alloc((size_t)n_nodes * dim);
    if (e == hipSuccess) e = hipMemset(s->syn1.p, 0, vbytes);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    const uint64_t n_items = n_walks * (uint64_t)(L + 1);
    SgnsVocab vocab;
    if (int rc = sgns_vocabulary(d_walks, n_walks, L, n_nodes, sample, &vocab)) return rc;
    const uint32_t table_size = vocab.table_size;
    s->table = std::move(vocab.table);
    s->keep = std::move(vocab.keep);
    s->vocab_ms = ms_since(t_vocab);
    // syn0 ~ U(-0.5, 0.5) / dim (word2vec.c), seeded
    auto t_init = clk::now();
    {
        std::vector<float> init((size_t)n_nodes * dim);
        uint64_t x = 0x9E3779B97F4A7C15ull ^ ((uint64_t)seed << 17);
        for (auto &f : init) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            f = (((float)((x >> 40) & 0xffffff) / 16777216.0f) - 0.5f) / (float)dim;
        }
        e = hipMemcpy(s->syn0.p, init.data(), vbytes, hipMemcpyHostToDevice);
    }
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) e = s->ev0.create(hipEventDefault);
    if (e == hipSuccess) e = s->ev1.create(hipEventDefault);
    if (e == hipSuccess && s->loss) {
        const size_t n_blocks = (size_t)((n_walks + pw::SGNS_LOSS_CHUNK - 1) / pw::SGNS_LOSS_CHUNK);
        e = s->walk_loss.alloc(n_walks);
        if (e == hipSuccess) e = s->walk_evals.alloc(n_walks);
        if (e == hipSuccess) e = s->block_loss.alloc(n_blocks);
        if (e == hipSuccess) e = s->block_evals.alloc(n_blocks);
    }
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    s->init_ms = ms_since(t_init);
    pw::SgnsArgs &a = s->a;
    a.walks = d_walks; a.n_walks = n_walks; a.L = L; a.dim = dim; a.window = window; a.negative = negative;
    a.syn0 = s->syn0.p; a.syn1 = s->syn1.p; a.table = s->table.p; a.table_size = table_size; a.keep = s->keep.p;
    a.alpha = alpha; a.min_alpha = min_alpha; a.item_base = 0; a.lr_base = 0; a.lr_total = n_items * epochs; a.seed = seed;
    a.counters = nullptr; a.walk_loss = s->walk_loss.p; a.walk_evals = s->walk_evals.p;
    a.lock0 = a.lock1 = nullptr;
    s->n_items = n_items;
    s->st.epoch = 0; s->st.sched_pos = 0; s->st.sched_total = epochs; s->st.alpha = alpha; s->st.min_alpha = min_alpha;
    // concurrency.  workers == 1: ONE wavefront takes the walks in order (deterministic: the run gensim's workers=1
    // corresponds to; compared with oracle/sgns_ref.c).  workers == 0: as many wavefronts as keep hogwild collisions
    // rare -- far more wavefronts than vocabulary rows in flight would overwrite most updates of a small graph.  The rule
    // "at least ~256 items per wavefront, at most 8 workgroups per CU" is now counted in walks: a wavefront owns at least
    // ceil(256 / (L + 1)) walks (4 for the default 80-step walks), and the cap is 32 wavefronts per CU whatever the
    // workgroup size.  workers > 1: that many wavefronts (rounded up to whole workgroups).
    unsigned blocks, threads = 64 * waves_per_block;
    if (workers == 1) { blocks = 1; threads = 64; }
    else if (workers > 1) blocks = (workers + waves_per_block - 1) / waves_per_block;
    else {
        const uint64_t walks_per_wave = (256 + (uint64_t)L) / ((uint64_t)L + 1);
        const uint64_t want_waves = (n_walks + walks_per_wave - 1) / walks_per_wave;
        const uint64_t waves = std::max<uint64_t>(1, std::min<uint64_t>(want_waves, (uint64_t)prop.multiProcessorCount * 32));
        blocks = (unsigned)((waves + waves_per_block - 1) / waves_per_block);
    }
    s->blocks = blocks; s->threads = threads; s->n_cus = (unsigned)std::max(1, prop.multiProcessorCount);
    s->lds = lds_wave * (threads / 64);
    a.n_waves = blocks * (threads / 64);
    *out = s.release();
    return PW_OK;
}

PW_EXPORT int pw_sgns_run(pw_sgns *s, uint32_t n_epochs, pw_sgns_epoch *per_epoch, pw_sgns_stats *stats) {
    if (!s) return fail(PW_ERR_INVALID, "null pointer");
    if (n_epochs == 0) return fail(PW_ERR_INVALID, "n_epochs must be positive");
    if (s->st.sched_pos + n_epochs > s->st.sched_total)   // (before any launch)
        return fail(PW_ERR_INVALID, "the schedule has " + std::to_string(s->st.sched_total - s->st.sched_pos) + " of " +
                                        std::to_string(s->st.sched_total) + " epochs left, " + std::to_string(n_epochs) + " asked for");
    HIP_TRY(hipSetDevice(s->device));
    hipError_t e = s->epoch_out.ensure(n_epochs);
    if (e == hipSuccess) e = hipMemset(s->epoch_out.p, 0, sizeof(pw_sgns_epoch) * (size_t)n_epochs);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    pw::SgnsArgs a = s->a;
    a.alpha = s->st.alpha; a.min_alpha = s->st.min_alpha; a.lr_total = s->n_items * s->st.sched_total;
    const int per = (int)((a.dim + 63) / 64);
    const unsigned n_blocks = (unsigned)((a.n_walks + pw::SGNS_LOSS_CHUNK - 1) / pw::SGNS_LOSS_CHUNK);
    const bool lock = a.lock0 || a.lock1;
    s->ran_locked = lock;
    (void)hipEventRecord(s->ev0, 0);
    for (uint32_t i = 0; i < n_epochs; i++) {
        a.item_base = s->n_items * (s->st.epoch + i);
        a.lr_base = s->n_items * (s->st.sched_pos + i);
        pw_sgns_epoch *cell = s->epoch_out.p + i;
        a.counters = (unsigned long long *)&cell->kept_occurrences;
        if (!s->loss) sgns_launch_lock<false>(lock, per, s->blocks, s->threads, s->lds, a);
        else {
            sgns_launch_lock<true>(lock, per, s->blocks, s->threads, s->lds, a);
            hipLaunchKernelGGL(pw::sgns_loss_reduce_kernel, dim3(n_blocks), dim3(256), 0, 0, s->walk_loss.p, s->walk_evals.p, a.n_walks,
                               (uint64_t)pw::SGNS_LOSS_CHUNK, s->block_loss.p, s->block_evals.p);
            hipLaunchKernelGGL(pw::sgns_loss_reduce_kernel, dim3(1), dim3(256), 0, 0, s->block_loss.p, s->block_evals.p, (uint64_t)n_blocks,
                               (uint64_t)n_blocks, &cell->loss, (unsigned long long *)&cell->evaluations);
        }
    }
    (void)hipEventRecord(s->ev1, 0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // (the launches were queued: whatever the outcome, the vectors have moved on by what ran)
    s->st.epoch += n_epochs; s->st.sched_pos += n_epochs;
    float train_ms = 0;
    std::vector<pw_sgns_epoch> got(n_epochs);
    if (e == hipSuccess) e = hipEventElapsedTime(&train_ms, s->ev0, s->ev1);
    if (e == hipSuccess) e = hipMemcpy(got.data(), s->epoch_out.p, sizeof(pw_sgns_epoch) * (size_t)n_epochs, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    if (per_epoch) std::copy(got.begin(), got.end(), per_epoch);
    if (stats) {
        stats->vocab_ms = s->vocab_ms; stats->init_ms = s->init_ms; stats->train_ms = train_ms;
        stats->kept_occurrences = stats->trained_pairs = 0;
        for (const pw_sgns_epoch &g : got) { stats->kept_occurrences += g.kept_occurrences; stats->trained_pairs += g.trained_pairs; }
        stats->wavefronts = (uint64_t)s->blocks * (s->threads / 64);
    }
    return PW_OK;
}

template <int PER>
static void sgns_eval_launch(unsigned blocks, unsigned threads, size_t lds, const pw::SgnsArgs &a) {
    hipLaunchKernelGGL((pw::sgns_eval_kernel<PER>), dim3(blocks), dim3(threads), lds, 0, a, a.walks, a.table, a.keep, a.syn0, a.syn1);
}

// Scores a walk matrix with the vectors as they are (sgns.hip.h: sgns_eval_kernel); nothing of the session changes.
PW_EXPORT int pw_sgns_evaluate(pw_sgns *s, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint64_t epoch,
                               pw_sgns_epoch *out) {
    if (!s || !out) return fail(PW_ERR_INVALID, "null pointer");
    const bool own = d_walks == nullptr;
    if (own) { d_walks = s->a.walks; n_walks = s->a.n_walks; walk_length = s->a.L; }
    if (!n_walks) return fail(PW_ERR_INVALID, "null pointer / empty corpus");
    const uint32_t L = walk_length;
    const size_t lds_limit = 64 << 10, lds_wave = pw::sgns_lds_bytes_per_wave(L);
    if (lds_wave > lds_limit) return fail(PW_ERR_INVALID, "walk_length must be below 8192");
    const unsigned waves_per_block = 4 * lds_wave <= lds_limit ? 4 : 1;
    // (the kernel counts items in 64 bits: n_items * epoch must fit)
    const uint64_t n_items = n_walks * (uint64_t)(L + 1);
    if (epoch >= ~0ull / n_items) return fail(PW_ERR_INVALID, "epoch index out of range");
    HIP_TRY(hipSetDevice(s->device));
    if (!own)   // (the session's own matrix passed these checks when it was taken)
        if (int rc = sgns_vocabulary(d_walks, n_walks, L, s->n_nodes, s->sample, nullptr)) return rc;
    const unsigned n_blocks = (unsigned)((n_walks + pw::SGNS_LOSS_CHUNK - 1) / pw::SGNS_LOSS_CHUNK);
    hipError_t e = s->eval_walk_loss.ensure(n_walks);
    if (e == hipSuccess) e = s->eval_walk_evals.ensure(n_walks);
    if (e == hipSuccess) e = s->eval_block_loss.ensure(n_blocks);
    if (e == hipSuccess) e = s->eval_block_evals.ensure(n_blocks);
    if (e == hipSuccess) e = s->eval_out.ensure(1);
    if (e == hipSuccess) e = hipMemset(s->eval_out.p, 0, sizeof(pw_sgns_epoch));
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_evaluate: ") + hipGetErrorString(e));
    pw::SgnsArgs a = s->a;
    a.walks = d_walks; a.n_walks = n_walks; a.L = L;
    a.item_base = n_items * epoch;
    a.counters = (unsigned long long *)&s->eval_out.p->kept_occurrences;
    a.walk_loss = s->eval_walk_loss.p; a.walk_evals = s->eval_walk_evals.p;
    // nothing is written, so nothing races: a wavefront per walk up to what the device holds at once, whatever `workers` is
    const uint64_t waves = std::min<uint64_t>(n_walks, (uint64_t)s->n_cus * 32);
    const unsigned blocks = (unsigned)((waves + waves_per_block - 1) / waves_per_block), threads = 64 * waves_per_block;
    a.n_waves = blocks * waves_per_block;
    const size_t lds = lds_wave * waves_per_block;
    switch ((a.dim + 63) / 64) {   // (as sgns_launch_per)
    case 1: sgns_eval_launch<1>(blocks, threads, lds, a); break;
    case 2: sgns_eval_launch<2>(blocks, threads, lds, a); break;
    case 3: sgns_eval_launch<3>(blocks, threads, lds, a); break;
    case 4: sgns_eval_launch<4>(blocks, threads, lds, a); break;
    case 5: sgns_eval_launch<5>(blocks, threads, lds, a); break;
    case 6: sgns_eval_launch<6>(blocks, threads, lds, a); break;
    case 7: sgns_eval_launch<7>(blocks, threads, lds, a); break;
    default: sgns_eval_launch<8>(blocks, threads, lds, a); break;
    }
    hipLaunchKernelGGL(pw::sgns_loss_reduce_kernel, dim3(n_blocks), dim3(256), 0, 0, a.walk_loss, a.walk_evals, n_walks,
                       (uint64_t)pw::SGNS_LOSS_CHUNK, s->eval_block_loss.p, s->eval_block_evals.p);
    hipLaunchKernelGGL(pw::sgns_loss_reduce_kernel, dim3(1), dim3(256), 0, 0, s->eval_block_loss.p, s->eval_block_evals.p, (uint64_t)n_blocks,
                       (uint64_t)n_blocks, &s->eval_out.p->loss, (unsigned long long *)&s->eval_out.p->evaluations);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, s->eval_out.p, sizeof(pw_sgns_epoch), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_evaluate: ") + hipGetErrorString(e));
    return PW_OK;
}

// Another matrix of the same shape under the session: the schedule arithmetic (n_items) stays, the state and both matrices
// are not touched.  Everything that can fail comes before the first assignment.
PW_EXPORT int pw_sgns_set_walks(pw_sgns *s, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint32_t flags) {
    if (!s || !d_walks) return fail(PW_ERR_INVALID, "null pointer");
    if (flags & ~(uint32_t)PW_SGNS_RECOUNT) return fail(PW_ERR_INVALID, "unknown flag");
    if (n_walks != s->a.n_walks || walk_length != s->a.L)
        return fail(PW_ERR_INVALID, "the session was created on " + std::to_string(s->a.n_walks) + " walks of length " + std::to_string(s->a.L) +
                                        ": a matrix of " + std::to_string(n_walks) + " walks of length " + std::to_string(walk_length) +
                                        " needs a session of its own");
    HIP_TRY(hipSetDevice(s->device));
    SgnsVocab vocab;
    const bool recount = (flags & PW_SGNS_RECOUNT) != 0;
    if (int rc = sgns_vocabulary(d_walks, n_walks, walk_length, s->n_nodes, s->sample, recount ? &vocab : nullptr)) return rc;
    s->a.walks = d_walks;
    if (recount) {
        s->table = std::move(vocab.table);
        s->keep = std::move(vocab.keep);
        s->a.table = s->table.p; s->a.table_size = vocab.table_size; s->a.keep = s->keep.p;
    }
    return PW_OK;
}

PW_EXPORT int pw_sgns_get_state(const pw_sgns *s, pw_sgns_state *st) {
    if (!s || !st) return fail(PW_ERR_INVALID, "null pointer");
    *st = s->st;
    return PW_OK;
}

PW_EXPORT int pw_sgns_set_state(pw_sgns *s, const pw_sgns_state *st) {
    if (!s || !st) return fail(PW_ERR_INVALID, "null pointer");
    if (st->sched_total == 0 || st->sched_pos > st->sched_total) return fail(PW_ERR_INVALID, "schedule position beyond its length");
    // (the kernel counts items in 64 bits: n_items * epoch must fit)
    const uint64_t most = ~0ull / s->n_items;
    if (st->epoch >= most || st->sched_total >= most) return fail(PW_ERR_INVALID, "epoch index out of range");
    if (!std::isfinite(st->alpha) || !std::isfinite(st->min_alpha)) return fail(PW_ERR_INVALID, "alpha and min_alpha must be finite");
    s->st = *st;
    return PW_OK;
}

static int sgns_vectors_copy(pw_sgns *s, int which, float *d_ptr, bool out) {
    if (!s || !d_ptr) return fail(PW_ERR_INVALID, "null pointer");
    if (which != 0 && which != 1) return fail(PW_ERR_INVALID, "which must be 0 (syn0) or 1 (syn1)");
    HIP_TRY(hipSetDevice(s->device));
    float *mine = which ? s->syn1.p : s->syn0.p;
    const hipError_t e = hipMemcpy(out ? d_ptr : mine, out ? mine : d_ptr, sizeof(float) * (size_t)s->n_nodes * s->a.dim, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_vectors: ") + hipGetErrorString(e));
    return PW_OK;
}
PW_EXPORT int pw_sgns_vectors_get(pw_sgns *s, int which, float *d_ptr) { return sgns_vectors_copy(s, which, d_ptr, true); }
PW_EXPORT int pw_sgns_vectors_set(pw_sgns *s, int which, const float *d_ptr) { return sgns_vectors_copy(s, which, (float *)d_ptr, false); }

// The byte mask of one matrix packed into bits; `words` is left unallocated when no byte is set.
static int sgns_pack_locks(uint32_t n_nodes, const uint8_t *d_mask, DevBuf<unsigned long long> &n_set, DevBuf<uint32_t> *words,
                           uint64_t *count) {
    *count = 0;
    if (!d_mask) return PW_OK;
    hipError_t e = words->alloc(pw::sgns_lock_words(n_nodes));
    if (e == hipSuccess) e = hipMemset(n_set.p, 0, sizeof(unsigned long long));
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_set_locks: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(pw::sgns_lock_pack_kernel, dim3(pw::sgns_lock_blocks(n_nodes)), dim3(pw::SGNS_LOCK_THREADS), 0, 0, d_mask, n_nodes,
                       words->p, n_set.p);
    unsigned long long n = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(&n, n_set.p, sizeof(n), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_set_locks: ") + hipGetErrorString(e));
    if (!n) words->release();   // (a mask without a non-zero byte is "none")
    *count = n;
    return PW_OK;
}

// Everything that can fail comes before the first assignment: on an error the session keeps the locks it had.
PW_EXPORT int pw_sgns_set_locks(pw_sgns *s, const uint8_t *d_lock0, const uint8_t *d_lock1) {
    if (!s) return fail(PW_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(s->device));
    DevBuf<unsigned long long> n_set;
    if (hipError_t e = n_set.alloc(1)) return fail(PW_ERR_HIP, std::string("pw_sgns_set_locks: ") + hipGetErrorString(e));
    DevBuf<uint32_t> w0, w1;
    uint64_t n0 = 0, n1 = 0;
    if (int rc = sgns_pack_locks(s->n_nodes, d_lock0, n_set, &w0, &n0)) return rc;
    if (int rc = sgns_pack_locks(s->n_nodes, d_lock1, n_set, &w1, &n1)) return rc;
    s->lock0 = std::move(w0); s->lock1 = std::move(w1);
    s->a.lock0 = s->lock0.p; s->a.lock1 = s->lock1.p;
    s->n_locked[0] = n0; s->n_locked[1] = n1;
    return PW_OK;
}

PW_EXPORT int pw_sgns_get_locks(const pw_sgns *s, uint8_t *d_lock0, uint8_t *d_lock1) {
    if (!s) return fail(PW_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t *words[2] = {s->lock0.p, s->lock1.p};
    uint8_t *outs[2] = {d_lock0, d_lock1};
    hipError_t e = hipSuccess;
    for (int m = 0; m < 2 && e == hipSuccess; m++) {
        if (!outs[m]) continue;
        if (!words[m]) e = hipMemset(outs[m], 0, s->n_nodes);
        else
            hipLaunchKernelGGL(pw::sgns_lock_unpack_kernel, dim3(pw::sgns_lock_blocks(s->n_nodes)), dim3(pw::SGNS_LOCK_THREADS), 0, 0, words[m],
                               s->n_nodes, outs[m]);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_get_locks: ") + hipGetErrorString(e));
    return PW_OK;
}

PW_EXPORT int pw_sgns_lock_info(const pw_sgns *s, uint64_t out[3]) {
    if (!s || !out) return fail(PW_ERR_INVALID, "null pointer");
    out[0] = s->n_locked[0]; out[1] = s->n_locked[1]; out[2] = s->ran_locked ? 1 : 0;
    return PW_OK;
}

PW_EXPORT void pw_sgns_destroy(pw_sgns *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

// the one-shot entry: a session that runs its whole schedule and leaves syn0 in the caller's buffer
PW_EXPORT int pw_sgns_train_device(int device, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length, uint32_t n_nodes,
                                   uint32_t dim, uint32_t window, uint32_t negative, uint32_t epochs, float alpha, float min_alpha,
                                   float sample, uint32_t seed, uint32_t workers, float *d_vectors, pw_sgns_stats *stats) {
    if (!d_walks || !d_vectors || !n_walks || !n_nodes) return fail(PW_ERR_INVALID, "null pointer / empty corpus");
    pw_sgns *raw = nullptr;
    int rc = pw_sgns_create_device(device, d_walks, n_walks, walk_length, n_nodes, dim, window, negative, epochs, alpha, min_alpha, sample,
                                   seed, workers, 0, &raw);
    if (rc != PW_OK) return rc;
    std::unique_ptr<pw_sgns, void (*)(pw_sgns *)> s(raw, pw_sgns_destroy);
    rc = pw_sgns_run(s.get(), epochs, nullptr, stats);
    if (rc != PW_OK) return rc;
    return pw_sgns_vectors_get(s.get(), 0, d_vectors);
}

// host-matrix entry: upload, the device entry, download
PW_EXPORT int pw_sgns_train(int device, const uint32_t *walks, uint64_t n_walks, uint32_t walk_length, uint32_t n_nodes,
                            uint32_t dim, uint32_t window, uint32_t negative, uint32_t epochs, float alpha, float min_alpha,
                            float sample, uint32_t seed, uint32_t workers, float *vectors) {
    if (!walks || !vectors || !n_walks || !n_nodes) return fail(PW_ERR_INVALID, "null pointer / empty corpus");
    if (dim == 0 || dim > 64 * pw::SGNS_MAX_PER_LANE) return fail(PW_ERR_INVALID, "dim must be in 1..512");
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t wbytes = sizeof(uint32_t) * (size_t)n_walks * ((size_t)walk_length + 2), vbytes = sizeof(float) * (size_t)n_nodes * dim;
    DevBuf<uint32_t> d_walks;
    DevBuf<float> d_vectors;
    hipError_t e = d_walks.alloc((size_t)n_walks * ((size_t)walk_length + 2));
    if (e == hipSuccess) e = d_vectors.alloc((size_t)n_nodes * dim);
    if (e == hipSuccess) e = hipMemcpy(d_walks.p, walks, wbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    int rc = pw_sgns_train_device(device, d_walks.p, n_walks, walk_length, n_nodes, dim, window, negative, epochs, alpha, min_alpha,
                                  sample, seed, workers, d_vectors.p, nullptr);
    if (rc == PW_OK) {
        e = hipMemcpy(vectors, d_vectors.p, vbytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(PW_ERR_HIP, std::string("pw_sgns_train: ") + hipGetErrorString(e));
    }
    return rc;
}
