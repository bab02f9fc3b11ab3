// seq_spec_host.hpp -- the speculation rounds of seq_spec.h on the host: its plan, round loop and per-item code, each pass
// over the candidates or the windows a plain loop, words from mt_words_host.  Behind
// pw_selftest_seq_offsets (FirstOrderUnweighted, offsets only), pw_selftest_seq_walks (all three modes on caller-built
// alias tables: rows and counters too) and tools/seq_spec_selfcheck.cpp.
#pragma once
#include <vector>

#include "mtjump.hpp"
#include "seq_spec.h"

namespace pw {

struct SeqHostBackend {
    SeqGraph g;
    const uint32_t *starts;
    uint32_t seed;
    uint64_t *offsets;            // [n_jobs + 1] absolute word offset of every job's start
    uint32_t *out = nullptr;      // the walk matrix, when the caller wants the rows too
    SeqCounts counts = {0, 0, 0, 0};   // of the committed jobs (candidates never count)
    uint64_t buf_first = 0;
    unsigned long long sumsq = 0;
    std::vector<uint32_t> words, consumed, jump, chain;

    int fill(uint64_t first_block, uint64_t n_blocks) {
        words.resize(n_blocks * SEQ_BLOCK);
        mt_words_host(seed, first_block * SEQ_BLOCK, words.size(), words.data());
        buf_first = first_block;
        return 0;
    }
    int round(uint64_t i0, uint64_t base, uint64_t n_words, const SeqWindow *win, uint32_t G, uint32_t total, SeqRoundRec *rec) {
        const uint32_t levels = seq_levels(G);
        consumed.assign(total, 0);
        jump.assign((size_t)(levels ? levels : 1) * total, SEQ_NONE);
        chain.assign(G, 0);
        SeqRoundArgs a{g, starts, words.data(), n_words, base, i0, win, G, total, consumed.data(), jump.data(), total, chain.data(), rec, out};
        for (uint32_t c = 0; c < total; c++) seq_candidate_item(a, c);
        if (levels)
            for (uint32_t c = 0; c < total; c++) seq_succ_item(a, c);
        for (uint32_t k = 1; k < levels; k++)
            for (uint32_t c = 0; c < total; c++) seq_double_item(a, k, c);
        for (uint32_t gi = 0; gi < G; gi++) seq_extract_item(a, gi);
        for (uint32_t gi = 0; gi < rec->n_commit; gi++) {
            const uint64_t w = seq_commit_item(a, gi, counts);
            sumsq += w * w;
            offsets[i0 + gi] = buf_first * SEQ_BLOCK + base + chain[gi];
        }
        rec->sumsq = sumsq;
        return 0;
    }
};

// offsets[i] = the word job i starts at, offsets[n_jobs] = the words the call consumed; out (optional): the walk matrix;
// counts (optional): steps, overflow reads, clamped reads, dead ends.  cfg->min_jobs = UINT64_MAX (or more than n_jobs): the
// plain sequential loop, one job after the other from a buffer that is re-expanded when a job runs dry.
inline int seq_host_walks(const SeqGraph &g, const uint32_t *starts, uint64_t n_jobs, uint32_t seed, const pw_seq_config *cfg,
                          uint64_t *offsets, uint32_t *out, SeqCounts *counts, pw_seq_info *info) {
    *info = pw_seq_info{};
    const uint32_t L = g.L;
    const SeqTuning t = seq_tuning(cfg, L);
    SeqCounts cn = {0, 0, 0, 0};
    if (n_jobs >= t.min_jobs) {
        SeqHostBackend be{g, starts, seed, offsets, out};
        if (int rc = seq_spec_drive(be, t, g.mode, L, n_jobs, info)) return rc;
        if (info->path == 1) {
            offsets[n_jobs] = info->words_consumed;
            if (counts) *counts = be.counts;
            return 0;
        }
        *info = pw_seq_info{};
        info->path = 2;
    }
    std::vector<uint32_t> words;
    uint64_t first = 0, S = 0;
    const uint64_t blocks = seq_min_blocks(L) + 64;
    for (uint64_t i = 0; i < n_jobs; i++) {
        offsets[i] = S;
        for (int attempt = 0;; attempt++) {
            if (words.empty() || attempt || S - first * SEQ_BLOCK >= words.size()) {
                first = S / SEQ_BLOCK;
                words.resize(blocks * SEQ_BLOCK);
                mt_words_host(seed, first * SEQ_BLOCK, words.size(), words.data());
                info->words_expanded += words.size();
            }
            const uint64_t at = S - first * SEQ_BLOCK;
            SeqWords ws{words.data() + at, 0, words.size() - at, false};
            SeqCounts job = {0, 0, 0, 0};
            if (seq_job(g, ws, starts[i], out ? out + i * ((uint64_t)L + 2) : (uint32_t *)nullptr, job)) {
                S += ws.pos;
                cn.steps += job.steps; cn.over += job.over; cn.clamp += job.clamp; cn.dead += job.dead;
                break;
            }
            if (attempt) return 1;   // a job longer than a fresh buffer: not a walk of this length
        }
        info->committed_jobs++;
    }
    offsets[n_jobs] = S;
    info->words_consumed = S;
    if (counts) *counts = cn;
    return 0;
}

// FirstOrderUnweighted on a bare CSR: the offsets alone
inline int seq_host_offsets(const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, const uint32_t *starts, uint64_t n_jobs,
                            uint32_t L, uint32_t seed, const pw_seq_config *cfg, uint64_t *offsets, pw_seq_info *info) {
    const SeqGraph g{indptr, indices, nullptr, indptr[n_nodes], nullptr, nullptr, nullptr, 0, 3, L};
    return seq_host_walks(g, starts, n_jobs, seed, cfg, offsets, nullptr, nullptr, info);
}

}  // namespace pw
