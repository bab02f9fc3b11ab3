// seq_spec.h -- the seeded alias / first-order modes job by job, and the speculation rounds that find many jobs' word
// offsets at a time.  Plain C++ apart from the PW_SQ_HD marker.  The rounds have a host form only (seq_spec_host.hpp:
// pw_selftest_seq_offsets, pw_selftest_seq_walks, tools/seq_spec_selfcheck.cpp); on the device seeded calls of these modes
// run walk_seq.hip.h's one-lane kernel.
//
// The reference draws a variable number of MT19937 words per step (masked rejection in np.random.randint), so the word
// offset S_i at which job i starts depends on every earlier draw.  That ONE integer per job is all that is sequential:
// given S_i, job i is independent of the others.  A round therefore has an exact base (job i0 starts at word S) and
//   plans      for g = 0 .. G-1 a window of candidate offsets for job i0 + g around S + g * mean (host),
//   walks      every (job, offset) candidate without storing its row: the words it would consume from there,
//   resolves   the one chain of candidates that starts at (i0, S) -- each candidate's end is the next job's start -- by
//              pointer doubling over the candidate table, up to the first end outside its window,
//   commits    the jobs on the chain: walked again from their now exact offsets, rows and counters written.
// A candidate is what the sequential walker would do if it reached that job at that offset, and only candidates on the
// true chain are used: the windows, the estimates behind them and the caps change how many jobs a round commits, never
// what is committed.
#pragma once
#include <math.h>
#include <stdint.h>

#include <chrono>
#include <vector>

#include "../../include/pecanpy_amd.h"

#if defined(__HIPCC__)
#define PW_SQ_HD __host__ __device__ inline
#else
#define PW_SQ_HD inline
#endif

namespace pw {

constexpr uint32_t SEQ_UNFINISHED = 0xffffffffu;   // a candidate that ran out of expanded words
constexpr uint32_t SEQ_NONE = 0xffffffffu;         // no successor: end outside the next window, unfinished, or last window
constexpr uint32_t SEQ_BLOCK = 624;                // words of one MT19937 block

// what a job reads: the CSR, the alias tables of its mode, the walk length
struct SeqGraph {
    const uint32_t *indptr, *indices;
    const float *data;               // nullptr: all 1.0
    uint32_t nnz;
    const uint64_t *alias_indptr;
    const uint32_t *alias_j;
    const float *alias_q;
    uint64_t n_alias;
    int mode;                        // pw_mode: 2 PreComp, 3 FirstOrderUnweighted, 4 PreCompFirstOrder
    uint32_t L;
};

struct SeqCounts {
    unsigned long long steps, over, clamp, dead;
};

// Word source over expanded stream words: w[0 .. end).  Past the end it hands out zeros and remembers: the job that
// asked is UNFINISHED, nothing waits for a word that is not there (a zero ends randint's rejection loop at once).
struct SeqWords {
    const uint32_t *w;
    uint64_t pos, end;
    bool dry;
    PW_SQ_HD uint32_t next32() {
        if (pos >= end) { dry = true; return 0u; }
        return w[pos++];
    }
    PW_SQ_HD bool failed() const { return dry; }
};

// np.random.random(): two words -> 53 bits
template <typename Rng> PW_SQ_HD double seq_random(Rng &rng) {
    const uint32_t a = rng.next32() >> 5, b = rng.next32() >> 6;
    return ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0);
}
// np.random.randint(n): n == 1 -> no words; else low bit_length(n-1) bits, reject >= n
template <typename Rng> PW_SQ_HD uint32_t seq_randint(Rng &rng, uint32_t n) {
    if (n == 1) return 0;
    const int nbits = 32 - __builtin_clz(n - 1);
    const uint32_t mask = nbits >= 32 ? 0xffffffffu : ((1u << nbits) - 1u);
    for (;;) {
        const uint32_t r = rng.next32() & mask;
        if (r < n) return r;
    }
}
template <typename Rng> PW_SQ_HD uint32_t seq_alias_draw(Rng &rng, const uint32_t *aj, const float *aq, uint32_t k) {
    const uint32_t kk = seq_randint(rng, k);
    const double u = seq_random(rng);
    return (u < (double)aq[kk]) ? kk : aj[kk];
}

// ONE job of a sequential-stream mode from `start`, drawing from rng: the walk of the reference's move_forward loop.
// row != nullptr: the row of the walk matrix (L + 2 words) is written; nullptr: only rng advances.  Returns false when rng
// ran dry (SeqWords); the row and the counts are then unfinished too.
//   randint(1) consumes nothing, random() two words, a start without neighbours nothing; an overflow read is
//   choice == d, clamped at nnz - 1 and counted; a table offset past the tables is clamped (off + d > n_alias).
// PreComp's first step is the first-order one: sequential float32 sum of the row, then the chain c += w[k] / tot
// (what seq_probs(..., has_prev = false) leaves in its buffer, added up), without a buffer.
template <typename Rng>
PW_SQ_HD bool seq_job(const SeqGraph &g, Rng &rng, uint32_t start, uint32_t *row, SeqCounts &cn) {
    const uint32_t L = g.L;
    if (row) {
        for (uint32_t z = 0; z < L + 2; z++) row[z] = 0;
        row[0] = start;
        row[L + 1] = L + 1;
    }
    uint32_t cur = start, prev = 0;
    for (uint32_t j = 1; j <= L; j++) {
        const uint32_t s0 = g.indptr[cur], d = g.indptr[cur + 1] - s0;
        if (d == 0) {
            if (row) row[L + 1] = j;
            if (j > 1) cn.dead++;
            break;
        }
        uint32_t choice;
        if (g.mode == 3) {
            choice = seq_randint(rng, d);
        } else if (g.mode == 4) {
            choice = seq_alias_draw(rng, g.alias_j + s0, g.alias_q + s0, d);
        } else if (j == 1) {
            float tot = 0.0f;
            for (uint32_t k = 0; k < d; k++) tot += g.data ? g.data[s0 + k] : 1.0f;
            const double r = seq_random(rng);
            float c = 0.0f;
            choice = d;
            for (uint32_t k = 0; k < d; k++) {
                c += (g.data ? g.data[s0 + k] : 1.0f) / tot;
                if ((double)c >= r) { choice = k; break; }
            }
        } else {
            uint32_t lo = 0, hi = d;  // np.searchsorted(row(cur), prev), left
            while (hi > lo) {
                const uint32_t mid = (lo + hi) >> 1;
                if (g.indices[s0 + mid] < prev) lo = mid + 1; else hi = mid;
            }
            uint64_t off = g.alias_indptr[cur] + (uint64_t)d * lo;
            if (off + d > g.n_alias) off = g.n_alias - d;  // reference would read past the table
            choice = seq_alias_draw(rng, g.alias_j + off, g.alias_q + off, d);
        }
        if (rng.failed()) return false;
        uint64_t pos = (uint64_t)s0 + choice;
        if (choice >= d) {
            cn.over++;
            if (pos >= g.nnz) { pos = g.nnz - 1; cn.clamp++; }
        }
        const uint32_t nxt = g.indices[pos];
        if (row) row[j] = nxt;
        prev = cur;
        cur = nxt;
        cn.steps++;
    }
    return true;
}

// ---- a round ---------------------------------------------------------------------------------------------------------
// window of job i0 + g: candidate offsets base + lo .. base + lo + width - 1; its candidates are cbase .. cbase + width - 1
struct SeqWindow {
    uint32_t lo, width, cbase;
};
// what a round reports (written by ONE lane of the resolve; sumsq: added up by the commit, over the whole call)
struct SeqRoundRec {
    uint32_t n_commit;             // jobs i0 .. i0 + n_commit - 1 are final
    uint32_t missed;               // 1: the chain ended at an offset outside the next window (0: last window, or unfinished)
    uint64_t words;                // the committed jobs consumed this many: the next base is base + words
    unsigned long long sumsq;      // sum of (words of a job)^2 over every job the call committed so far
};

struct SeqRoundArgs {
    SeqGraph g;
    const uint32_t *starts;        // of the whole call
    const uint32_t *words;         // the word buffer; words[base] = the word job i0 starts at
    uint64_t n_words, base;        // words in the buffer, position of the base in it
    uint64_t i0;
    const SeqWindow *win;
    uint32_t G, total;             // windows, candidates
    uint32_t *consumed;            // [total] words a candidate consumed, or SEQ_UNFINISHED
    uint32_t *jump;                // [levels][stride]: jump[k][c] = the candidate 2^k jobs behind c on its chain, or SEQ_NONE
    uint32_t stride;
    uint32_t *chain;               // [G] offset (relative to the base) of the chain's candidate in window g
    SeqRoundRec *rec;
    uint32_t *out;                 // walk matrix of the whole call
};

PW_SQ_HD uint32_t seq_window_of(const SeqWindow *win, uint32_t G, uint32_t c) {   // the g with cbase[g] <= c < cbase[g + 1]
    uint32_t lo = 0, hi = G;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (win[mid].cbase <= c) lo = mid; else hi = mid;
    }
    return lo;
}

PW_SQ_HD SeqWords seq_words_at(const SeqRoundArgs &a, uint64_t rel) {
    const uint64_t at = a.base + rel;
    if (at >= a.n_words) return SeqWords{a.words, 0, 0, false};   // (a job that draws nothing still finishes)
    return SeqWords{a.words + at, 0, a.n_words - at, false};
}

// candidate c: the words job i0 + g would consume from offset lo_g + (c - cbase_g); no row, no counters
PW_SQ_HD void seq_candidate_item(const SeqRoundArgs &a, uint32_t c) {
    const uint32_t g = seq_window_of(a.win, a.G, c);
    SeqWords ws = seq_words_at(a, (uint64_t)a.win[g].lo + (c - a.win[g].cbase));
    SeqCounts cn = {0, 0, 0, 0};
    const bool ok = seq_job(a.g, ws, a.starts[a.i0 + g], (uint32_t *)nullptr, cn);
    a.consumed[c] = ok ? (uint32_t)ws.pos : SEQ_UNFINISHED;
}

// the candidate of window g + 1 that starts where candidate c of window g ends
PW_SQ_HD uint32_t seq_succ(const SeqRoundArgs &a, uint32_t g, uint32_t c) {
    if (g + 1 >= a.G || a.consumed[c] == SEQ_UNFINISHED) return SEQ_NONE;
    const uint64_t rel = (uint64_t)a.win[g].lo + (c - a.win[g].cbase) + a.consumed[c];
    const SeqWindow nw = a.win[g + 1];
    if (rel < nw.lo || rel >= (uint64_t)nw.lo + nw.width) return SEQ_NONE;
    return nw.cbase + (uint32_t)(rel - nw.lo);
}
PW_SQ_HD void seq_succ_item(const SeqRoundArgs &a, uint32_t c) { a.jump[c] = seq_succ(a, seq_window_of(a.win, a.G, c), c); }
// level k from level k - 1
PW_SQ_HD void seq_double_item(const SeqRoundArgs &a, uint32_t k, uint32_t c) {
    const uint32_t *prev = a.jump + (size_t)(k - 1) * a.stride;
    const uint32_t mid = prev[c];
    a.jump[(size_t)k * a.stride + c] = mid == SEQ_NONE ? SEQ_NONE : prev[mid];
}
// depth g of the chain from candidate 0 (window 0 holds the exact base alone): one jump per set bit of g.  The lane that
// finds the chain's last finished candidate writes the record; lane 0 writes it when job i0 itself is unfinished.
PW_SQ_HD void seq_extract_item(const SeqRoundArgs &a, uint32_t g) {
    uint32_t node = 0;
    for (uint32_t k = 0; (g >> k) != 0 && node != SEQ_NONE; k++)
        if ((g >> k) & 1u) node = a.jump[(size_t)k * a.stride + node];
    if (node == SEQ_NONE) return;
    const uint32_t rel = a.win[g].lo + (node - a.win[g].cbase);
    a.chain[g] = rel;
    if (a.consumed[node] == SEQ_UNFINISHED) {
        if (g == 0) { a.rec->n_commit = 0; a.rec->missed = 0; a.rec->words = 0; }
        return;
    }
    const uint32_t nxt = seq_succ(a, g, node);
    if (nxt != SEQ_NONE && a.consumed[nxt] != SEQ_UNFINISHED) return;
    a.rec->n_commit = g + 1;
    a.rec->missed = (nxt == SEQ_NONE && g + 1 < a.G) ? 1u : 0u;
    a.rec->words = (uint64_t)rel + a.consumed[node];
}
// job i0 + g from its exact offset: the row, its counts, the words it consumed
PW_SQ_HD uint64_t seq_commit_item(const SeqRoundArgs &a, uint32_t g, SeqCounts &cn) {
    SeqWords ws = seq_words_at(a, a.chain[g]);
    (void)seq_job(a.g, ws, a.starts[a.i0 + g], a.out ? a.out + (a.i0 + g) * ((uint64_t)a.g.L + 2) : (uint32_t *)nullptr, cn);
    return ws.pos;
}
PW_SQ_HD uint32_t seq_levels(uint32_t G) {   // jump levels a round of G windows needs: the bits of G - 1
    uint32_t k = 0;
    while (G > 1 && ((G - 1) >> k) != 0) k++;
    return k;
}

// ---- the plan and the round loop (host) ------------------------------------------------------------------------------
struct SeqTuning {
    uint32_t jobs_per_round, max_candidates, buffer_blocks;
    uint64_t min_jobs;
    double k;                       // window half width in deviations; 0: the centre alone
    uint32_t slack;
    double force_mean, force_sigma; // > 0: in place of the running estimates
};

constexpr uint32_t SEQ_JOBS_PER_ROUND = 512, SEQ_MAX_JOBS_PER_ROUND = 4096;
constexpr uint32_t SEQ_MAX_CANDIDATES = 1u << 19, SEQ_CANDIDATES_LIMIT = 1u << 22;
constexpr uint32_t SEQ_BUFFER_BLOCKS = 1u << 16, SEQ_BUFFER_LIMIT = 1u << 20;   // 163 MB of words; at most 2.6 GB
// Below this many jobs a call takes the plain sequential loop.  A GUESS: nothing has been measured on a device.
constexpr uint64_t SEQ_MIN_JOBS = 64;

inline uint32_t seq_min_blocks(uint32_t L) {   // one job of 3 L + 4096 words from anywhere inside the first block
    return (uint32_t)((3ull * L + 4096 + SEQ_BLOCK - 1) / SEQ_BLOCK) + 1;
}

inline SeqTuning seq_tuning(const pw_seq_config *cfg, uint32_t L) {
    pw_seq_config c = {};
    if (cfg) c = *cfg;
    SeqTuning t;
    t.jobs_per_round = c.jobs_per_round ? c.jobs_per_round : SEQ_JOBS_PER_ROUND;
    if (t.jobs_per_round > SEQ_MAX_JOBS_PER_ROUND) t.jobs_per_round = SEQ_MAX_JOBS_PER_ROUND;
    t.max_candidates = c.max_candidates ? c.max_candidates : SEQ_MAX_CANDIDATES;
    if (t.max_candidates > SEQ_CANDIDATES_LIMIT) t.max_candidates = SEQ_CANDIDATES_LIMIT;
    t.buffer_blocks = c.word_buffer_blocks ? c.word_buffer_blocks : SEQ_BUFFER_BLOCKS;
    if (t.buffer_blocks > SEQ_BUFFER_LIMIT) t.buffer_blocks = SEQ_BUFFER_LIMIT;
    if (t.buffer_blocks < seq_min_blocks(L)) t.buffer_blocks = seq_min_blocks(L);
    t.min_jobs = c.min_jobs ? c.min_jobs : SEQ_MIN_JOBS;
    t.k = c.window_sigmas == 0.0f ? 3.0 : (c.window_sigmas < 0.0f ? 0.0 : (double)c.window_sigmas);
    t.slack = t.k > 0.0 ? 2u : 0u;
    t.force_mean = c.force_mean > 0.0f ? (double)c.force_mean : 0.0;
    t.force_sigma = c.force_sigma > 0.0f ? (double)c.force_sigma : 0.0;
    return t;
}

// running mean and deviation of the words per committed job; before any job: a guess from the mode and L
struct SeqEstimate {
    uint64_t n = 0;
    double sum = 0, sumsq = 0, mu0 = 0, sigma0 = 0;
    SeqEstimate(int mode, uint32_t L) {
        mu0 = (mode == 3 ? 1.5 : 3.5) * L;   // randint: one word and its rejections; an alias draw: two more
        sigma0 = sqrt((double)L);
    }
    double mean() const { return n ? sum / (double)n : mu0; }
    double sigma() const {
        if (!n) return sigma0;
        const double m = mean(), v = sumsq / (double)n - m * m;
        return v > 0 ? sqrt(v) : 0.0;
    }
    bool settled() const { return n >= 32; }
};

// The windows of a round: centre_g = round(g mu), half_0 = 0, half_g = ceil(k sigma sqrt(g + g^2 / n)) + slack -- the
// spread of g jobs, and of a mean known from n of them -- plus, while fewer than 32 jobs are known, 0.3 mu0 g for a first
// guess that is off.  G = the windows that fit the candidate cap and whose jobs can end inside `reach_limit` words, and no
// more than a mean known from n jobs carries.
inline uint32_t seq_plan_round(const SeqTuning &t, const SeqEstimate &est, uint64_t jobs_left, uint64_t reach_limit, uint64_t job_reach,
                               std::vector<SeqWindow> &win, uint32_t *total) {
    const double mu = t.force_mean > 0 ? t.force_mean : est.mean();
    const double sigma = t.force_sigma > 0 ? t.force_sigma : est.sigma();
    const bool forced = t.force_mean > 0 || t.force_sigma > 0;
    const double n_known = est.n ? (double)est.n : 1.0;
    const double drift = (forced || est.settled() || t.k == 0.0) ? 0.0 : 0.3 * est.mu0;
    uint64_t gmax = t.jobs_per_round < jobs_left ? t.jobs_per_round : jobs_left;
    if (!forced) {   // a mean known from n jobs carries about 4 n windows before its own error outgrows their spread
        const uint64_t carry = est.settled() ? 4 * est.n : 32;
        if (gmax > carry) gmax = carry;
    }
    win.clear();
    uint64_t cands = 0;
    for (uint64_t g = 0; g < gmax; g++) {
        const uint64_t centre = (uint64_t)llround((double)g * mu);
        uint64_t half = 0;
        if (g) half = (uint64_t)ceil(t.k * sigma * sqrt((double)g + (forced ? 0.0 : (double)g * (double)g / n_known)) + drift * (double)g) + t.slack;
        const uint64_t lo = centre > half ? centre - half : 0, hi = centre + half;
        if (g && (cands + (hi - lo + 1) > t.max_candidates || hi + job_reach > reach_limit)) break;
        win.push_back(SeqWindow{(uint32_t)lo, (uint32_t)(hi - lo + 1), (uint32_t)cands});
        cands += hi - lo + 1;
    }
    *total = (uint32_t)cands;
    return (uint32_t)win.size();
}

// The round loop over a backend:
//   int fill(uint64_t first_block, uint64_t n_blocks)        the words of these blocks into the buffer
//   int round(uint64_t i0, uint64_t base, uint64_t n_words, const SeqWindow *win, uint32_t G, uint32_t total, SeqRoundRec *rec)
//                                                            candidates, resolve, commit; the record back on the host
// Returns 0 with info->path = 1, or with info->path = 2 when the caller has to hand the whole call to the sequential
// walker (job i0 unfinished with the buffer starting at its block and at full size); a backend's error otherwise.
// Every pass of the loop commits a job or is the one retry of its base: at most 2 n_jobs passes, nothing spins.
template <typename Backend>
int seq_spec_drive(Backend &be, const SeqTuning &t, int mode, uint32_t L, uint64_t n_jobs, pw_seq_info *info) {
    SeqEstimate est(mode, L);
    std::vector<SeqWindow> win;
    uint64_t S = 0, i0 = 0, buf_first = 0, buf_blocks = 0;
    const uint64_t cap = t.buffer_blocks;
    info->path = 1;
    while (i0 < n_jobs) {
        const auto t0 = std::chrono::steady_clock::now();
        // words a job may need behind its start: from what was seen, never from the forced figures
        const uint64_t job_reach = (uint64_t)ceil(est.mean() + 4.0 * est.sigma() + (est.settled() ? 0.0 : est.mu0)) + 64;
        uint32_t total = 0;
        const uint32_t G = seq_plan_round(t, est, n_jobs - i0, cap * SEQ_BLOCK - SEQ_BLOCK, job_reach, win, &total);
        const uint64_t need_end = S + win[G - 1].lo + win[G - 1].width + job_reach;
        const bool at_full = buf_blocks == cap && buf_first == S / SEQ_BLOCK;
        info->plan_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (need_end > (buf_first + buf_blocks) * SEQ_BLOCK && !at_full) {
            const uint64_t first = S / SEQ_BLOCK;
            const double rest = (double)(n_jobs - i0) * (est.mean() + est.sigma()) + (double)job_reach;
            uint64_t want_end = need_end > S + (uint64_t)rest ? need_end : S + (uint64_t)rest;
            uint64_t nb = (want_end + SEQ_BLOCK - 1) / SEQ_BLOCK - first;
            if (nb > cap) nb = cap;
            if (nb < seq_min_blocks(L)) nb = seq_min_blocks(L);
            if (int rc = be.fill(first, nb)) return rc;
            buf_first = first;
            buf_blocks = nb;
            info->words_expanded += nb * SEQ_BLOCK;
        }
        SeqRoundRec rec = {0, 0, 0, 0};
        if (int rc = be.round(i0, S - buf_first * SEQ_BLOCK, buf_blocks * SEQ_BLOCK, win.data(), G, total, &rec)) return rc;
        info->candidate_walks += total;
        if (rec.n_commit == 0) {   // job i0 itself ran out of words: expand as far as the buffer goes and repeat the round, once
            if (buf_blocks == cap && buf_first == S / SEQ_BLOCK) { info->path = 2; return 0; }
            info->unfinished_retries++;
            if (int rc = be.fill(S / SEQ_BLOCK, cap)) return rc;
            buf_first = S / SEQ_BLOCK;
            buf_blocks = cap;
            info->words_expanded += cap * SEQ_BLOCK;
            continue;
        }
        info->rounds++;
        info->committed_jobs += rec.n_commit;
        info->window_misses += rec.missed;
        est.n += rec.n_commit;
        est.sum += (double)rec.words;
        est.sumsq = (double)rec.sumsq;
        S += rec.words;
        i0 += rec.n_commit;
    }
    info->words_consumed = S;
    return 0;
}

}  // namespace pw
