// sgns.hip.h -- skip-gram with negative sampling over a walk matrix (gfx950): the stage that follows the walks in
// the reference's pipeline (Base.embed / cli.learn_embeddings: gensim Word2Vec(walks, sg=1, negative=5, window, epochs),
// src/pecanpy/pecanpy.py:276-290, cli.py:307-325).  SURVEY.md section 8(f) rank 4.  The model and update rule are
// word2vec.c's (gensim's sg / negative path):
//   a walk is thinned by word2vec's frequent-word subsampling, windows are taken over what is left; for every centre
//   position a window shrunk by a random amount, and for every context word c in it: input vector syn0[c], targets =
//   the centre (label 1) and `negative` words drawn from the unigram^0.75 table (label 0),
//   g = (label - sigmoid(v.u)) * lr, u += g v, v += sum g u; learning rate decaying linearly over the run.
// Every random choice is a hash of (seed, epoch, walk, position[, context, draw]) -- no generator state -- so the set
// of updates is a function of the seed alone; what the hardware adds is their ORDER.
//
// Walk-resident kernel: a wavefront owns a WALK and visits its positions in order (hogwild -- unsynchronised, like gensim's
// worker threads -- is over walks).  Per (epoch, walk) the subsampling decision of every occurrence is taken once, 64
// occurrences per ballot word, and the survivors are compacted into LDS as (position, node) pairs; the window of a centre
// over the thinned walk is then index arithmetic on that list: no hash and no dependent keep[row[p]] load per neighbour.
// Per (centre, context) pair the chain of target indices (it depends on no vector data) is evaluated first and the rows of
// syn1 are requested together, SGNS_GROUP at a time, then consumed in order; a target that repeats inside a group is read
// again after the row was written, so the sequential semantics hold.  The arithmetic order is the restatement's
// (oracle/sgns_ref.c): component k on lane k % 64, per-lane partial sums in ascending k, xor butterfly 32 -> 1, neu1e
// accumulated in draw order.  With ONE wavefront (pw_sgns_train*: workers = 1) the updates run in sentence order and the
// result is compared with that restatement within float tolerance (tests/test_gpu_sgns.py, tests/test_gpu_embed_device.py).
// The PARALLEL form (several wavefronts of a workgroup on their LDS slices, several workgroups, the stride over the walks,
// the rounding of workers to whole workgroups, one wavefront per workgroup from L = 2048, exactly 64 KiB of LDS at L = 2047
// and L = 8191) is held to two things that need no tolerance of their own (tests/test_gpu_sgns_waves.py): on a corpus whose
// walk wk names only rows of component wk % n_waves, with negative = 0, no two wavefronts share a row and each takes its
// walks in ascending order, so the vectors equal those of workers = 1 bit for bit; and the two counters, hashes of
// (seed, epoch, walk, position), equal the restatement's counts in any run, a racing one with negatives included.  What
// a racing run's vectors are compared by stays statistical (similarity structure, tests/test_gpu_sgns.py).
// The kernel writes global memory through vector stores only; the two counters are per-lane atomics of lane 0, once per walk.
// Frozen rows (the LOCK instances): a row whose bit is set in lock0 / lock1 is read like any other and never stored; what is
// evaluated -- pairs, draws, dot, loss, g, counters -- is what the LOCK = false instance evaluates on the same values.
#pragma once
#include <cstddef>
#include "wave.h"

namespace pw {

struct SgnsArgs {
    const uint32_t *__restrict__ walks;   // [n_walks, L + 2], last cell = number of nodes in the walk
    uint64_t n_walks;
    uint32_t L;
    uint32_t dim, window, negative;
    float *syn0, *syn1;                   // [n_nodes, dim]
    const uint32_t *__restrict__ table;   // negative-sampling table (word2vec's unigram^0.75 table)
    uint32_t table_size;
    const float *__restrict__ keep;       // per word: probability of keeping an occurrence (subsampling), or nullptr
    float alpha, min_alpha;
    uint64_t item_base;                   // n_items * (global epoch index): what the hashes of this launch start from
    uint64_t lr_base, lr_total;           // n_items * (epochs of the schedule done / in all): where the learning rate stands
    uint64_t seed;
    uint32_t n_waves;                     // wavefronts of the launch (the stride of a wavefront over the walks)
    unsigned long long *counters;         // [0] occurrences that survived the subsampling, [1] (centre, context) pairs trained
    double *walk_loss;                    // LOSS instances: [n_walks] sum of the loss terms of a walk's evaluations, one writer each
    unsigned long long *walk_evals;       // LOSS instances: [n_walks] number of those evaluations
    // LOCK instances: frozen rows of syn0 / syn1, bit r % 32 of word r / 32 covers row r; nullptr = no row of that matrix
    const uint32_t *__restrict__ lock0, *__restrict__ lock1;
};

__device__ __forceinline__ uint64_t sgns_mix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

constexpr int SGNS_MAX_PER_LANE = 8;   // dim <= 512
constexpr int SGNS_GROUP = 6;          // target rows requested together (negative + 1 of the default model)

// LDS of one wavefront: positions and nodes of the occurrences of its walk that survived the subsampling
__host__ __device__ inline size_t sgns_lds_bytes_per_wave(uint32_t L) { return sizeof(uint32_t) * 2 * ((size_t)L + 1); }

// PER: components per lane, 64 * (PER - 1) < dim <= 64 * PER: only the last component of a lane can lie beyond dim, so one
// lane mask (`tail`) guards it and the others are read and written without a guard
// LOSS: every trained evaluation also adds its term of the skip-gram / negative-sampling loss (gensim's definition:
// softplus(-dot) for the centre, softplus(dot) for a negative) to a per-walk sum, taken in float64 from the exact `dot` the
// update uses -- before the row is written, not from the clipped sigmoid, so a saturated evaluation contributes its finite
// term.  `dot` is wave-uniform after wave_sum: every lane carries the same sum and lane 0 stores it, once per walk, with
// plain vector stores.  The update arithmetic is the same instructions on the same values; the LOSS = false instances are
// the kernel without any of this.
// LOCK: rows can be frozen.  The row index of a pair's context (`ctx`) and of every target (`tgt[t]`) is wave-uniform, so its
// lock bit is one scalar-cache read: the context's with the pair, those of a group's SGNS_GROUP targets together, right after
// the table reads that name them.  A frozen syn0 row skips the store of `v` at the end of the pair; a frozen syn1 row skips
// the store of `u` and still adds g * u to `acc`, so a free context row learns from a frozen target.  A frozen target that
// repeats inside a group is read again like a free one: nothing wrote it, the values are the same.  Everything else --
// ballot, window, the chain `rs`, `dot`, the loss term, `sig`, `g`, `lr`, the counters -- is the same code: a lock changes what
// is written, not what is evaluated.  The LOCK = false instances never look at lock0 / lock1 and are the kernel without any of
// this; the driver launches them whenever no row of either matrix is frozen.  They keep the kernel's four arguments: the two
// lock arguments are a pack (LK = uint32_t, uint32_t) that only the LOCK instances have.
__device__ __forceinline__ const uint32_t *sgns_lock_arg(int) { return nullptr; }
__device__ __forceinline__ const uint32_t *sgns_lock_arg(int which, const uint32_t *lock0, const uint32_t *lock1) { return which ? lock1 : lock0; }
template <int PER, bool LOSS = false, bool LOCK = false, typename... LK>
__global__ void __launch_bounds__(256)
sgns_walk_kernel(SgnsArgs a, const uint32_t *__restrict__ walks, const uint32_t *__restrict__ table, const float *__restrict__ keep,
                 const LK *__restrict__... lk) {
    // (walks / table / keep / the lock words once more as arguments of their own: __restrict__ on a kernel argument is what
    // lets the compiler read them through the scalar cache although the loop stores to syn0 / syn1)
    static_assert(sizeof...(LK) == (LOCK ? 2 : 0), "lock0 and lock1 are arguments of the LOCK instances and of no other");
    const uint32_t *const lock0 = sgns_lock_arg(0, lk...), *const lock1 = sgns_lock_arg(1, lk...);
    extern __shared__ uint32_t sgns_lds[];
    const int lane = lane_id();
    const uint32_t wib = readfirst_u32(threadIdx.x / WAVE), wpb = blockDim.x / WAVE;   // (uniform: walk state lives in SGPRs)
    const uint32_t wave = blockIdx.x * wpb + wib;
    const uint32_t L1 = a.L + 1;
    const bool tail = (uint32_t)lane < a.dim - 64u * (PER - 1);
    uint32_t *kpos = sgns_lds + (size_t)wib * 2 * L1, *knode = kpos + L1;
    // arguments that are needed once per walk or once per centre are read again from the kernarg segment where they are
    // used (wave.h: kernarg) instead of living in SGPRs across the pair loop, which needs every one of them
#define SGNS_ARG(T, field) kernarg<T>(offsetof(SgnsArgs, field))
    for (uint64_t wk = wave; wk < SGNS_ARG(uint64_t, n_walks); wk += SGNS_ARG(uint32_t, n_waves)) {
        const uint32_t *row = walks + wk * (uint64_t)(a.L + 2);      // (L < 8192)
        const uint32_t len = min(row[L1], L1);                        // (the count kernel rejected longer; bounds the LDS writes)
        const uint64_t occ0 = SGNS_ARG(uint64_t, item_base) + wk * (uint64_t)L1;
#define occ(p) sgns_mix(a.seed ^ (occ0 + (p)) * 0x9E3779B97F4A7C15ull)
        // which occurrences of this epoch survive the subsampling: one ballot per 64, compacted in walk order
        wave_lds_fence();                                             // (the previous walk's readers are done)
        uint32_t nk = 0;
        for (uint32_t base = 0; base < len; base += WAVE) {
            const uint32_t p = base + lane;
            bool k = p < len;
            uint32_t node = 0;
            if (k) {
                node = row[p];
                if (keep) k = (float)(occ(p) >> 40) * (1.0f / 16777216.0f) < keep[node];
            }
            const uint64_t m = ballot(k);
            if (k) {
                const uint32_t j = nk + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                kpos[j] = p;
                knode[j] = node;
            }
            nk += (uint32_t)__popcll(m);
        }
        wave_lds_fence();
        uint32_t n_pairs = 0;
        double loss = 0.0;
        unsigned long long n_evals = 0;
        for (uint32_t j = 0; j < nk; j++) {
            const uint32_t pos = readfirst_u32(kpos[j]), centre = readfirst_u32(knode[j]);
            uint64_t rs = sgns_mix(occ(pos));
            const uint32_t window = SGNS_ARG(uint32_t, window);
            const uint32_t eff = window - (uint32_t)(rs % window);                              // shrunk window, 1 .. window
            const float alpha = SGNS_ARG(float, alpha), min_alpha = SGNS_ARG(float, min_alpha);
            // the item's place in the schedule: its place in the hash sequence moved from item_base to lr_base (mod 2^64; the
            // two coincide in a one-shot run)
            const uint64_t lr_shift = SGNS_ARG(uint64_t, lr_base) - SGNS_ARG(uint64_t, item_base);
            const float lr = fmaxf(min_alpha, alpha - (alpha - min_alpha) * (float)((double)(occ0 + pos + lr_shift) / (double)SGNS_ARG(uint64_t, lr_total)));
            // the window over the thinned walk: up to eff survivors on either side
            const uint32_t lo = j - min(eff, j), hi = j + min(eff, nk - 1 - j);
            for (uint32_t i = lo; i <= hi; i++) {
                if (i == j) continue;
                const uint32_t c = readfirst_u32(kpos[i]), ctx = readfirst_u32(knode[i]);
                rs = sgns_mix(rs + c);
                float *v = a.syn0 + (uint64_t)ctx * a.dim;
                bool vlock = false;                                    // (uniform) the context's row of syn0 is frozen
                if (LOCK && lock0) vlock = lock0[ctx >> 5] >> (ctx & 31u) & 1u;
                float vin[PER], acc[PER];
#pragma unroll
                for (int s = 0; s < PER; s++) {
                    const uint32_t k = (uint32_t)s * WAVE + lane;
                    vin[s] = (s < PER - 1 || tail) ? v[k] : 0.0f;
                    acc[s] = 0.0f;
                }
                for (uint32_t g0 = 0; g0 <= a.negative; g0 += SGNS_GROUP) {
                    // the targets of this group: the chain of draws reads no vector
                    uint32_t tgt[SGNS_GROUP];
                    uint32_t act = 0;                                  // bit t: target t is trained
#pragma unroll
                    for (int t = 0; t < SGNS_GROUP; t++) {
                        // (no branch: the table reads of a group are independent of each other and go out together)
                        const uint32_t ng = g0 + (uint32_t)t;
                        const bool draw = ng != 0 && ng <= a.negative;
                        const uint64_t next = sgns_mix(rs + ng);
                        rs = draw ? next : rs;
                        const uint32_t drawn = table[(uint32_t)(rs >> 16) % a.table_size];
                        tgt[t] = draw ? drawn : centre;
                        act |= (uint32_t)(ng <= a.negative && !(draw && drawn == centre)) << t;
                    }
                    uint32_t ulock = 0;                                // bit t: target t's row of syn1 is frozen
                    if (LOCK && lock1) {
#pragma unroll
                        for (int t = 0; t < SGNS_GROUP; t++) ulock |= (lock1[tgt[t] >> 5] >> (tgt[t] & 31u) & 1u) << t;
                    }
                    uint32_t again = 0;                                // bit t: an earlier target of the group writes row t first
#pragma unroll
                    for (int t = 1; t < SGNS_GROUP; t++)
#pragma unroll
                        for (int e = 0; e < t; e++) again |= (uint32_t)((act >> e & 1u) && tgt[e] == tgt[t]) << t;
                    // their rows, requested together
                    float uu[SGNS_GROUP][PER];
#pragma unroll
                    for (int t = 0; t < SGNS_GROUP; t++) {
                        const float *u = a.syn1 + (uint64_t)tgt[t] * a.dim;
#pragma unroll
                        for (int s = 0; s < PER; s++) {
                            const uint32_t k = (uint32_t)s * WAVE + lane;
                            uu[t][s] = ((act >> t & 1u) && (s < PER - 1 || tail)) ? u[k] : 0.0f;
                        }
                    }
                    // consumed in order
#pragma unroll
                    for (int t = 0; t < SGNS_GROUP; t++) {
                        if (!(act >> t & 1u)) continue;
                        float *u = a.syn1 + (uint64_t)tgt[t] * a.dim;
                        if (again >> t & 1u) {                          // read the row again, after the store
#pragma unroll
                            for (int s = 0; s < PER; s++) {
                                const uint32_t k = (uint32_t)s * WAVE + lane;
                                uu[t][s] = (s < PER - 1 || tail) ? u[k] : 0.0f;
                            }
                        }
                        float dot = 0.0f;
#pragma unroll
                        for (int s = 0; s < PER; s++) dot += vin[s] * uu[t][s];
                        dot = wave_sum(dot);
                        if (LOSS) {                                     // softplus(x) = max(x, 0) + log1p(exp(-|x|)), x = -dot for label 1
                            const double x = g0 + (uint32_t)t == 0 ? -(double)dot : (double)dot;
                            loss += fmax(x, 0.0) + log1p(exp(-fabs(x)));
                            n_evals++;
                        }
                        const float sig = dot > 6.0f ? 1.0f : (dot < -6.0f ? 0.0f : 1.0f / (1.0f + __expf(-dot)));
                        const float g = ((g0 + (uint32_t)t == 0 ? 1.0f : 0.0f) - sig) * lr;
#pragma unroll
                        for (int s = 0; s < PER; s++) {
                            const uint32_t k = (uint32_t)s * WAVE + lane;
                            if (s < PER - 1 || tail) {
                                acc[s] += g * uu[t][s];
                                if (!(LOCK && (ulock >> t & 1u))) u[k] = uu[t][s] + g * vin[s];
                            }
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < PER; s++) {
                    const uint32_t k = (uint32_t)s * WAVE + lane;
                    if ((s < PER - 1 || tail) && !(LOCK && vlock)) v[k] = vin[s] + acc[s];
                }
                n_pairs++;
            }
        }
#undef occ
        unsigned long long *counters = SGNS_ARG(unsigned long long *, counters);
        if (counters && lane == 0 && nk) {                            // (per walk: two atomics against thousands of row updates)
            atomicAdd(&counters[0], (unsigned long long)nk);
            atomicAdd(&counters[1], (unsigned long long)n_pairs);
        }
        if (LOSS && lane == 0) {                                       // (every walk of a launch is visited once: one writer per cell;
            SGNS_ARG(double *, walk_loss)[wk] = loss;                  //  a walk without survivors writes zeros)
            SGNS_ARG(unsigned long long *, walk_evals)[wk] = n_evals;
        }
    }
#undef SGNS_ARG
}

// The read-only form: the evaluations sgns_walk_kernel<PER, true> performs for the epoch of a.item_base on the matrix
// `walks` -- the same ballot and compaction, the same shrunk window, the same chain `rs`, a negative that equals the centre
// skipped -- scored against syn0 / syn1 as they are, and no update: no learning rate is read and no vector written.  `dot` is
// the training kernel's (component k on lane k % 64, per-lane partial sums in ascending k, xor butterfly 32 -> 1), the term
// the LOSS instances' float64 expression, the per-walk sum is taken in evaluation order with one writer per walk, and
// sgns_loss_reduce_kernel follows: the result is a function of (seed, epoch, matrix, vectors) and bit-identical at any number
// of wavefronts -- a.n_waves is the stride over the walks and nothing else.  What the missing stores buy:
//   * syn0 / syn1 are const __restrict__, no row is read again after a write, and all SGNS_GROUP target rows of a group are
//     requested without a guard on `act` together with the context row (a skipped target names the centre's row: a valid
//     address whose dot is dropped), so a pair's loads go out in one batch with no branch between them;
//   * `dot` is wave-uniform, so the float64 softplus need not run once per evaluation on 64 identical lanes: evaluation e of
//     a batch parks x = -+dot in lane e, and when 64 are parked (or the walk ends) every lane takes the term of its own x at
//     once; the terms are then added to the walk's sum one lane after the other -- the sequential order of the training
//     kernel, so the sum has its bits;
//   * nothing races, so the launch takes as many wavefronts as the corpus feeds whatever the session's `workers` is.
// LDS per wavefront and the workgroup shapes are the training kernel's (sgns_lds_bytes_per_wave; one wavefront per workgroup
// from L = 2048).  Global memory is written through vector stores only: the two per-walk cells by lane 0, the two counters
// by lane 0's atomics, once per walk.
template <int PER>
__global__ void __launch_bounds__(256)
sgns_eval_kernel(SgnsArgs a, const uint32_t *__restrict__ walks, const uint32_t *__restrict__ table, const float *__restrict__ keep,
                 const float *__restrict__ syn0, const float *__restrict__ syn1) {
    extern __shared__ uint32_t sgns_lds[];
    const int lane = lane_id();
    const uint32_t wib = readfirst_u32(threadIdx.x / WAVE), wpb = blockDim.x / WAVE;
    const uint32_t wave = blockIdx.x * wpb + wib;
    const uint32_t L1 = a.L + 1;
    const bool tail = (uint32_t)lane < a.dim - 64u * (PER - 1);
    uint32_t *kpos = sgns_lds + (size_t)wib * 2 * L1, *knode = kpos + L1;
    for (uint64_t wk = wave; wk < a.n_walks; wk += a.n_waves) {
        const uint32_t *row = walks + wk * (uint64_t)(a.L + 2);      // (L < 8192)
        const uint32_t len = min(row[L1], L1);                        // (the count kernel rejected longer; bounds the LDS writes)
        const uint64_t occ0 = a.item_base + wk * (uint64_t)L1;
#define occ(p) sgns_mix(a.seed ^ (occ0 + (p)) * 0x9E3779B97F4A7C15ull)
        wave_lds_fence();                                             // (the previous walk's readers are done)
        uint32_t nk = 0;
        for (uint32_t base = 0; base < len; base += WAVE) {
            const uint32_t p = base + lane;
            bool k = p < len;
            uint32_t node = 0;
            if (k) {
                node = row[p];
                if (keep) k = (float)(occ(p) >> 40) * (1.0f / 16777216.0f) < keep[node];
            }
            const uint64_t m = ballot(k);
            if (k) {
                const uint32_t j = nk + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                kpos[j] = p;
                knode[j] = node;
            }
            nk += (uint32_t)__popcll(m);
        }
        wave_lds_fence();
        uint32_t n_pairs = 0;
        double loss = 0.0;
        unsigned long long n_evals = 0;
        float parked = 0.0f;                                           // lane e: x of the batch's evaluation e
        uint32_t n_parked = 0;                                         // (uniform) evaluations parked, < 64 between groups
        // the terms of the parked evaluations, added in evaluation order; softplus(x) = max(x, 0) + log1p(exp(-|x|))
#define SGNS_EVAL_FLUSH()                                                                              \
        do {                                                                                           \
            const double x = (double)parked;                                                           \
            const double term = fmax(x, 0.0) + log1p(exp(-fabs(x)));                                   \
            for (uint32_t e = 0; e < n_parked; e++) loss += readlane_f64(term, (int)e);                \
            n_evals += n_parked;                                                                       \
            n_parked = 0;                                                                              \
        } while (0)
        for (uint32_t j = 0; j < nk; j++) {
            const uint32_t pos = readfirst_u32(kpos[j]), centre = readfirst_u32(knode[j]);
            uint64_t rs = sgns_mix(occ(pos));
            const uint32_t eff = a.window - (uint32_t)(rs % a.window);                          // shrunk window, 1 .. window
            const uint32_t lo = j - min(eff, j), hi = j + min(eff, nk - 1 - j);
            for (uint32_t i = lo; i <= hi; i++) {
                if (i == j) continue;
                const uint32_t c = readfirst_u32(kpos[i]), ctx = readfirst_u32(knode[i]);
                rs = sgns_mix(rs + c);
                const float *v = syn0 + (uint64_t)ctx * a.dim;
                float vin[PER];
#pragma unroll
                for (int s = 0; s < PER; s++) {
                    const uint32_t k = (uint32_t)s * WAVE + lane;
                    vin[s] = (s < PER - 1 || tail) ? v[k] : 0.0f;
                }
                for (uint32_t g0 = 0; g0 <= a.negative; g0 += SGNS_GROUP) {
                    if (n_parked + SGNS_GROUP > WAVE) SGNS_EVAL_FLUSH();
                    uint32_t tgt[SGNS_GROUP];
                    uint32_t act = 0;                                  // bit t: target t is scored
#pragma unroll
                    for (int t = 0; t < SGNS_GROUP; t++) {
                        const uint32_t ng = g0 + (uint32_t)t;
                        const bool draw = ng != 0 && ng <= a.negative;
                        const uint64_t next = sgns_mix(rs + ng);
                        rs = draw ? next : rs;
                        const uint32_t drawn = table[(uint32_t)(rs >> 16) % a.table_size];
                        tgt[t] = draw ? drawn : centre;
                        act |= (uint32_t)(ng <= a.negative && !(draw && drawn == centre)) << t;
                    }
                    float uu[SGNS_GROUP][PER];
#pragma unroll
                    for (int t = 0; t < SGNS_GROUP; t++) {
                        const float *u = syn1 + (uint64_t)tgt[t] * a.dim;
#pragma unroll
                        for (int s = 0; s < PER; s++) {
                            const uint32_t k = (uint32_t)s * WAVE + lane;
                            uu[t][s] = (s < PER - 1 || tail) ? u[k] : 0.0f;
                        }
                    }
#pragma unroll
                    for (int t = 0; t < SGNS_GROUP; t++) {
                        float dot = 0.0f;
#pragma unroll
                        for (int s = 0; s < PER; s++) dot += vin[s] * uu[t][s];
                        dot = wave_sum(dot);
                        const bool on = act >> t & 1u;
                        const float x = g0 + (uint32_t)t == 0 ? -dot : dot;   // (the float64 of -dot is minus the float64 of dot)
                        parked = (on && (uint32_t)lane == n_parked) ? x : parked;
                        n_parked += on;
                    }
                }
                n_pairs++;
            }
        }
        SGNS_EVAL_FLUSH();
#undef SGNS_EVAL_FLUSH
#undef occ
        if (a.counters && lane == 0 && nk) {
            atomicAdd(&a.counters[0], (unsigned long long)nk);
            atomicAdd(&a.counters[1], (unsigned long long)n_pairs);
        }
        if (lane == 0) {                                               // (one writer per cell; a walk without survivors writes zeros)
            a.walk_loss[wk] = loss;
            a.walk_evals[wk] = n_evals;
        }
    }
}

// The epoch's loss from the per-walk values, in an order that depends on nothing but their count: block b owns the indices
// [b * chunk, (b + 1) * chunk), thread t of its 256 adds its indices t, t + 256, ... in ascending order, the 64 partial sums
// of a wavefront meet in the xor butterfly 32 -> 1 and the four wavefront sums are added in wavefront order.  The host calls
// it twice: chunk = SGNS_LOSS_CHUNK over the walks (a constant: the block ranges do not follow the device or the trainer's
// launch), then one block with chunk = the number of block sums.  No floating-point atomic takes part; the evaluation counts
// ride along (integers: any order gives the same sum).
constexpr uint32_t SGNS_LOSS_CHUNK = 4096;
__global__ void __launch_bounds__(256)
sgns_loss_reduce_kernel(const double *__restrict__ in_loss, const unsigned long long *__restrict__ in_evals, uint64_t n, uint64_t chunk,
                        double *__restrict__ out_loss, unsigned long long *__restrict__ out_evals) {
    __shared__ double s_loss[4];
    __shared__ unsigned long long s_evals[4];
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double loss = 0.0;
    unsigned long long evals = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) { loss += in_loss[i]; evals += in_evals[i]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        loss += __shfl_xor(loss, off, WAVE);
        evals += __shfl_xor(evals, off, WAVE);
    }
    if (threadIdx.x % WAVE == 0) { s_loss[threadIdx.x / WAVE] = loss; s_evals[threadIdx.x / WAVE] = evals; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out_loss[blockIdx.x] = ((s_loss[0] + s_loss[1]) + s_loss[2]) + s_loss[3];
        out_evals[blockIdx.x] = s_evals[0] + s_evals[1] + s_evals[2] + s_evals[3];
    }
}

// The lock bits of one matrix from a byte mask (non-zero = frozen): a wavefront takes 64 rows, one ballot, and its lane 0
// stores the two words; rows at and beyond n_rows vote 0, so the bits past the end of the last word are zero.  `words` holds
// 2 * ceil(n_rows / 64) cells.  n_set[0] += the rows frozen (one atomic per wavefront that has any).
__global__ void __launch_bounds__(256)
sgns_lock_pack_kernel(const uint8_t *__restrict__ mask, uint32_t n_rows, uint32_t *__restrict__ words, unsigned long long *n_set) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = ballot(r < n_rows && mask[r < n_rows ? r : 0] != 0);
    if (lane_id() == 0 && (r & ~63ull) < n_rows) {
        words[r >> 5] = (uint32_t)m;
        words[(r >> 5) + 1] = (uint32_t)(m >> 32);
        if (m) atomicAdd(n_set, (unsigned long long)__popcll(m));
    }
}
// ... and back: mask[r] = bit r, as 0 / 1
__global__ void __launch_bounds__(256)
sgns_lock_unpack_kernel(const uint32_t *__restrict__ words, uint32_t n_rows, uint8_t *__restrict__ mask) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows) mask[r] = (uint8_t)(words[r >> 5] >> (r & 31u) & 1u);
}

// word counts of a walk matrix (vocabulary statistics for the sampling table and the subsampling probabilities);
// bad[0] = first walk whose length cell exceeds L + 1 or that names a node >= n_nodes (atomicMin, ~0: none)
__global__ void __launch_bounds__(256)
sgns_count_kernel(const uint32_t *__restrict__ walks, uint64_t n_walks, uint32_t L, uint32_t n_nodes, unsigned long long *counts,
                  unsigned long long *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t wk = i / (L + 1);
    if (wk >= n_walks) return;
    const uint32_t pos = (uint32_t)(i - wk * (L + 1));
    const uint32_t *row = walks + wk * ((uint64_t)L + 2);
    const uint32_t len = row[L + 1];
    if (len > L + 1) { atomicMin(bad, (unsigned long long)wk); return; }
    if (pos < len) {
        if (row[pos] >= n_nodes) { atomicMin(bad, (unsigned long long)wk); return; }
        atomicAdd(&counts[row[pos]], 1ull);
    }
}

}  // namespace pw
