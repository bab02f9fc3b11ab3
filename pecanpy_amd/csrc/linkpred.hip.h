// linkpred.hip.h -- link prediction in device memory (gfx950): the score of given pairs of rows, the exact AUC of two sets of
// scores, non-edges of a CSR graph drawn from the seeded stream.  pw_knn_score_pairs_device, pw_auc_device,
// pw_sample_non_edges_device, pw_selftest_score_pairs / _auc / _sample_non_edges.
//
// THE DEFINITIONS (the whole contract; DESIGN.md 4.9 repeats them).
//
//   pair scores   A is float32[na, dim] and B float32[nb, dim] (B = A when no second index is given), both with their norms
//                 as knn.hip.h defines them.  score[i] = knn_score(knn_dot(A[u[i]], B[v[i]]), norm(A[u[i]]), norm(B[v[i]]), metric):
//                 float64 accumulation from +0.0, k ascending, one rounding per addition; cosine divides by the ONE product
//                 of the two norms and is +0.0 where that product is 0.  u[i] == v[i] and repeated pairs are pairs like any
//                 other; m = 0 is a valid call that does nothing.
//       invalid   u[i] >= na or v[i] >= nb: refused, naming the first such position (u before v at the same position),
//                 nothing written.  A and B of different dim or on different devices: refused.
//
//   AUC           pos is float64[m], neg float64[n], m, n >= 1, m * n < 2^62, n < 2^32 (the sort's positions are 32-bit).
//                 wins = #{(i, j): pos[i] > neg[j]}, ties = #{(i, j): pos[i] == neg[j]}, compared as IEEE compares:
//                 -0.0 == +0.0, the infinities are ordinary values.  auc_key maps a double that is no NaN to a uint64 with
//                 key(x) < key(y) <=> x < y and key(x) == key(y) <=> x == y (-0.0 is made +0.0 first), so with the
//                 negatives' keys sorted ascending  wins = sum_i lower_bound(key(pos[i])),
//                 ties = sum_i (upper_bound(key(pos[i])) - lower_bound(key(pos[i]))).
//                 AUC = (2 wins + ties) / (2 m n): the caller forms it from the two integers.
//       invalid   a NaN: refused, naming the first (pos is looked at before neg), nothing written.
//
//   non-edges     w = the tempered 32-bit words of RandomState(seed) (pw_mt_words); N = n_nodes.  Candidate c, counted from
//                 first_candidate, is  u = (uint64(w[2 c]) * N) >> 32,  v = (uint64(w[2 c + 1]) * N) >> 32.  It is ACCEPTED when
//                 u != v and v is not in row u of the CSR (rows ascending: a binary search).  The output is the first m
//                 accepted candidates in candidate order; candidates_used = (the index of the last candidate examined for
//                 them) + 1 - first_candidate, 0 for m = 0: a second call at first_candidate + candidates_used continues the
//                 same sequence.  Accepted pairs may repeat (the draws are independent).
//       cap       A = N (N - 1) - (nnz - loops) ordered pairs are acceptable, a share s = A / N^2 of the candidates.  A call
//                 examines at most  cap = 16 * ceil(m N^2 / A) + 64  candidates (lp_candidate_cap; saturated at 2^62): sixteen
//                 times the expected number m / s, plus a slack.  The count needed is a sum of m geometric waits: for m = 1
//                 it passes the cap with probability (1 - s)^cap <= e^-16 = 1.2e-7, and for larger m with less (the sum
//                 concentrates about its mean).  So the cap ends a call that the stream has starved -- on a near-complete
//                 graph that is the alternative to a hang -- and is nothing a user meets otherwise.  A call that would
//                 examine more is refused, naming the count, nothing written.
//       invalid   A == 0 (no off-diagonal non-edge: the complete graph, a graph of one vertex): refused.  Dense handles:
//                 PW_ERR_UNSUPPORTED.
// No result depends on the grid, the tiling, the batch size or which form ran.
//
// The definitions are written once -- knn_step / knn_score (knn.hip.h), auc_key, lp_candidate, lp_row_has, lp_accept,
// lp_candidate_cap -- for host and device; lp_host_* run them with plain loops (the selftests with on_device = 0), and that
// half of the file compiles with a plain C++ compiler as well.
//
// The device form:
//   lp_check_pairs_kernel  the lowest position with a row number out of range, by an integer atomic minimum
//   lp_score_pairs_kernel  the kernel is gather bound -- two rows of dim float32 per pair and a dependent chain of dim float64
//                          FMAs.  A WAVEFRONT takes 64 pairs and owns a piece of LDS; no workgroup barrier anywhere.  It stages
//                          both rows of each of its pairs 32 columns at a time: the 8 lanes of a group read the 128
//                          consecutive bytes of one row's chunk (16-byte loads), 8 rows per instruction.  Each lane then
//                          runs its own pair's chain from LDS with 16-byte reads; the 36-float row stride puts the lanes'
//                          reads on distinct banks (knn_score_kernel's layout).  The accumulator lives across the chunks;
//                          plain V_FMA_F64 only.  2 wavefronts x 36 KiB / 2 per workgroup: 8 wavefronts per CU.
//   auc_keys_kernel        keys of an array, the lowest position of a NaN
//   radix_hist_kernel / radix_scatter_kernel (coo_csr.hip.h)
//                          the negatives' keys sorted in eight 8-bit passes
//   auc_count_kernel       a lane takes positives in a grid stride: two binary searches each; the lanes' sums are added in the
//                          wavefront and leave by two 64-bit integer atomic adds
//   lp_loops_kernel        the number of self loops of the CSR (for A)
//   lp_flag_kernel         a batch of candidates from the batch's words (expanded by the handle's stream machinery:
//                          mt_words_kernel): flag[i] = accepted
//   exclusive scan (scan.hip.h) of the flags, the total read back once per batch
//   lp_compact_kernel      accepted candidate number p of the batch, p < the number still wanted, goes to out[written + p];
//                          the one with p = wanted - 1 leaves its index: where the final batch is cut
#pragma once
#include <stdint.h>

#include "knn.hip.h"

namespace pw {

// ---- the definitions -------------------------------------------------------------------------------------------------
// order-preserving key of a double that is no NaN; -0.0 and +0.0 share a key
PW_KNN_HD uint64_t auc_key(double x) {
    if (x == 0.0) x = 0.0;   // -0.0 -> +0.0
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

PW_KNN_HD bool auc_is_nan(double x) { return x != x; }

// first position in the ascending keys[0, n) whose key is >= k (upper = false) or > k (upper = true)
PW_KNN_HD uint64_t auc_bound(const uint64_t *keys, uint64_t n, uint64_t k, bool upper) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (upper ? keys[mid] <= k : keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

PW_KNN_HD uint32_t lp_candidate(uint32_t w, uint32_t n_nodes) { return (uint32_t)(((uint64_t)w * n_nodes) >> 32); }

// v is in the ascending row u of the CSR
PW_KNN_HD bool lp_row_has(const uint32_t *indptr, const uint32_t *indices, uint32_t u, uint32_t v) {
    uint32_t lo = indptr[u], hi = indptr[u + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t x = indices[mid];
        if (x == v) return true;
        if (x < v) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

PW_KNN_HD bool lp_accept(const uint32_t *indptr, const uint32_t *indices, uint32_t u, uint32_t v) {
    return u != v && !lp_row_has(indptr, indices, u, v);
}

constexpr uint64_t LP_CAP_MAX = 1ull << 62;

// acceptable ordered pairs of a CSR of n_nodes vertices and nnz entries, `loops` of them on the diagonal
PW_KNN_HD uint64_t lp_acceptable(uint64_t n_nodes, uint64_t nnz, uint64_t loops) { return n_nodes * (n_nodes - 1) - (nnz - loops); }

// cap = 16 * ceil(m N^2 / A) + 64, saturated (A >= 1)
PW_KNN_HD uint64_t lp_candidate_cap(uint64_t m, uint64_t n_nodes, uint64_t acceptable) {
    const unsigned __int128 num = (unsigned __int128)m * n_nodes * n_nodes;   // < 2^64 * 2^64: m < 2^64, N^2 < 2^64
    const unsigned __int128 need = (num + acceptable - 1) / acceptable;
    if (need >= (LP_CAP_MAX >> 5)) return LP_CAP_MAX;
    return 16 * (uint64_t)need + 64;
}

// ---- the host forms: plain loops over the definitions --------------------------------------------------------------
enum LpHostResult { LP_HOST_OK = 0, LP_HOST_U_RANGE = 1, LP_HOST_V_RANGE = 2, LP_HOST_POS_NAN = 3, LP_HOST_NEG_NAN = 4, LP_HOST_CAP = 5 };

// the first position whose row number is out of range, before anything is written
inline int lp_host_check_pairs(const uint32_t *u, const uint32_t *v, uint64_t m, uint64_t na, uint64_t nb, uint64_t *where) {
    for (uint64_t i = 0; i < m; i++) {
        if (u[i] >= na) { *where = i; return LP_HOST_U_RANGE; }
        if (v[i] >= nb) { *where = i; return LP_HOST_V_RANGE; }
    }
    return LP_HOST_OK;
}

inline int lp_host_score_pairs(const float *A, const double *anorms, uint64_t na, const float *B, const double *bnorms, uint64_t nb, uint32_t dim,
                               const uint32_t *u, const uint32_t *v, uint64_t m, int metric, double *score, uint64_t *where) {
    if (int rc = lp_host_check_pairs(u, v, m, na, nb, where)) return rc;
    for (uint64_t i = 0; i < m; i++)
        score[i] = knn_score(knn_dot(A + (uint64_t)u[i] * dim, B + (uint64_t)v[i] * dim, dim), anorms[u[i]], bnorms[v[i]], metric);
    return LP_HOST_OK;
}

// keys[i] = auc_key(x[i]); 1 with *where = the first NaN
inline int auc_host_keys(const double *x, uint64_t n, uint64_t *keys, uint64_t *where) {
    for (uint64_t i = 0; i < n; i++) {
        if (auc_is_nan(x[i])) { *where = i; return 1; }
        keys[i] = auc_key(x[i]);
    }
    return 0;
}

// sorted_neg: the negatives' keys ascending
inline void auc_host_count(const double *pos, uint64_t m, const uint64_t *sorted_neg, uint64_t n, uint64_t out[2]) {
    uint64_t wins = 0, ties = 0;
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t k = auc_key(pos[i]);
        const uint64_t lb = auc_bound(sorted_neg, n, k, false), ub = auc_bound(sorted_neg, n, k, true);
        wins += lb;
        ties += ub - lb;
    }
    out[0] = wins;
    out[1] = ties;
}

inline uint64_t lp_host_loops(const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes) {
    uint64_t loops = 0;
    for (uint32_t r = 0; r < n_nodes; r++) loops += lp_row_has(indptr, indices, r, r) ? 1 : 0;
    return loops;
}

// words[2 c], words[2 c + 1]: the words of candidate first_candidate + c, for c < cap (the caller expands them as they are
// needed: `more(c)` makes candidate c available and returns the pointer to its two words).  u / v: room for m, filled as the
// candidates are accepted -- scratch of the caller's, copied out on LP_HOST_OK; *used is written on LP_HOST_OK only.
template <class Words>
inline int lp_host_sample(const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, uint64_t m, uint64_t cap, Words &&more, uint32_t *u,
                          uint32_t *v, uint64_t *used) {
    uint64_t got = 0, c = 0;
    for (; got < m; c++) {
        if (c >= cap) return LP_HOST_CAP;
        const uint32_t *w = more(c);
        const uint32_t cu = lp_candidate(w[0], n_nodes), cv = lp_candidate(w[1], n_nodes);
        if (lp_accept(indptr, indices, cu, cv)) { u[got] = cu; v[got] = cv; got++; }
    }
    *used = c;
    return LP_HOST_OK;
}

}  // namespace pw

// ---- the device form -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "wave.h"

namespace pw {

constexpr uint32_t LP_WAVES = 2;                 // wavefronts of a pair-score workgroup, each with its own 64 pairs
constexpr uint32_t LP_THREADS = LP_WAVES * WAVE;
constexpr uint32_t LP_KC = KNN_KC;               // columns staged per chunk
constexpr uint32_t LP_STRIDE = KNN_STRIDE;       // floats per staged row (36: the lanes' 16-byte reads fall on distinct banks)

struct LpFound {   // what the check passes report, by integer atomics
    unsigned long long first;   // lowest offending position; ~0: none
};

__global__ __launch_bounds__(256) void lp_check_pairs_kernel(const uint32_t *__restrict__ u, const uint32_t *__restrict__ v, uint64_t m, uint64_t na,
                                                             uint64_t nb, LpFound *found) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x)
        if (u[i] >= na || v[i] >= nb) atomicMin(&found->first, (unsigned long long)i);
}

struct LpScoreArgs {
    const float *A, *B;              // [na, dim], [nb, dim]
    const double *anorms, *bnorms;
    const uint32_t *u, *v;           // [m], checked
    double *score;                   // [m]
    uint64_t m, n_tiles;             // pairs; tiles of 64 pairs
    uint32_t dim, metric;
};

__global__ __launch_bounds__(LP_THREADS) void lp_score_pairs_kernel(const LpScoreArgs a) {
    __shared__ __attribute__((aligned(16))) float rows_lds[LP_WAVES][2 * WAVE * LP_STRIDE];
    __shared__ uint32_t idx_lds[LP_WAVES][2 * WAVE];
    const uint32_t w = readfirst_u32(threadIdx.x >> 6), lane = (uint32_t)lane_id();
    float *tile = rows_lds[w];
    uint32_t *idx = idx_lds[w];
    const bool vec4 = (a.dim & 3u) == 0;   // (A and B are the indexes' own allocations: 16-byte aligned)
    const float *my_u = tile + (size_t)lane * LP_STRIDE, *my_v = tile + (size_t)(WAVE + lane) * LP_STRIDE;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LP_WAVES + w, n_waves = (uint64_t)gridDim.x * LP_WAVES;

    for (uint64_t t = wave0; t < a.n_tiles; t += n_waves) {   // (wavefront-uniform)
        const uint64_t i = t * WAVE + lane;
        const bool valid = i < a.m;
        const uint32_t ru = valid ? a.u[i] : 0u, rv = valid ? a.v[i] : 0u;   // (row 0 exists: n >= 1)
        wave_lds_fence();   // the tile before has been read
        idx[lane] = ru;
        idx[WAVE + lane] = rv;
        double acc = 0.0;
        for (uint32_t k0 = 0; k0 < a.dim; k0 += LP_KC) {
            const uint32_t kcur = min(LP_KC, a.dim - k0), kc4 = (kcur + 3) >> 2;
            wave_lds_fence();   // the chunk before has been read; the row numbers are in place
            for (uint32_t e = lane; e < 2 * WAVE * kc4; e += WAVE) {
                const uint32_t r = e / kc4, c = (e - r * kc4) << 2;
                const uint32_t col = k0 + c;
                const float *src = (r < WAVE ? a.A : a.B) + (uint64_t)idx[r] * a.dim + col;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (vec4) {
                    x = *(const float4 *)src;
                } else {
                    x.x = src[0];
                    if (col + 1 < a.dim) x.y = src[1];
                    if (col + 2 < a.dim) x.z = src[2];
                    if (col + 3 < a.dim) x.w = src[3];
                }
                *(float4 *)(tile + (size_t)r * LP_STRIDE + c) = x;
            }
            wave_lds_fence();
            for (uint32_t kk = 0; kk < kc4; kk++) {   // (the padded columns add exact zeros)
                const float4 x = *(const float4 *)(my_u + (kk << 2)), y = *(const float4 *)(my_v + (kk << 2));
                acc = knn_step(acc, x.x, y.x);
                acc = knn_step(acc, x.y, y.y);
                acc = knn_step(acc, x.z, y.z);
                acc = knn_step(acc, x.w, y.w);
            }
        }
        if (valid) a.score[i] = knn_score(acc, a.anorms[ru], a.bnorms[rv], (int)a.metric);
    }
}

// keys[i] = auc_key(x[i]); the lowest position of a NaN
__global__ __launch_bounds__(256) void auc_keys_kernel(const double *__restrict__ x, uint64_t n, uint64_t *__restrict__ keys, LpFound *found) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double d = x[i];
        if (auc_is_nan(d)) atomicMin(&found->first, (unsigned long long)i);
        keys[i] = auc_key(d);
    }
}

// counts[0] += wins, counts[1] += ties of this launch's positives against the negatives' sorted keys
__global__ __launch_bounds__(256) void auc_count_kernel(const uint64_t *__restrict__ pos_keys, uint64_t m, const uint64_t *__restrict__ neg_sorted,
                                                        uint64_t n, unsigned long long *__restrict__ counts) {
    uint64_t wins = 0, ties = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = pos_keys[i];
        const uint64_t lb = auc_bound(neg_sorted, n, k, false), ub = auc_bound(neg_sorted, n, k, true);
        wins += lb;
        ties += ub - lb;
    }
    wins = wave_incl_scan_u64(wins);   // (every lane is here: the loop above has no early exit)
    ties = wave_incl_scan_u64(ties);
    if (lane_id() == WAVE - 1) {
        if (wins) atomicAdd(&counts[0], (unsigned long long)wins);
        if (ties) atomicAdd(&counts[1], (unsigned long long)ties);
    }
}

__global__ __launch_bounds__(256) void lp_loops_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint32_t n_nodes,
                                                       unsigned long long *__restrict__ loops) {
    uint32_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_nodes; r += (uint64_t)gridDim.x * blockDim.x)
        mine += lp_row_has(indptr, indices, (uint32_t)r, (uint32_t)r) ? 1u : 0u;
    const uint32_t wave_loops = wave_sum_u32(mine);
    if (lane_id() == 0 && wave_loops) atomicAdd(loops, (unsigned long long)wave_loops);
}

// words: the two words of the batch's candidate i at words[2 i], words[2 i + 1].  flag[i] = accepted, flag[n] = 0 (the scan
// runs over n + 1 cells, so that every accepted candidate sees pos[i + 1] = pos[i] + 1)
__global__ __launch_bounds__(256) void lp_flag_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint32_t n_nodes,
                                                      const uint32_t *__restrict__ words, uint64_t n, uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t f = 0;
        if (i < n) {
            const uint32_t u = lp_candidate(words[2 * i], n_nodes), v = lp_candidate(words[2 * i + 1], n_nodes);
            f = lp_accept(indptr, indices, u, v) ? 1u : 0u;
        }
        flag[i] = f;
    }
}

// pos: the exclusive scan of the flags (n + 1 cells).  The accepted candidates numbered p < want go to out_u / out_v[p]
// (the caller passes the pointers advanced by what earlier batches wrote); number want - 1 leaves its index in *last.
__global__ __launch_bounds__(256) void lp_compact_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ pos, uint64_t n,
                                                         uint32_t n_nodes, uint64_t want, uint32_t *__restrict__ out_u, uint32_t *__restrict__ out_v,
                                                         unsigned long long *__restrict__ last) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = pos[i];
        if (pos[i + 1] == p || p >= want) continue;
        out_u[p] = lp_candidate(words[2 * i], n_nodes);
        out_v[p] = lp_candidate(words[2 * i + 1], n_nodes);
        if (p + 1 == want) *last = (unsigned long long)i;
    }
}

}  // namespace pw
#endif
