// knn.hip.h -- exact, ordered nearest neighbours of embedding vectors (gfx950): pw_knn_create_device, pw_knn_query_device,
// pw_selftest_knn.
//
// THE DEFINITION (the whole contract; DESIGN.md repeats it).  X is float32[n, dim], the database; Q is float32[nq, dim],
// the queries, given as vectors or as row numbers of X.
//   dot      dot(a, b) = (((0.0 + a[0] b[0]) + a[1] b[1]) + ...), k ascending, in float64 on the float32 values widened.
//            A product of two float32 values is exact in float64 (48 significand bits, no overflow, no underflow), so the
//            only roundings are the dim additions, in that fixed order -- and fma(a, b, acc) and acc + a * b give the same
//            bits: the device uses the first (one V_FMA_F64), the host build the second (knn_step).  The accumulator
//            starts at +0.0, so no score is ever -0.0.
//   norm     norm(x) = sqrt(dot(x, x)), the correctly rounded float64 square root.
//   score    metric dot: dot(q, x).  metric cosine: dot(q, x) / (norm(q) * norm(x)), one multiplication, then one
//            division; a product norm(q) * norm(x) of 0 gives +0.0 (the zero-vector rule, no further special case).
//   invalid  a NaN or an infinity anywhere in X or Q is refused, naming the first such row: finite float32 input cannot
//            overflow float64 here, so "dot(x, x) is not finite" is the whole test, and the norm pass finds it for free.
//   order    candidates rank by descending score, equal scores by ascending row number: a total order, so the top topn
//            are unique.
//   self     with exclude_self and a query given as a row number, that one row is no candidate (another row with the
//            same contents still is); with a query given as a vector nothing is excluded.
//   output   idx uint32[nq, topn], score float64[nq, topn]; slots beyond the number of candidates hold 0xFFFFFFFF / -inf.
//   limits   1 <= topn <= 128 (PW_KNN_MAX_TOPN), 1 <= dim <= 4096, n < 2^32; nq = 0 is a valid call that does nothing.
// The answer does not depend on tiling, on the grid, on the number of wavefronts or on which form ran.
//
// The definition is written once -- knn_step, knn_dot, knn_norm, knn_score, knn_before, knn_insert -- for host and device;
// knn_host_query runs it with plain loops (pw_selftest_knn with on_device = 0), and that half of the file compiles with
// a plain C++ compiler as well.
//
// The device form:
//   knn_norms_kernel    a lane owns a row: its sequential float64 sum, the norm; rows whose sum is not finite are counted
//                       and the lowest kept, by integer atomics (there is no floating-point atomic in this file)
//   knn_query_norms_kernel / knn_stage_queries_kernel
//                       the same for the queries (a query by row number is checked against n and takes the row's
//                       norm); then a batch of queries widened to float64 in the layout the score kernel reads with
//                       scalar loads: [slot][k][8], a slot being the up to 8 queries of one wavefront
//   knn_score_kernel    512 threads = 8 wavefronts = RG row groups x 8 / RG query groups.  The workgroup stages 64 RG
//                       rows of X into LDS, 32 columns at a time (16-byte loads; 36-float row stride: the lanes' 16-byte
//                       reads of their own rows fall on distinct banks).  A lane owns one row and keeps a float64
//                       accumulator for each of its wavefront's 8 queries in registers; the query values are
//                       wavefront-uniform and arrive by scalar loads, an operand of the FMA itself.  k ascends across
//                       the chunks and the accumulators live across them.  Plain vector V_FMA_F64 only: the f64 MFMA
//                       sums in an internal order that is part of no contract, so it has no place here.
//                       A workgroup is persistent: it walks the query tiles of its tile part and, per tile, the row
//                       blocks of its row part, so a query has row_parts x RG partial lists, not n / block.
//                       Per (wavefront, query) a sorted list of the best topn (score, row) pairs lives in LDS, born as
//                       (-inf, 0xFFFFFFFF).  A wavefront compares its lanes' scores with the list's last entry, the
//                       wavefront-uniform threshold, and inserts the few that beat it, one at a time, all lanes
//                       shifting (knn_wave_insert: knn_insert spread over the lanes).  After warm-up insertions are rare.
//   knn_merge_kernel    a wavefront per query streams the query's partial lists through the same insertion.  The order
//                       is total, so the result is the top topn of the union whatever order the lists arrive in.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PW_KNN_HD __host__ __device__ __forceinline__
#else
#define PW_KNN_HD inline
#endif

namespace pw {

constexpr uint32_t KNN_MAX_TOPN = 128;   // PW_KNN_MAX_TOPN
constexpr uint32_t KNN_MAX_DIM = 4096;
constexpr uint32_t KNN_NONE = 0xFFFFFFFFu;
constexpr int KNN_DOT = 0, KNN_COSINE = 1;   // PW_KNN_DOT, PW_KNN_COSINE

// ---- the definition --------------------------------------------------------------------------------------------------
PW_KNN_HD double knn_step(double acc, float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fma((double)a, (double)b, acc);   // the product is exact: the same bits as below
#else
    return acc + (double)a * (double)b;
#endif
}

PW_KNN_HD double knn_dot(const float *a, const float *b, uint32_t dim) {
    double acc = 0.0;
    for (uint32_t k = 0; k < dim; k++) acc = knn_step(acc, a[k], b[k]);
    return acc;
}

PW_KNN_HD bool knn_finite(double x) { return __builtin_isfinite(x); }

PW_KNN_HD double knn_norm(double dot_xx) { return sqrt(dot_xx); }

PW_KNN_HD double knn_score(double dot, double norm_q, double norm_x, int metric) {
    if (metric == KNN_DOT) return dot;
    const double den = norm_q * norm_x;
    return den == 0.0 ? 0.0 : dot / den;
}

// (s1, r1) ranks before (s2, r2)
PW_KNN_HD bool knn_before(double s1, uint32_t r1, double s2, uint32_t r2) { return s1 > s2 || (s1 == s2 && r1 < r2); }

PW_KNN_HD double knn_neg_inf() { return -__builtin_huge_val(); }

// the sorted list sc / ix of topn entries takes (s, r) if it ranks before the last entry
PW_KNN_HD void knn_insert(double *sc, uint32_t *ix, uint32_t topn, double s, uint32_t r) {
    if (!knn_before(s, r, sc[topn - 1], ix[topn - 1])) return;
    uint32_t p = topn - 1;
    while (p > 0 && knn_before(s, r, sc[p - 1], ix[p - 1])) {
        sc[p] = sc[p - 1];
        ix[p] = ix[p - 1];
        p--;
    }
    sc[p] = s;
    ix[p] = r;
}

// ---- the host form: plain loops over the definition ----------------------------------------------------------------
enum KnnHostResult { KNN_HOST_OK = 0, KNN_HOST_BAD_ROW = 1, KNN_HOST_BAD_QUERY = 2, KNN_HOST_ROW_RANGE = 3 };

// norms[n] of X; KNN_HOST_BAD_ROW with *where = the first row that holds a NaN or an infinity
inline int knn_host_norms(const float *X, uint64_t n, uint32_t dim, double *norms, uint64_t *where) {
    for (uint64_t i = 0; i < n; i++) {
        const double d = knn_dot(X + i * dim, X + i * dim, dim);
        if (!knn_finite(d)) { *where = i; return KNN_HOST_BAD_ROW; }
        norms[i] = knn_norm(d);
    }
    return KNN_HOST_OK;
}

// Exactly one of Q and rows is given.  Everything is checked before anything is written; on a refusal *where is the
// row of X (BAD_ROW) or the position among the queries (BAD_QUERY, ROW_RANGE).  norms / qnorms: scratch of n / nq doubles.
inline int knn_host_query(const float *X, uint64_t n, uint32_t dim, const float *Q, const uint32_t *rows, uint64_t nq, uint32_t topn,
                          int metric, int exclude_self, uint32_t *idx, double *score, double *norms, double *qnorms, uint64_t *where) {
    if (int rc = knn_host_norms(X, n, dim, norms, where)) return rc;
    for (uint64_t q = 0; q < nq; q++) {
        if (rows) {
            if (rows[q] >= n) { *where = q; return KNN_HOST_ROW_RANGE; }
            qnorms[q] = norms[rows[q]];
        } else {
            const double d = knn_dot(Q + q * dim, Q + q * dim, dim);
            if (!knn_finite(d)) { *where = q; return KNN_HOST_BAD_QUERY; }
            qnorms[q] = knn_norm(d);
        }
    }
    for (uint64_t q = 0; q < nq; q++) {
        const float *qv = rows ? X + (uint64_t)rows[q] * dim : Q + q * dim;
        const uint32_t self = rows && exclude_self ? rows[q] : KNN_NONE;
        double *sc = score + q * topn;
        uint32_t *ix = idx + q * topn;
        for (uint32_t e = 0; e < topn; e++) { sc[e] = knn_neg_inf(); ix[e] = KNN_NONE; }
        for (uint64_t i = 0; i < n; i++) {
            if ((uint32_t)i == self) continue;
            knn_insert(sc, ix, topn, knn_score(knn_dot(qv, X + i * dim, dim), qnorms[q], norms[i], metric), (uint32_t)i);
        }
    }
    return KNN_HOST_OK;
}

}  // namespace pw

// ---- the device form -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "wave.h"

namespace pw {

constexpr uint32_t KNN_QT = 8;             // queries a wavefront keeps accumulators for
constexpr uint32_t KNN_WAVES = 8;          // wavefronts of a score workgroup: row groups x query groups
constexpr uint32_t KNN_THREADS = KNN_WAVES * WAVE;
constexpr uint32_t KNN_KC = 32;            // columns staged per chunk, at most
constexpr uint32_t KNN_STRIDE = KNN_KC + 4;   // floats per staged row: lane r's 16-byte read at 36 r dwords, banks 4 (9 r mod 16) ..

struct KnnFound {   // what the norm passes report, by integer atomics
    unsigned long long first_bad;   // lowest row (position) whose sum is not finite; ~0: none
    unsigned long long first_range; // lowest position of a row number >= n; ~0: none
};

__device__ __forceinline__ double knn_dot_global(const float *a, const float *b, uint32_t dim) {
    double acc = 0.0;
    uint32_t k = 0;
    if (((dim & 3u) == 0) && ((((uintptr_t)a | (uintptr_t)b) & 15u) == 0)) {
        for (; k < dim; k += 4) {
            const float4 x = *(const float4 *)(a + k), y = *(const float4 *)(b + k);
            acc = knn_step(acc, x.x, y.x);
            acc = knn_step(acc, x.y, y.y);
            acc = knn_step(acc, x.z, y.z);
            acc = knn_step(acc, x.w, y.w);
        }
        return acc;
    }
    for (; k < dim; k++) acc = knn_step(acc, a[k], b[k]);
    return acc;
}

// norms[i] = norm(X[i]); rows with a NaN or an infinity: the lowest in found->first_bad
__global__ __launch_bounds__(256) void knn_norms_kernel(const float *__restrict__ X, uint64_t n, uint32_t dim, double *__restrict__ norms,
                                                        KnnFound *found) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double d = knn_dot_global(X + i * dim, X + i * dim, dim);
        if (!knn_finite(d)) atomicMin(&found->first_bad, (unsigned long long)i);
        norms[i] = knn_norm(d);
    }
}

// qnorms[q] of every query of the call: a row number is checked against n and takes the row's norm, a vector its own
__global__ __launch_bounds__(256) void knn_query_norms_kernel(const float *__restrict__ Q, const uint32_t *__restrict__ rows, uint64_t nq,
                                                              uint64_t n, uint32_t dim, const double *__restrict__ xnorms,
                                                              double *__restrict__ qnorms, KnnFound *found) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * blockDim.x) {
        if (rows) {
            const uint32_t r = rows[q];
            if (r >= n) atomicMin(&found->first_range, (unsigned long long)q);
            qnorms[q] = r < n ? xnorms[r] : 0.0;
        } else {
            const double d = knn_dot_global(Q + q * dim, Q + q * dim, dim);
            if (!knn_finite(d)) atomicMin(&found->first_bad, (unsigned long long)q);
            qnorms[q] = knn_norm(d);
        }
    }
}

// qd[slot][k][8], k < dimp (dim rounded up to 4): the queries q0 + slot qt + j, j < qt, of a batch of nqb, widened; every
// other cell +0.0 (a wavefront's unused accumulators and the padded columns add exact zeros).  One thread per (slot, j).
__global__ __launch_bounds__(256) void knn_stage_queries_kernel(const float *__restrict__ X, const float *__restrict__ Q,
                                                                const uint32_t *__restrict__ rows, uint64_t q0, uint32_t nqb, uint32_t qt,
                                                                uint32_t n_slots, uint32_t dim, uint32_t dimp, double *__restrict__ qd) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n_slots * KNN_QT) return;
    const uint32_t slot = (uint32_t)(t / KNN_QT), j = (uint32_t)(t % KNN_QT);
    const uint64_t q = (uint64_t)slot * qt + j;
    const float *src = nullptr;
    if (j < qt && q < nqb) src = rows ? X + (uint64_t)rows[q0 + q] * dim : Q + (q0 + q) * dim;
    double *dst = qd + (uint64_t)slot * dimp * KNN_QT + j;
    for (uint32_t k = 0; k < dimp; k++) dst[(uint64_t)k * KNN_QT] = (src && k < dim) ? (double)src[k] : 0.0;
}

// knn_insert spread over the 64 lanes: the wavefront's sorted list sc / ix (LDS, topn <= 128: two entries per lane) takes
// the lanes' candidates (s, r) that rank before its last entry, lowest lane first; every lane shifts its entries.
// Called by the whole wavefront in uniform control flow.
__device__ __forceinline__ void knn_wave_insert(double *sc, uint32_t *ix, uint32_t topn, double s, uint32_t r, bool valid) {
    const uint32_t lane = (uint32_t)lane_id();
    bool want = valid && knn_before(s, r, sc[topn - 1], ix[topn - 1]);
    uint64_t m = ballot(want);
    while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        const double cs = readlane_f64(s, src);
        const uint32_t cr = readlane_u32(r, src);
        const uint32_t e0 = lane, e1 = lane + WAVE;
        double a0 = 0.0, a1 = 0.0;
        uint32_t i0 = 0, i1 = 0;
        bool b0 = false, b1 = false;
        if (e0 < topn) { a0 = sc[e0]; i0 = ix[e0]; b0 = knn_before(a0, i0, cs, cr); }
        if (e1 < topn) { a1 = sc[e1]; i1 = ix[e1]; b1 = knn_before(a1, i1, cs, cr); }
        const uint32_t p = (uint32_t)__popcll(ballot(b0)) + (uint32_t)__popcll(ballot(b1));   // < topn: the candidate beats the last entry
        wave_lds_fence();
        if (e0 >= p && e0 + 1 < topn) { sc[e0 + 1] = a0; ix[e0 + 1] = i0; }
        if (e1 >= p && e1 + 1 < topn) { sc[e1 + 1] = a1; ix[e1 + 1] = i1; }
        if (lane == 0) { sc[p] = cs; ix[p] = cr; }
        wave_lds_fence();
        want = want && (int)lane != src && knn_before(s, r, sc[topn - 1], ix[topn - 1]);
        m = ballot(want);
    }
}

struct KnnScoreArgs {
    const float *X;          // [n, dim]
    const double *xnorms;    // [n]
    const double *qd;        // [n_tiles * qg][dimp][8]
    const double *qnorms;    // [nqb]: the batch's
    const uint32_t *qself;   // [nqb]: the row a query excludes, or nullptr
    double *part_sc;         // [row_parts * rg][nqb][topn]
    uint32_t *part_ix;
    uint64_t n, n_blocks;    // rows; row blocks of 64 rg rows
    uint32_t dim, dimp, nqb, qt, topn, metric;
    uint32_t rg, kc;         // row groups (1, 2, 4); columns per chunk (a multiple of 4, <= 32)
    uint32_t row_parts, tile_parts, n_tiles;
};

inline size_t knn_score_lds_bytes(uint32_t rg, uint32_t topn) {
    return (size_t)WAVE * rg * KNN_STRIDE * sizeof(float) + (size_t)KNN_WAVES * KNN_QT * topn * (sizeof(double) + sizeof(uint32_t));
}

__global__ __launch_bounds__(KNN_THREADS) void knn_score_kernel(const KnnScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    const uint32_t R = WAVE * a.rg, qg_n = KNN_WAVES / a.rg;
    float *tile = (float *)knn_lds;
    double *lsc_all = (double *)(knn_lds + (size_t)R * KNN_STRIDE * sizeof(float));
    uint32_t *lix_all = (uint32_t *)(lsc_all + (size_t)KNN_WAVES * KNN_QT * a.topn);

    const uint32_t w = readfirst_u32(threadIdx.x >> 6), lane = (uint32_t)lane_id();
    const uint32_t rgi = w % a.rg, qgi = w / a.rg;
    double *lsc = lsc_all + (size_t)w * KNN_QT * a.topn;
    uint32_t *lix = lix_all + (size_t)w * KNN_QT * a.topn;
    const uint32_t row_part = blockIdx.x % a.row_parts, tile_part = blockIdx.x / a.row_parts;
    const bool vec4 = (a.dim & 3u) == 0;   // (X is the index's own allocation: 16-byte aligned)
    const float *my_row = tile + (size_t)(rgi * WAVE + lane) * KNN_STRIDE;

    for (uint32_t t = tile_part; t < a.n_tiles; t += a.tile_parts) {
        const uint32_t slot = t * qg_n + qgi;
        const uint64_t qbase = (uint64_t)slot * a.qt;
        const uint32_t n_valid = qbase < a.nqb ? (uint32_t)min((uint64_t)a.qt, a.nqb - qbase) : 0u;   // wavefront-uniform
        for (uint32_t e = lane; e < KNN_QT * a.topn; e += WAVE) { lsc[e] = knn_neg_inf(); lix[e] = KNN_NONE; }
        sptr<double> qv = as_scalar<double>((uint64_t)(a.qd + (uint64_t)slot * a.dimp * KNN_QT));

        for (uint64_t b = row_part; b < a.n_blocks; b += a.row_parts) {
            const uint64_t row0 = b * R;
            double acc[KNN_QT];
#pragma unroll
            for (uint32_t j = 0; j < KNN_QT; j++) acc[j] = 0.0;

            for (uint32_t k0 = 0; k0 < a.dim; k0 += a.kc) {
                const uint32_t kcur = min(a.kc, a.dim - k0), kc4 = (kcur + 3) >> 2;
                __syncthreads();   // the chunk before has been read
                for (uint32_t i = threadIdx.x; i < R * kc4; i += KNN_THREADS) {
                    const uint32_t r = i / kc4, c = (i - r * kc4) << 2;
                    const uint64_t row = row0 + r;
                    const uint32_t col = k0 + c;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (row < a.n) {
                        const float *src = a.X + row * a.dim + col;
                        if (vec4) {
                            v = *(const float4 *)src;
                        } else {
                            v.x = src[0];
                            if (col + 1 < a.dim) v.y = src[1];
                            if (col + 2 < a.dim) v.z = src[2];
                            if (col + 3 < a.dim) v.w = src[3];
                        }
                    }
                    *(float4 *)(tile + (size_t)r * KNN_STRIDE + c) = v;
                }
                __syncthreads();
                if (n_valid) {
                    sptr<double> qk = qv + (uint64_t)k0 * KNN_QT;
                    for (uint32_t kk = 0; kk < kc4; kk++) {
                        const float4 x = *(const float4 *)(my_row + (kk << 2));
                        const double xd[4] = {(double)x.x, (double)x.y, (double)x.z, (double)x.w};
#pragma unroll
                        for (uint32_t i = 0; i < 4; i++) {
#pragma unroll
                            for (uint32_t j = 0; j < KNN_QT; j++) acc[j] = __builtin_fma(qk[(kk * 4 + i) * KNN_QT + j], xd[i], acc[j]);
                        }
                    }
                }
            }

            const uint64_t row = row0 + rgi * WAVE + lane;
            const double xn = row < a.n ? a.xnorms[row] : 0.0;
#pragma unroll
            for (uint32_t j = 0; j < KNN_QT; j++) {
                if (j < n_valid) {
                    const double s = knn_score(acc[j], a.qnorms[qbase + j], xn, (int)a.metric);
                    const uint32_t self = a.qself ? a.qself[qbase + j] : KNN_NONE;
                    knn_wave_insert(lsc + (size_t)j * a.topn, lix + (size_t)j * a.topn, a.topn, s, (uint32_t)row, row < a.n && (uint32_t)row != self);
                }
            }
        }

        wave_lds_fence();
        const uint64_t list = (uint64_t)row_part * a.rg + rgi;
        for (uint32_t j = 0; j < n_valid; j++) {
            const uint64_t out = (list * a.nqb + qbase + j) * a.topn;
            for (uint32_t e = lane; e < a.topn; e += WAVE) {
                a.part_sc[out + e] = lsc[(size_t)j * a.topn + e];
                a.part_ix[out + e] = lix[(size_t)j * a.topn + e];
            }
        }
        wave_lds_fence();   // (the lists are born again at the top of the next tile)
    }
}

// a wavefront per query: the query's n_lists partial lists through the same insertion -> idx / score rows q0 + q
__global__ __launch_bounds__(256) void knn_merge_kernel(const double *__restrict__ part_sc, const uint32_t *__restrict__ part_ix, uint32_t n_lists,
                                                        uint32_t nqb, uint32_t topn, uint32_t *__restrict__ idx, double *__restrict__ score) {
    __shared__ double msc[4][KNN_MAX_TOPN];
    __shared__ uint32_t mix[4][KNN_MAX_TOPN];
    const uint32_t w = readfirst_u32(threadIdx.x >> 6), lane = (uint32_t)lane_id();
    const uint64_t q = (uint64_t)blockIdx.x * 4 + w;
    if (q >= nqb) return;   // (wavefront-uniform; no block barrier below)
    double *sc = msc[w];
    uint32_t *ix = mix[w];
    for (uint32_t e = lane; e < topn; e += WAVE) { sc[e] = knn_neg_inf(); ix[e] = KNN_NONE; }
    wave_lds_fence();
    for (uint32_t l = 0; l < n_lists; l++) {
        const uint64_t in = ((uint64_t)l * nqb + q) * topn;
        for (uint32_t e0 = 0; e0 < topn; e0 += WAVE) {
            const uint32_t e = e0 + lane;
            double s = knn_neg_inf();
            uint32_t r = KNN_NONE;
            if (e < topn) { s = part_sc[in + e]; r = part_ix[in + e]; }
            knn_wave_insert(sc, ix, topn, s, r, r != KNN_NONE);
        }
    }
    wave_lds_fence();
    for (uint32_t e = lane; e < topn; e += WAVE) {
        idx[q * topn + e] = ix[e];
        score[q * topn + e] = sc[e];
    }
}

}  // namespace pw
#endif
