// nbr_scores.hip.h -- the neighbourhood heuristics of link prediction in device memory (gfx950): common neighbours, Jaccard's
// coefficient, preferential attachment and a table-weighted sum over the common neighbours (Adamic-Adar, resource allocation),
// scored directly on given pairs of rows of a CSR graph.  pw_nbr_degrees_device, pw_nbr_scores_device, pw_selftest_nbr_scores,
// pw_selftest_nbr_degrees.
//
// THE DEFINITION (the whole contract; DESIGN.md 4.11 repeats it).  For a CSR of N vertices whose rows are ascending and
// duplicate-free (pw_csr_create's invariant):
//
//   N(x)   the entries of row x other than x itself: a self loop is no neighbour.  Stored weights are not looked at, an entry of
//          weight 0 is an entry; a directed graph's N(x) is its out-row.
//   d(x)   |N(x)|
//   C(u,v) N(u) n N(v), which therefore contains neither u nor v;  cn = |C|.
//
//   score[i], float64, of the pair (u[i], v[i]) by `kind`:
//     NBR_COMMON     double(cn)
//     NBR_JACCARD    double(cn) / double(d(u) + d(v) - cn): one IEEE division; +0.0 when the denominator is 0
//     NBR_PREF       double(uint64(d(u)) * uint64(d(v))): the product exact in 64-bit integers, one rounding in the conversion
//     NBR_WEIGHTED   t is the caller's float64[N] table: (((+0.0 + t[z0]) + t[z1]) + ...) over z in C ASCENDING, one rounding per
//                    addition.  A NaN or an infinity in t is an ordinary value.  Adamic-Adar and resource allocation are this kind
//                    with a table the caller builds (the Python layer: t[z] = 1 / ln d(z) and 1 / d(z), 0.0 for d(z) < 2, the
//                    function evaluated on the host on the distinct degrees): the table is an input, no device log is part of any
//                    result.
//   u[i] == v[i], repeated pairs and pairs that are edges are pairs like any other; m = 0 is a valid call that does nothing.
//       invalid   u[i] >= N or v[i] >= N: refused, naming the first such position (u before v at the same position), nothing
//                 written.  An unknown kind, NBR_WEIGHTED without a table: refused.  Dense handles: PW_ERR_UNSUPPORTED.
// No result depends on the grid, the tile, the cut between the two forms below (short_max), the cut between search and merge,
// or which row of a pair was scanned: C is symmetric in u and v and its elements are met in ascending order from either row.
//
// The definition is written once -- nbr_degree, nbr_lower_bound, nbr_hit, nbr_score -- for host and device; nbr_host_* run it
// with plain loops (the selftests with on_device = 0), and that half of the file compiles with a plain C++ compiler as well.
//
// The device form:
//   lp_check_pairs_kernel (linkpred.hip.h)   the lowest position with a row number out of range
//   nbr_degrees_kernel     d(x) for every row: indptr and one look for the loop
//   nbr_scores_kernel      the work of a pair is its shorter row searched in its longer one: 0 .. 10^5 elements on a skewed graph,
//                          and hub-hub pairs are common among degree-biased positives.  One kernel, no binning pass.  A
//                          WAVEFRONT takes a tile of 64 pairs.  (1) Each lane settles its own pair when the shorter row has at
//                          most short_max elements: it walks the shorter row and searches each element in the longer one, in a
//                          window whose lower end only moves forward (both rows ascend); when the lengths are close
//                          (longer < NBR_MERGE_RATIO * shorter) it merges the two rows instead.  (2) The pairs left over are
//                          found by a ballot and the whole wavefront takes them one at a time: the lanes take 64 consecutive
//                          elements of the shorter row, each searches its own in the window of the longer row that the chunk
//                          before left, the hits are a ballot and cn grows by its popcount.  For NBR_WEIGHTED the hit lanes'
//                          t[z] are added to the ONE accumulator in lane order -- ascending z -- by a loop over the set bits
//                          with readlane_f64: the sequential order of the definition, not a tree.  The other kinds skip that
//                          loop; NBR_PREF skips the intersection.  No LDS, no workgroup barrier, no floating-point atomic.
#pragma once
#include <stdint.h>

#include "linkpred.hip.h"

namespace pw {

// ---- the definition ----------------------------------------------------------------------------------------------------
enum NbrKind { NBR_COMMON = 0, NBR_JACCARD = 1, NBR_PREF = 2, NBR_WEIGHTED = 3, NBR_KINDS = 4 };

constexpr uint32_t NBR_SHORT_MAX = 8;       // a lane settles its own pair up to this many elements in the shorter row: the best of
                                            // the sweep 0 .. all-lane of tools/nbr_bench.py (MEASUREMENTS.md, "Neighbourhood baselines")
constexpr uint32_t NBR_ALL_LANE = 0xFFFFFFFFu;   // short_max: every pair stays with its lane
constexpr uint32_t NBR_MERGE_RATIO = 4;     // lane form: merge when longer < NBR_MERGE_RATIO * shorter, search otherwise

// d(x): the entries of row x without its self loop
PW_KNN_HD uint32_t nbr_degree(const uint32_t *indptr, const uint32_t *indices, uint32_t x) {
    return indptr[x + 1] - indptr[x] - (lp_row_has(indptr, indices, x, x) ? 1u : 0u);
}

// first position in [lo, hi) of the ascending `indices` whose entry is >= z (hi when there is none)
PW_KNN_HD uint32_t nbr_lower_bound(const uint32_t *indices, uint32_t lo, uint32_t hi, uint32_t z) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (indices[mid] < z) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the intersection step: z, an entry of one row of the pair (u, v), is looked for in [*lo, hi) of the other row; *lo moves to
// z's lower bound (entries after z in its row are larger: they are found from there on).  True when z is in C(u, v).
PW_KNN_HD bool nbr_hit(const uint32_t *indices, uint32_t *lo, uint32_t hi, uint32_t z, uint32_t u, uint32_t v) {
    *lo = nbr_lower_bound(indices, *lo, hi, z);
    return *lo < hi && indices[*lo] == z && z != u && z != v;
}

PW_KNN_HD double nbr_jaccard(uint32_t cn, uint32_t du, uint32_t dv) {
    const uint64_t den = (uint64_t)du + dv - cn;
    return den == 0 ? 0.0 : (double)cn / (double)den;
}

PW_KNN_HD double nbr_pref(uint32_t du, uint32_t dv) { return (double)((uint64_t)du * (uint64_t)dv); }

// the four formulas: cn and sum of C(u, v) (sum: NBR_WEIGHTED only), du / dv the degrees (NBR_JACCARD, NBR_PREF only)
PW_KNN_HD double nbr_score(int kind, uint32_t cn, double sum, uint32_t du, uint32_t dv) {
    return kind == NBR_COMMON ? (double)cn : kind == NBR_JACCARD ? nbr_jaccard(cn, du, dv) : kind == NBR_PREF ? nbr_pref(du, dv) : sum;
}

PW_KNN_HD bool nbr_needs_degrees(int kind) { return kind == NBR_JACCARD || kind == NBR_PREF; }

// ---- the host forms: plain loops over the definition ---------------------------------------------------------------------
inline void nbr_host_degrees(const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, uint32_t *deg) {
    for (uint32_t x = 0; x < n_nodes; x++) deg[x] = nbr_degree(indptr, indices, x);
}

// cn and (table != nullptr) the ascending sum of one pair: the shorter row walked, each entry searched in the longer one
inline uint32_t nbr_host_common(const uint32_t *indptr, const uint32_t *indices, uint32_t u, uint32_t v, const double *table, double *sum) {
    const bool u_short = indptr[u + 1] - indptr[u] <= indptr[v + 1] - indptr[v];
    const uint32_t a = u_short ? u : v, b = u_short ? v : u;
    uint32_t cn = 0, lo = indptr[b];
    double acc = 0.0;
    for (uint32_t p = indptr[a]; p < indptr[a + 1]; p++) {
        const uint32_t z = indices[p];
        if (!nbr_hit(indices, &lo, indptr[b + 1], z, u, v)) continue;
        cn++;
        if (table) acc = acc + table[z];
    }
    *sum = acc;
    return cn;
}

// LP_HOST_U_RANGE / LP_HOST_V_RANGE with *where before anything is written (kind and table are the caller's to check)
inline int nbr_host_scores(const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, const uint32_t *u, const uint32_t *v, uint64_t m,
                           int kind, const double *table, double *score, uint64_t *where) {
    if (int rc = lp_host_check_pairs(u, v, m, n_nodes, n_nodes, where)) return rc;
    for (uint64_t i = 0; i < m; i++) {
        uint32_t cn = 0, du = 0, dv = 0;
        double sum = 0.0;
        if (kind != NBR_PREF) cn = nbr_host_common(indptr, indices, u[i], v[i], kind == NBR_WEIGHTED ? table : nullptr, &sum);
        if (nbr_needs_degrees(kind)) { du = nbr_degree(indptr, indices, u[i]); dv = nbr_degree(indptr, indices, v[i]); }
        score[i] = nbr_score(kind, cn, sum, du, dv);
    }
    return LP_HOST_OK;
}

}  // namespace pw

// ---- the device form -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "wave.h"

namespace pw {

constexpr uint32_t NBR_WAVES = 4;                  // wavefronts of a workgroup, each with its own tiles of 64 pairs
constexpr uint32_t NBR_THREADS = NBR_WAVES * WAVE;

__global__ __launch_bounds__(256) void nbr_degrees_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint32_t n_nodes,
                                                          uint32_t *__restrict__ deg) {
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_nodes; x += (uint64_t)gridDim.x * blockDim.x)
        deg[x] = nbr_degree(indptr, indices, (uint32_t)x);
}

struct NbrArgs {
    const uint32_t *indptr, *indices;   // the CSR: [N + 1], [nnz]
    const double *table;                // [N]; NBR_WEIGHTED only
    const uint32_t *u, *v;              // [m], checked
    double *score;                      // [m]
    uint64_t m, n_tiles;                // pairs; tiles of 64 pairs
    uint32_t kind, short_max;
};

__global__ __launch_bounds__(NBR_THREADS) void nbr_scores_kernel(const NbrArgs a) {
    const uint32_t w = readfirst_u32(threadIdx.x >> 6), lane = (uint32_t)lane_id();
    const uint32_t *__restrict__ indptr = a.indptr, *__restrict__ indices = a.indices;
    const bool weighted = a.kind == NBR_WEIGHTED, intersect = a.kind != NBR_PREF;   // (wavefront-uniform)
    const uint64_t wave0 = (uint64_t)blockIdx.x * NBR_WAVES + w, n_waves = (uint64_t)gridDim.x * NBR_WAVES;

    for (uint64_t t = wave0; t < a.n_tiles; t += n_waves) {   // (wavefront-uniform)
        const uint64_t i = t * WAVE + lane;
        const bool valid = i < a.m;
        const uint32_t ru = valid ? a.u[i] : 0u, rv = valid ? a.v[i] : 0u;   // (row 0 exists: m >= 1 passed the range check)
        const uint32_t su = indptr[ru], eu = indptr[ru + 1], sv = indptr[rv], ev = indptr[rv + 1];
        const bool u_short = eu - su <= ev - sv;
        const uint32_t s0 = u_short ? su : sv, e0 = u_short ? eu : ev;   // the shorter row: walked
        const uint32_t l0 = u_short ? sv : su, l1 = u_short ? ev : eu;   // the longer row: searched
        const uint32_t n_short = e0 - s0, n_long = l1 - l0;
        uint32_t cn = 0;
        double sum = 0.0;

        // (1) the lane form
        const bool mine = valid && intersect && n_short <= a.short_max;
        if (mine && n_short) {
            if (n_long < (uint64_t)NBR_MERGE_RATIO * n_short) {   // close lengths: a merge
                uint32_t p = s0, q = l0;
                uint32_t x = indices[p], y = indices[q];
                for (;;) {
                    if (x == y) {
                        if (x != ru && x != rv) {
                            cn++;
                            if (weighted) sum = sum + a.table[x];
                        }
                        if (++p == e0 || ++q == l1) break;
                        x = indices[p];
                        y = indices[q];
                    } else if (x < y) {
                        if (++p == e0) break;
                        x = indices[p];
                    } else {
                        if (++q == l1) break;
                        y = indices[q];
                    }
                }
            } else {
                uint32_t lo = l0;
                for (uint32_t p = s0; p < e0 && lo < l1; p++) {
                    const uint32_t z = indices[p];
                    if (nbr_hit(indices, &lo, l1, z, ru, rv)) {
                        cn++;
                        if (weighted) sum = sum + a.table[z];
                    }
                }
            }
        }

        // (2) the wavefront form: the pairs left over, one at a time
        uint64_t todo = ballot(valid && intersect && !mine);
        while (todo) {   // (wavefront-uniform)
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t ws0 = readlane_u32(s0, l), we0 = readlane_u32(e0, l), wl1 = readlane_u32(l1, l);
            const uint32_t wu = readlane_u32(ru, l), wv = readlane_u32(rv, l);
            uint32_t wlo = readlane_u32(l0, l), wcn = 0;
            double wsum = 0.0;
            for (uint32_t c0 = ws0; c0 < we0 && wlo < wl1; c0 += WAVE) {   // (wavefront-uniform)
                const uint32_t left = we0 - c0, n_here = left < (uint32_t)WAVE ? left : (uint32_t)WAVE;
                const bool have = lane < n_here;
                const uint32_t z = have ? indices[c0 + lane] : 0xFFFFFFFFu;
                uint32_t pos = wlo;
                const bool hit = have && nbr_hit(indices, &pos, wl1, z, wu, wv);
                uint64_t hits = ballot(hit);
                wcn += (uint32_t)__builtin_popcountll(hits);
                if (weighted) {
                    const double tz = hit ? a.table[z] : 0.0;
                    while (hits) {   // lane order = ascending z: the sequential sum of the definition
                        const int b = __builtin_ctzll(hits);
                        hits &= hits - 1;
                        wsum = wsum + readlane_f64(tz, b);
                    }
                }
                wlo = readlane_u32(pos, (int)n_here - 1);   // the lower bound of the chunk's last element: where the next chunk starts
            }
            if (lane == (uint32_t)l) {
                cn = wcn;
                sum = wsum;
            }
        }

        if (valid) {
            uint32_t du = 0, dv = 0;
            if (nbr_needs_degrees((int)a.kind)) {
                du = eu - su - (lp_row_has(indptr, indices, ru, ru) ? 1u : 0u);
                dv = ev - sv - (lp_row_has(indptr, indices, rv, rv) ? 1u : 0u);
            }
            a.score[i] = nbr_score((int)a.kind, cn, sum, du, dv);
        }
    }
}

}  // namespace pw
#endif
