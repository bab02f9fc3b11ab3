// holdout.hip.h -- edges of a CSR graph held out by the seeded stream, in device memory (gfx950): the train graph as a CSR and
// the held-out pairs.  pw_holdout_edges_device, pw_holdout_dev_shape / _fill / _destroy, pw_selftest_holdout_edges.
//
// THE DEFINITION (the whole contract; DESIGN.md 4.10 repeats it).
//
//   inputs      a CSR as the handles hold it -- indptr uint32[N + 1], rows ascending and duplicate-free, data float32 or none --
//               directed (0 / 1), seed, first_word (an offset into the stream), threshold (uint32), protect (0 / 1).
//   stream      w = the tempered 32-bit words of RandomState(seed) (pw_mt_words).  The Python layer makes
//               threshold = int(Fraction(fraction) * 2^32) for 0 <= fraction < 1: integer arithmetic, no float multiply.
//   units       directed = 1: every entry e = (r -> c) with r != c is a unit.  directed = 0: the CSR must be structurally
//               symmetric -- every entry r -> c, r != c, has a mate c -> r; the first entry position without one is refused,
//               naming it, nothing written -- and a unit is an entry with r < c (the UPPER entry); its mate belongs to it and
//               shares its fate.  Self loops are never units and always stay.
//   protected   (protect = 1)  f(r) = the position of the first non-loop entry of row r: indptr[r], or indptr[r] + 1 when
//               indices[indptr[r]] == r; none when the row ends there (ho_first).  A directed unit at e in row r is protected
//               when e == f(r); an undirected unit (r < c) at e with mate m when e == f(r) or m == f(c).  So every row that
//               had a non-loop entry keeps one, and an undirected train graph stays symmetric.
//   decision    the unit at position e is HELD OUT iff  w[first_word + e] < threshold  and it is not protected (ho_decide).
//               The position is the upper entry's for undirected graphs; words at other positions are simply not used: no
//               rank, no scan enters the rule.
//   outputs     the train CSR: all entries not held out, in order, data carried over, new indptr, rows still ascending.
//               The held-out list in ascending unit position: u[k], v[k] (u < v when undirected, (r, c) when directed),
//               weight[k] = the float32 of the unit's own entry, 1.0 when the graph has no data.
//               words_used = nnz: a later call at first_word + nnz draws an independent split.
//   must hold   threshold = 0 returns the graph's arrays bit for bit and an empty list.  No result depends on the grid, the
//               batch of words expanded at a time or which form ran.  A refused call leaves nothing allocated or written.
//
// The definition is written once -- ho_row_of, ho_find, ho_first, ho_decide -- for host and device; ho_host_split runs it with
// plain loops (pw_selftest_holdout_edges with on_device = 0, tools/holdout_selfcheck.cpp), and that half of the file compiles
// with a plain C++ compiler as well.
//
// The device form.  One byte per entry, flags[e] = HO_KEEP | HO_HELD bits, zeroed first; every byte has ONE writer:
//   ho_flag_kernel     a batch of entry positions with the batch's words (expanded by the handle's stream machinery:
//                      mt_words_kernel).  A LANE PER ENTRY, never per row (an RMAT hub has a row of 10^5 entries): the lane
//                      bisects indptr for its row -- the lanes of a wavefront hold consecutive entries, so all but the last
//                      few levels of the search are one address for the wavefront -- and, undirected, bisects the other row
//                      for its mate: the scattered, dependent part (lp_flag_kernel's pattern).  The upper entry writes its
//                      own byte and its mate's, a loop or a directed entry its own, a lower entry nothing.  The lowest
//                      position without a mate leaves by an integer atomicMin; units and protected units are summed in the
//                      wavefront and leave by two integer atomic adds.
//   exclusive scan (scan.hip.h) of the keep bits over nnz + 1 cells: pos[e]; pos[nnz] = the train graph's entries
//   ho_compact_kernel  kept entry e goes to position pos[e] of the train indices / data
//   ho_indptr_kernel   train indptr[r] = pos[indptr[r]], r = 0 .. N
//   exclusive scan of the held bits into the same pos; ho_held_kernel: held unit e, row bisected once more, to u / v / weight[pos[e]]
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PW_HO_HD __host__ __device__ __forceinline__
#else
#define PW_HO_HD inline
#endif

namespace pw {

// ---- the definition ----------------------------------------------------------------------------------------------------
constexpr uint32_t HO_NONE = 0xffffffffu;
// what ho_decide says of an entry; the flag byte of the device form keeps HO_KEEP and HO_HELD
constexpr uint32_t HO_KEEP = 1, HO_HELD = 2, HO_UNIT = 4, HO_PROT = 8, HO_LOWER = 16, HO_MISSING = 32;

// the row of entry position e < indptr[n_nodes]: indptr[r] <= e < indptr[r + 1]
PW_HO_HD uint32_t ho_row_of(const uint32_t *indptr, uint32_t n_nodes, uint32_t e) {
    uint32_t lo = 0, hi = n_nodes;   // indptr[lo] <= e < indptr[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (indptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the position of c in the ascending row r, HO_NONE when it is not there
PW_HO_HD uint32_t ho_find(const uint32_t *indptr, const uint32_t *indices, uint32_t r, uint32_t c) {
    uint32_t lo = indptr[r], hi = indptr[r + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t x = indices[mid];
        if (x == c) return mid;
        if (x < c) lo = mid + 1;
        else hi = mid;
    }
    return HO_NONE;
}

// f(r): the position of the first non-loop entry of row r, HO_NONE when the row has none
PW_HO_HD uint32_t ho_first(const uint32_t *indptr, const uint32_t *indices, uint32_t r) {
    uint32_t s = indptr[r];
    const uint32_t end = indptr[r + 1];
    if (s < end && indices[s] == r) s++;
    return s < end ? s : HO_NONE;
}

// Entry e of row r, w = w[first_word + e].  HO_KEEP alone: a self loop.  HO_MISSING: undirected and no mate.  HO_LOWER:
// undirected and r > c, the fate is the upper entry's.  Else a unit: HO_UNIT | HO_PROT? | (HO_HELD or HO_KEEP), *mate = the
// mate's position (undirected).
PW_HO_HD uint32_t ho_decide(const uint32_t *indptr, const uint32_t *indices, int directed, int protect, uint32_t threshold, uint32_t e, uint32_t r,
                            uint32_t w, uint32_t *mate) {
    const uint32_t c = indices[e];
    *mate = HO_NONE;
    if (c == r) return HO_KEEP;
    bool prot;
    if (directed) {
        prot = protect && e == ho_first(indptr, indices, r);
    } else {
        const uint32_t m = ho_find(indptr, indices, c, r);
        if (m == HO_NONE) return HO_MISSING;
        if (r > c) return HO_LOWER;
        *mate = m;
        prot = protect && (e == ho_first(indptr, indices, r) || m == ho_first(indptr, indices, c));
    }
    const bool held = w < threshold && !prot;
    return HO_UNIT | (prot ? HO_PROT : 0u) | (held ? HO_HELD : HO_KEEP);
}

// ---- the host form: plain loops over the definition ------------------------------------------------------------------
enum HoHostResult { HO_HOST_OK = 0, HO_HOST_MISSING = 1 };

// word(e) = w[first_word + e].  Outputs: out_indptr[n_nodes + 1]; out_indices / out_data / u / v / weight with room for nnz
// (out_data may be NULL; data NULL: every weight 1.0).  counts = {train entries, held units, units, protected units}.
// HO_HOST_MISSING: *where = the first entry position without a mate, nothing written.
template <class Word>
inline int ho_host_split(const uint32_t *indptr, const uint32_t *indices, const float *data, uint32_t n_nodes, int directed, int protect,
                         uint32_t threshold, Word &&word, uint32_t *out_indptr, uint32_t *out_indices, float *out_data, uint32_t *u, uint32_t *v,
                         float *weight, uint64_t counts[4], uint64_t *where) {
    const uint32_t nnz = indptr[n_nodes];
    std::vector<uint8_t> flags(nnz, 0);
    uint64_t units = 0, prot = 0;
    for (uint32_t r = 0; r < n_nodes; r++)
        for (uint32_t e = indptr[r]; e < indptr[r + 1]; e++) {
            uint32_t mate;
            const uint32_t d = ho_decide(indptr, indices, directed, protect, threshold, e, r, word(e), &mate);
            if (d & HO_MISSING) { *where = e; return HO_HOST_MISSING; }
            if (d & HO_LOWER) continue;
            flags[e] = (uint8_t)(d & (HO_KEEP | HO_HELD));
            if (mate != HO_NONE) flags[mate] = (uint8_t)(d & HO_KEEP);
            units += (d & HO_UNIT) ? 1 : 0;
            prot += (d & HO_PROT) ? 1 : 0;
        }
    uint64_t kept = 0, held = 0;
    for (uint32_t r = 0; r < n_nodes; r++) {
        out_indptr[r] = (uint32_t)kept;
        for (uint32_t e = indptr[r]; e < indptr[r + 1]; e++) {
            if (flags[e] & HO_KEEP) {
                out_indices[kept] = indices[e];
                if (out_data) out_data[kept] = data ? data[e] : 1.0f;
                kept++;
            }
            if (flags[e] & HO_HELD) {
                u[held] = r;
                v[held] = indices[e];
                weight[held] = data ? data[e] : 1.0f;
                held++;
            }
        }
    }
    out_indptr[n_nodes] = (uint32_t)kept;
    counts[0] = kept; counts[1] = held; counts[2] = units; counts[3] = prot;
    return HO_HOST_OK;
}

}  // namespace pw

// ---- the device form -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "wave.h"

namespace pw {

struct HoCells {                 // what the flag passes report, by integer atomics
    unsigned long long missing;  // lowest entry position without a mate; ~0: none
    unsigned long long units, prot;
};

// entries [e0, e0 + n) of the CSR, words[i] = w[first_word + e0 + i]
__global__ __launch_bounds__(256) void ho_flag_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint32_t n_nodes,
                                                      int directed, int protect, uint32_t threshold, const uint32_t *__restrict__ words, uint32_t e0,
                                                      uint32_t n, uint8_t *__restrict__ flags, HoCells *cells) {
    uint32_t units = 0, prot = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {   // (workgroup-uniform)
        const uint64_t i = base + threadIdx.x;
        if (i >= n) continue;
        const uint32_t e = e0 + (uint32_t)i;
        uint32_t mate;
        const uint32_t d = ho_decide(indptr, indices, directed, protect, threshold, e, ho_row_of(indptr, n_nodes, e), words[i], &mate);
        if (d & HO_MISSING) { atomicMin(&cells->missing, (unsigned long long)e); continue; }
        if (d & HO_LOWER) continue;
        flags[e] = (uint8_t)(d & (HO_KEEP | HO_HELD));
        if (mate != HO_NONE) flags[mate] = (uint8_t)(d & HO_KEEP);
        units += (d & HO_UNIT) ? 1u : 0u;
        prot += (d & HO_PROT) ? 1u : 0u;
    }
    const uint32_t wave_units = wave_sum_u32(units), wave_prot = wave_sum_u32(prot);   // (every lane is here: no early exit above)
    if (lane_id() == 0) {
        if (wave_units) atomicAdd(&cells->units, (unsigned long long)wave_units);
        if (wave_prot) atomicAdd(&cells->prot, (unsigned long long)wave_prot);
    }
}

// the counts of the two scans: bit `bit` of the flag bytes over nnz + 1 cells (the last one 0)
struct HoBitCount {
    const uint8_t *flags;
    uint64_t nnz;
    uint32_t bit;
    __device__ uint32_t operator()(uint64_t i) const { return i < nnz && (flags[i] & bit) ? 1u : 0u; }
};

// pos: the exclusive scan of the keep bits (nnz + 1 cells)
__global__ __launch_bounds__(256) void ho_compact_kernel(const uint32_t *__restrict__ indices, const float *__restrict__ data,
                                                         const uint8_t *__restrict__ flags, const uint32_t *__restrict__ pos, uint32_t nnz,
                                                         uint32_t *__restrict__ out_indices, float *__restrict__ out_data) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * blockDim.x) {
        if (!(flags[e] & HO_KEEP)) continue;
        const uint32_t p = pos[e];
        out_indices[p] = indices[e];
        if (data) out_data[p] = data[e];
    }
}

__global__ __launch_bounds__(256) void ho_indptr_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ pos, uint32_t n_nodes,
                                                        uint32_t *__restrict__ out_indptr) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_nodes; r += (uint64_t)gridDim.x * blockDim.x) out_indptr[r] = pos[indptr[r]];
}

// pos: the exclusive scan of the held bits
__global__ __launch_bounds__(256) void ho_held_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                      const float *__restrict__ data, uint32_t n_nodes, const uint8_t *__restrict__ flags,
                                                      const uint32_t *__restrict__ pos, uint32_t nnz, uint32_t *__restrict__ u, uint32_t *__restrict__ v,
                                                      float *__restrict__ weight) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * blockDim.x) {
        if (!(flags[e] & HO_HELD)) continue;
        const uint32_t p = pos[e];
        u[p] = ho_row_of(indptr, n_nodes, (uint32_t)e);
        v[p] = indices[e];
        weight[p] = data ? data[e] : 1.0f;
    }
}

}  // namespace pw
#endif
