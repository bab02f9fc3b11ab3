// coo_csr.hip.h -- CSR from an edge list (COO) in device memory (gfx950): pw_coo_to_csr_device.
//
// Semantics = the reference's AdjlstGraph.add_edge / to_csr (graph.py:238-268, 323-341) with implicit integer ids:
// kept edge i inserts (src, dst) and, unless directed, (dst, src); for every ordered pair the LAST insertion's weight
// wins; rows ascending and duplicate-free.
//
// One code path for any m and any row length:
//   1. coo_validate_kernel   ids in range, weights finite, keep[i] = weight > 0, dropped count, largest id
//   2. scan of keep[]        rank of every kept edge = its place in insertion order (this scan and those below: scan.hip.h)
//   3. coo_expand_kernel     insertion j -> key (src << bits | dst), bits = ceil(log2 n_nodes), in insertion order
//   4. LSD radix sort        ceil(2 bits / 8) passes of 8 bits: per-wavefront histogram, scan, STABLE scatter -- equal
//                            keys stay in insertion order, so the last of a run of equal keys is the last insertion
//   5. coo_mark / scan / coo_compact   keep-last-of-run, output position, indices / data / row of every kept entry
//   6. coo_indptr_kernel     indptr[r] = lower bound of r among the (ascending) rows
// The edge-list reader (edgelist_dev.hip.h) takes the same path with float64 weights: coo_expand_lines_kernel, the sort carrying
// the line index, coo_conflict_kernel (a pair inserted again with another float64 weight), coo_compact_lines_kernel (which
// also leaves the winner's float64 weight beside its float32 rounding when the caller keeps them for the dense build).
// Determinism: every output word is a function of the input alone.  Atomics are used for integer counts, a minimum and a
// maximum only (order-independent results); the scatter ranks equal digits by lane order (ballots), never by arrival.
//
// Work split of the sort: a WAVEFRONT owns RADIX_SUB consecutive elements and its own 256 counters in LDS, so neither the
// histogram nor the scatter needs a workgroup barrier; the counters go to hist[digit * n_waves + wave], whose exclusive
// scan is each (digit, wave)'s first output position.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave.h"

namespace pw {

constexpr int RADIX_BITS = 8;
constexpr int RADIX_BINS = 1 << RADIX_BITS;
constexpr int RADIX_SUB = 2048;                   // elements per wavefront (32 rounds of 64)

// ---- edge list -> keys --------------------------------------------------------------------------------------------------
// flags: [0] first edge with an id outside [0, limit)   [1] first edge with a NaN / infinite weight
//        [2] edges dropped (weight <= 0)                [3] largest id + 1 over the edges with valid ids
__global__ void __launch_bounds__(256)
coo_validate_kernel(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const float *__restrict__ weight, uint64_t m,
                    uint64_t limit, uint32_t *__restrict__ keep, unsigned long long *__restrict__ flags) {
    uint32_t dropped = 0;
    unsigned long long top = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const int64_t s = src[i], d = dst[i];
        if (s < 0 || d < 0 || (uint64_t)s >= limit || (uint64_t)d >= limit) atomicMin(&flags[0], (unsigned long long)i);
        else {
            const unsigned long long hi = (unsigned long long)(s > d ? s : d) + 1;
            if (hi > top) top = hi;
        }
        if (weight) {
            const float w = weight[i];
            if (!isfinite(w)) atomicMin(&flags[1], (unsigned long long)i);
            const bool kept = w > 0.0f;
            keep[i] = kept ? 1u : 0u;
            dropped += kept ? 0u : 1u;
        }
    }
    const uint32_t wave_dropped = wave_sum_u32(dropped);
    if (lane_id() == 0 && wave_dropped) atomicAdd(&flags[2], (unsigned long long)wave_dropped);
    if (top) atomicMax(&flags[3], top);
}

// rank: exclusive scan of keep[] (NULL: every edge kept, rank = i).  Undirected: insertions 2 rank (forward), 2 rank + 1 (reverse).
__global__ void __launch_bounds__(256)
coo_expand_kernel(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const float *__restrict__ weight, uint64_t m,
                  const uint32_t *__restrict__ rank, int directed, int bits, uint64_t n_ins, uint64_t *__restrict__ keys,
                  float *__restrict__ wout) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const float w = weight ? weight[i] : 1.0f;
        if (!(w > 0.0f)) continue;
        const uint64_t r = rank ? (uint64_t)rank[i] : i;
        const uint64_t s = (uint64_t)src[i], d = (uint64_t)dst[i];
        const uint64_t j = directed ? r : 2 * r;
        if (j + (directed ? 0 : 1) >= n_ins) continue;   // (cannot happen: the ranks count the kept edges)
        keys[j] = (s << bits) | d;
        if (weight) wout[j] = w;
        if (!directed) {
            keys[j + 1] = (d << bits) | s;
            if (weight) wout[j + 1] = w;
        }
    }
}

// The edge-list reader's form (edgelist_dev.hip.h): every edge kept, and what travels with insertion j is the index of its
// LINE -- the float64 weights as parsed stay where they are, so that coo_conflict_kernel can compare them after the sort.
__global__ void __launch_bounds__(256)
coo_expand_lines_kernel(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, uint64_t m, int directed, int bits, uint64_t n_ins,
                        uint64_t *__restrict__ keys, uint32_t *__restrict__ line) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint64_t s = (uint64_t)src[i], d = (uint64_t)dst[i];
        const uint64_t j = directed ? i : 2 * i;
        if (j + (directed ? 0 : 1) >= n_ins) continue;   // (cannot happen: n_ins = m or 2 m)
        keys[j] = (s << bits) | d;
        line[j] = (uint32_t)i;
        if (!directed) {
            keys[j + 1] = (d << bits) | s;
            line[j + 1] = (uint32_t)i;
        }
    }
}

// ---- stable LSD radix pass ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
radix_hist_kernel(const uint64_t *__restrict__ keys, uint64_t n, int shift, uint32_t *__restrict__ hist, uint64_t n_waves) {
    __shared__ uint32_t cnt[4][RADIX_BINS];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + wave;
    if (w >= n_waves) return;
    for (int d = lane; d < RADIX_BINS; d += WAVE) cnt[wave][d] = 0;
    wave_lds_fence();
    const uint64_t first = w * RADIX_SUB;
    for (int r = 0; r < RADIX_SUB / WAVE; r++) {
        const uint64_t idx = first + (uint64_t)r * WAVE + lane;
        if (idx < n) atomicAdd(&cnt[wave][(uint32_t)(keys[idx] >> shift) & (RADIX_BINS - 1)], 1u);   // (a count: order-independent)
    }
    wave_lds_fence();
    for (int d = lane; d < RADIX_BINS; d += WAVE) hist[(uint64_t)d * n_waves + w] = cnt[wave][d];
}

// WEIGHTS: every key carries four bytes with it -- its float32 weight's bits, or (the edge-list reader) its line's index
template <bool WEIGHTS>
__global__ void __launch_bounds__(256)
radix_scatter_kernel(const uint64_t *__restrict__ kin, const uint32_t *__restrict__ win, uint64_t *__restrict__ kout,
                     uint32_t *__restrict__ wout, uint64_t n, int shift, const uint32_t *__restrict__ hist, uint64_t n_waves) {
    __shared__ uint32_t base[4][RADIX_BINS];   // next output position of every digit of this wavefront's elements
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + wave;
    if (w >= n_waves) return;
    for (int d = lane; d < RADIX_BINS; d += WAVE) base[wave][d] = hist[(uint64_t)d * n_waves + w];
    wave_lds_fence();
    const uint64_t first = w * RADIX_SUB;
    const uint64_t below = (1ull << lane) - 1;
    for (int r = 0; r < RADIX_SUB / WAVE; r++) {
        const uint64_t idx = first + (uint64_t)r * WAVE + lane;
        const bool valid = idx < n;
        const uint64_t key = valid ? kin[idx] : 0;
        const uint32_t digit = (uint32_t)(key >> shift) & (RADIX_BINS - 1);
        uint64_t same = ballot(valid);   // the valid lanes that hold this lane's digit
        for (int b = 0; b < RADIX_BITS; b++) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t has = ballot(valid && bit);
            same &= bit ? has : ~has;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below), count = (uint32_t)__popcll(same);
        const uint32_t off = valid ? base[wave][digit] : 0u;
        wave_lds_fence();   // every lane has read its digit's position before the digit's last lane moves it
        if (valid) {
            const uint64_t pos = (uint64_t)off + rank;
            if (pos < n) {   // (always: the positions come from the histogram of the same keys)
                kout[pos] = key;
                if (WEIGHTS) wout[pos] = win[idx];
            }
            if (rank + 1 == count) base[wave][digit] = off + count;
        }
        wave_lds_fence();
    }
}

// ---- keep the last of every run of equal keys, compact, row offsets --------------------------------------------------------
__global__ void __launch_bounds__(256)
coo_mark_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ flag) {   // flag[n] = 0: the scan's total
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) flag[j] = (j + 1 == n || keys[j] != keys[j + 1]) ? 1u : 0u;
    else if (j == n) flag[j] = 0u;
}

__global__ void __launch_bounds__(256)
coo_compact_kernel(const uint64_t *__restrict__ keys, const float *__restrict__ w, uint64_t n, const uint32_t *__restrict__ pos, int bits,
                   uint64_t nnz, uint32_t *__restrict__ indices, float *__restrict__ data, uint32_t *__restrict__ rows) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint64_t key = keys[j];
    if (j + 1 != n && key == keys[j + 1]) return;
    const uint64_t p = pos[j];
    if (p >= nnz) return;   // (cannot happen: nnz is the scan's total)
    indices[p] = (uint32_t)(key & ((1ull << bits) - 1));
    rows[p] = (uint32_t)(key >> bits);
    if (data) data[p] = w[j];
}

// ... the edge-list reader's forms.  An ordered pair inserted again with another float64 weight makes the reference warn: all
// weights of a run of equal keys are equal exactly when every two neighbours in it are (the weights are > 0: no NaN).
__global__ void __launch_bounds__(256)
coo_conflict_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ line, const double *__restrict__ w64, uint64_t n, uint64_t m,
                    uint32_t *__restrict__ conflict) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j + 1 >= n || keys[j] != keys[j + 1]) return;
    const uint32_t a = line[j], b = line[j + 1];
    if (a >= m || b >= m) return;   // (cannot happen: the payloads are line indices)
    if (w64[a] != w64[b]) atomicOr(conflict, 1u);
}

__global__ void __launch_bounds__(256)
coo_compact_lines_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ line, const double *__restrict__ w64, uint64_t n,
                         uint64_t m, const uint32_t *__restrict__ pos, int bits, uint64_t nnz, uint32_t *__restrict__ indices,
                         float *__restrict__ data, double *__restrict__ data64, uint32_t *__restrict__ rows) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint64_t key = keys[j];
    if (j + 1 != n && key == keys[j + 1]) return;
    const uint64_t p = pos[j];
    if (p >= nnz) return;   // (cannot happen: nnz is the scan's total)
    indices[p] = (uint32_t)(key & ((1ull << bits) - 1));
    rows[p] = (uint32_t)(key >> bits);
    const uint32_t l = line[j];
    const double w = l < m ? w64[l] : 0.0;
    data[p] = (float)w;            // the winner's weight as parsed, rounded once to float32 (to_csr)
    if (data64) data64[p] = w;     // ... and as parsed (to_dense keeps the Python float): the dense build's values
}

__global__ void __launch_bounds__(256)
coo_indptr_kernel(const uint32_t *__restrict__ rows, uint64_t nnz, uint64_t n_nodes, uint32_t *__restrict__ indptr) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_nodes) return;
    uint64_t lo = 0, hi = nnz;   // first entry whose row is >= r
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rows[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    indptr[r] = (uint32_t)lo;
}

}  // namespace pw
