// dense_build.hip.h -- dense graph handles built on the device (gfx950): pw_dense_create_device, pw_dense_create_from_csr,
// pw_dense_noise_thresholds.
//
// The handle's declared format: packed adjacency rows adjbits u64[n][ceil(n / 64)], the non-zeros of
// every row compressed in ascending column order (indices u32, data f64 -- dropped when every value is 1.0), deg, indptr and
// the flags unit / dense_nonneg.  pw_dense_create makes it on one host thread; here a row-major matrix that is already in
// device memory is turned into the same arrays by two streams over the matrix:
//   dense_count_kernel   a wavefront reads 64 consecutive columns of a row (lane l = column 64 k + l: one coalesced
//                        request); the ballot of v != 0 IS word k of the row's adjbits, its population count adds to the
//                        row's degree; the two flags are reduced with the host code's predicates
//   (host)               indptr = prefix sum of the degrees, the 2^32 - 1 edge limit, max_degree
//   dense_fill_kernel    entry (i, x) goes to indptr[i] + population of the row's earlier words + population of its own word
//                        below its bit: ascending columns, a function of the input alone
// and a CSR in device memory (pw_csr_dev) by csr_to_dense_kernel: bits set from the CSR rows, values widened to float64 -- or,
// for the CSR of an edge-list file read with its float64 weights kept, those weights as parsed.
// Atomics produce flags (atomicOr of constant bits) and the bits of a SET (csr_to_dense_kernel) only: no position and no
// value depends on the order they arrive in.  One workgroup of 256 threads per row, rows strided over the grid; one code
// path for every n >= 1 and every row population from 0 to n.
//
// threshold_row is the node2vec+ threshold of ONE row, restating pw::numpy_mean_std / noise_thresholds_dense
// (thresholds.hpp) without a scratch array and without recursion, so that one text serves the device kernel and the host
// (pw_selftest_thresholds_row).  -ffp-contract=off is part of its contract: a fused multiply-add anywhere in it changes bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scan.hip.h"

namespace pw {

constexpr uint32_t DENSE_FLAG_NOT_UNIT = 1u;      // some non-zero entry != 1.0
constexpr uint32_t DENSE_FLAG_NOT_NONNEG = 2u;    // some non-zero entry fails v > 0 && v < 2^1000 (NaN included)

__device__ __forceinline__ uint32_t dense_entry_flags(double v) {   // of a non-zero entry (pw_dense_create's predicates)
    return (v != 1.0 ? DENSE_FLAG_NOT_UNIT : 0u) | ((!(v > 0.0) || !(v < 0x1p1000)) ? DENSE_FLAG_NOT_NONNEG : 0u);
}

// ---- matrix -> adjbits, deg, flags ----------------------------------------------------------------------------------------
// Wave w of the workgroup takes words w, w + 4, ... of the row, DENSE_UNROLL of them per trip so that as many 512-byte
// requests are in flight per wavefront.  Lanes beyond column n - 1 load nothing and vote 0: the tail bits of every row's
// last word are zero (the walk kernels rely on that).
constexpr int DENSE_UNROLL = 4;

template <typename T>
__global__ void __launch_bounds__(256)
dense_count_kernel(const T *__restrict__ mat, uint32_t n, uint32_t wpr, uint64_t *__restrict__ adjbits, uint32_t *__restrict__ deg,
                   uint32_t *__restrict__ flags) {
    __shared__ uint32_t wave_deg[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t bad = 0;
    for (uint32_t row = blockIdx.x; row < n; row += gridDim.x) {
        const T *__restrict__ src = mat + (uint64_t)row * n;
        uint64_t *__restrict__ bits = adjbits + (uint64_t)row * wpr;
        uint32_t count = 0;
        for (uint32_t k0 = (uint32_t)wave; k0 < wpr; k0 += 4 * DENSE_UNROLL) {
            double v[DENSE_UNROLL];
#pragma unroll
            for (int u = 0; u < DENSE_UNROLL; u++) {
                const uint64_t col = (uint64_t)(k0 + 4u * u) * 64u + (uint32_t)lane;   // (k0 + 4 u < wpr + 16: no wrap)
                v[u] = col < n ? (double)src[col] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < DENSE_UNROLL; u++) {
                const uint32_t k = k0 + 4u * u;
                const uint64_t word = ballot(v[u] != 0.0);
                if (v[u] != 0.0) bad |= dense_entry_flags(v[u]);
                if (k < wpr) {   // (wave-uniform)
                    if (lane == 0) bits[k] = word;
                    count += (uint32_t)__popcll(word);
                }
            }
        }
        if (lane == 0) wave_deg[wave] = count;
        __syncthreads();
        if (threadIdx.x == 0) deg[row] = wave_deg[0] + wave_deg[1] + wave_deg[2] + wave_deg[3];
        __syncthreads();
    }
    const uint64_t any_unit = ballot((bad & DENSE_FLAG_NOT_UNIT) != 0), any_neg = ballot((bad & DENSE_FLAG_NOT_NONNEG) != 0);
    if (lane == 0 && (any_unit | any_neg))
        atomicOr(flags, (any_unit ? DENSE_FLAG_NOT_UNIT : 0u) | (any_neg ? DENSE_FLAG_NOT_NONNEG : 0u));
}

// ---- adjbits + matrix -> indices, data --------------------------------------------------------------------------------------
// The row's words go through LDS 256 at a time: thread t reads word c + t and the workgroup scans the 256 population counts
// (plus the count of the chunks before), then wave w takes words w, w + 4, ... of the chunk: lane l of a set bit writes column
// 64 k + l at indptr[row] + base[k] + popcount(word below bit l).  `mat` is not read when data == NULL (unit graphs).
template <typename T>
__global__ void __launch_bounds__(256)
dense_fill_kernel(const T *__restrict__ mat, uint32_t n, uint32_t wpr, const uint64_t *__restrict__ adjbits,
                  const uint32_t *__restrict__ indptr, uint32_t *__restrict__ indices, double *__restrict__ data) {
    __shared__ uint64_t s_word[256];
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_tot[4];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t row = blockIdx.x; row < n; row += gridDim.x) {
        const uint32_t first = indptr[row];
        if (indptr[row + 1] == first) continue;   // (the same for every thread of the workgroup)
        const T *__restrict__ src = mat + (uint64_t)row * n;
        const uint64_t *__restrict__ bits = adjbits + (uint64_t)row * wpr;
        uint32_t run = first;
        for (uint32_t c = 0; c < wpr; c += 256) {
            const uint32_t k = c + threadIdx.x;
            const uint64_t word = k < wpr ? bits[k] : 0ull;
            uint32_t total;
            const uint32_t before = block_excl_scan((uint32_t)__popcll(word), s_tot, &total);
            s_word[threadIdx.x] = word;
            s_base[threadIdx.x] = run + before;
            __syncthreads();
            const uint32_t m = wpr - c < 256u ? wpr - c : 256u;
            for (uint32_t j = (uint32_t)wave; j < m; j += 4) {
                const uint64_t w = s_word[j];
                if (w == 0) continue;   // (wave-uniform)
                if ((w >> lane) & 1ull) {
                    const uint32_t col = (c + j) * 64u + (uint32_t)lane;
                    const uint64_t pos = (uint64_t)s_base[j] + (uint32_t)__popcll(w & ((1ull << lane) - 1ull));
                    indices[pos] = col;
                    if (data) data[pos] = (double)src[col];
                }
            }
            run += total;
            __syncthreads();   // s_word / s_base / s_tot are rewritten by the next chunk
        }
    }
}

// ---- device CSR -> adjbits (zeroed by the caller), data64, deg, flags ----------------------------------------------------------
// One wavefront per row, rows strided over the waves of the grid.  The bits are a set: atomicOr of single bits, the result
// does not depend on arrival order.  W = float: the CSR's float32 weights, widened (exact); W = double: the float64 weights an
// edge-list file's CSR carries beside them (coo_compact_lines_kernel), stored as they are -- the flags are reduced from the
// float64 values either way, so 1.00000001 (1.0 in float32) is not unit.  src == NULL: every weight is 1.0 (nothing stored,
// no flag raised).
template <typename W>
__global__ void __launch_bounds__(256)
csr_to_dense_kernel(const uint32_t *__restrict__ indptr, const uint32_t *__restrict__ indices, const W *__restrict__ src,
                    uint32_t n, uint32_t wpr, uint64_t *__restrict__ adjbits, double *__restrict__ data64, uint32_t *__restrict__ deg,
                    uint32_t *__restrict__ flags) {
    const int lane = lane_id();
    const uint32_t n_waves = gridDim.x * 4u;
    uint32_t bad = 0;
    for (uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6); row < n; row += n_waves) {
        const uint32_t lo = indptr[row], hi = indptr[row + 1];
        if (lane == 0) deg[row] = hi - lo;
        unsigned long long *bits = (unsigned long long *)(adjbits + (uint64_t)row * wpr);
        for (uint32_t e = lo + (uint32_t)lane; e < hi; e += WAVE) {
            const uint32_t col = indices[e];
            if (col < n) atomicOr(&bits[col >> 6], 1ull << (col & 63u));   // (a CSR of pw_coo_to_csr_device has no column >= n)
            if (src) {
                const double v = (double)src[e];
                data64[e] = v;
                bad |= dense_entry_flags(v);
            }
        }
    }
    const uint64_t any_unit = ballot((bad & DENSE_FLAG_NOT_UNIT) != 0), any_neg = ballot((bad & DENSE_FLAG_NOT_NONNEG) != 0);
    if (lane == 0 && (any_unit | any_neg))
        atomicOr(flags, (any_unit ? DENSE_FLAG_NOT_UNIT : 0u) | (any_neg ? DENSE_FLAG_NOT_NONNEG : 0u));
}

// ---- node2vec+ threshold of one row -----------------------------------------------------------------------------------------
// NumPy's pairwise_sum over get(off) .. get(off + n - 1), n <= 128: eight accumulators, then the tail one by one
template <typename Get>
__host__ __device__ inline double numpy_pairwise_leaf(const Get &get, uint64_t off, uint32_t n) {
    if (n < 8) {
        double res = 0.0;
        for (uint32_t i = 0; i < n; i++) res = res + get(off + i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = get(off + j);
    uint32_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] = r[j] + get(off + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res = res + get(off + i);
    return res;
}

// NumPy's pairwise_sum for n <= 8192 (one buffer of the reduction): above 128 elements it splits at n2 = n / 2 rounded down to
// a multiple of 8 and adds the two halves' sums, left + right.  The tree is a fixed function of n; it is walked here with an
// explicit stack (8192 elements: 7 levels; a right half is at most 7 elements longer than n / 2, so 16 frames are never reached).
template <typename Get>
__host__ __device__ inline double numpy_pairwise_buffer(const Get &get, uint64_t off, uint32_t n) {
    constexpr int DEPTH = 16;
    uint64_t f_off[DEPTH];
    uint32_t f_n[DEPTH];
    double f_left[DEPTH];
    uint8_t f_state[DEPTH];   // 0: nothing done, 1: left half running, 2: right half running
    int sp = 0;
    f_off[0] = off; f_n[0] = n; f_state[0] = 0;
    sp = 1;
    double ret = 0.0;
    while (sp > 0) {
        const int t = sp - 1;
        const uint32_t len = f_n[t];
        if (len <= 128 || sp == DEPTH) {   // (sp == DEPTH cannot happen for n <= 8192; a leaf keeps the walk bounded)
            ret = len <= 128 ? numpy_pairwise_leaf(get, f_off[t], len) : 0.0;
            sp--;
            continue;
        }
        uint32_t n2 = len / 2;
        n2 -= n2 % 8;
        if (f_state[t] == 0) {
            f_state[t] = 1;
            f_off[sp] = f_off[t]; f_n[sp] = n2; f_state[sp] = 0;
            sp++;
        } else if (f_state[t] == 1) {
            f_left[t] = ret;
            f_state[t] = 2;
            f_off[sp] = f_off[t] + n2; f_n[sp] = len - n2; f_state[sp] = 0;
            sp++;
        } else {
            ret = f_left[t] + ret;
            sp--;
        }
    }
    return ret;
}

// np.add.reduce: out = out + pairwise_sum(buffer) per buffer of 8192 elements, starting from 0
template <typename Get>
__host__ __device__ inline double numpy_add_reduce_fn(const Get &get, uint64_t n) {
    double acc = 0.0;
    for (uint64_t i = 0; i < n; i += 8192) acc = acc + numpy_pairwise_buffer(get, i, (uint32_t)(n - i < 8192 ? n - i : 8192));
    return acc;
}

// max(mean + gamma * std, 0) of the n values get(0) .. get(n - 1) as noise_thresholds_dense computes it from a row's non-zeros:
// mean = sum / n, var = sum((a - mean)^2) / n with the squares recomputed inside the second reduction, std = sqrt(var), the
// sum rounded to float32, NaN propagating through the maximum; n == 0 gives NaN (0 / 0)
template <typename Get>
__host__ __device__ inline float threshold_row(const Get &get, uint64_t n, double gamma) {
    const double cnt = (double)n;
    const double mean = numpy_add_reduce_fn(get, n) / cnt;
    const auto sq = [&get, mean](uint64_t i) {
        const double x = get(i) - mean;
        return x * x;
    };
    const double var = numpy_add_reduce_fn(sq, n) / cnt;
    const double s = sqrt(var);
    const float t = (float)(mean + gamma * s);
    return (t != t) ? t : (t > 0.0f ? t : 0.0f);
}

// one thread per row of the handle's compressed rows; data == NULL: every value is 1.0 (unit handles)
__global__ void __launch_bounds__(256)
dense_thresholds_kernel(const uint32_t *__restrict__ indptr, const double *__restrict__ data, uint32_t n, double gamma,
                        float *__restrict__ thr) {
    for (uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (uint64_t)gridDim.x * 256) {
        const uint32_t lo = indptr[row], len = indptr[row + 1] - lo;
        if (data) {
            const double *a = data + lo;
            thr[row] = threshold_row([a](uint64_t i) { return a[i]; }, len, gamma);
        } else {
            thr[row] = threshold_row([](uint64_t) { return 1.0; }, len, gamma);
        }
    }
}

}  // namespace pw
