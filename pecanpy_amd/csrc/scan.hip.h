// scan.hip.h -- the exclusive prefix sum of the library (gfx950): one workgroup scan, one kernel pair, one host entry.
//
// Every offset table of the auxiliary kernels is the exclusive prefix sum of a per-element count: the ranks of the kept edges
// and the radix histograms (coo_csr.hip.h), the line and vertex numbers of the edge-list reader, the row offsets of the text
// writers, the list / log / table offsets of the lane index (walk_lanes.hip.h), the stream offsets of the jobs
// (aux_kernels.hip.h).  Integer sums: the result does not depend on how it is computed.
//
//   block_excl_scan      one value per thread over the 256 threads of a workgroup: the wavefronts' DPP scans and four totals
//   tile_sums_kernel     sums[b] = the counts of tile b (256 threads x 16 consecutive elements)
//   tile_offsets_kernel  emit(i, scanned sums[tile of i] + the counts before i in its tile)
//   exclusive_scan       tile sums, the same scan of the tile sums in place (recursively: 4096 elements per level), offsets
// The counts come from a functor  count(i)  and the results leave through a functor  emit(i, offset)  -- structs, so that the
// kernels carry their callers' names in a trace.  A scan of an array in place is the pair ScanLoad / ScanStore.  The sums are
// of the type S of the scratch array: uint64_t, or uint32_t where the caller knows that the total fits.
//
// Scratch: scan_scratch_elems(n) words of S.  scratch[0] receives the GRAND TOTAL; the tile sums of the first level start at
// scratch + 1 and those of the levels above follow them.  n == 0 launches no kernel (the total is set to 0).
//
// Tile size: 16 elements per thread for every type.  The compiler's resource report shows no scratch for any instantiation
// (the sixteen 64-bit counts of a thread are 32 VGPRs), and a thread's elements are one or two whole 64-byte lines; eight
// per thread, what the 64-bit scan of the text writers had, only doubles the tile sums of the level above.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave.h"

namespace pw {

constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_ITEMS = 16;                       // consecutive elements per thread
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;   // elements per workgroup

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) { return wave_incl_scan_u32(v); }
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) { return wave_incl_scan_u64(v); }

// exclusive scan of one value per thread over the 256 threads of the workgroup, *total = their sum; `wave_tot` = 4 words of
// LDS that the caller does not touch between two calls without a barrier of its own
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T *wave_tot, T *total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const T incl = wave_incl_scan(v);
    if (lane == WAVE - 1) wave_tot[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const T t = wave_tot[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + incl - v;
}

// the smallest of one value per thread over the workgroup, in every thread; `wave_min` as wave_tot above
__device__ __forceinline__ uint64_t block_min(uint64_t v, uint64_t *wave_min) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const uint64_t t = (uint64_t)__shfl_xor((long long)v, d, WAVE);
        if (t < v) v = t;
    }
    if (lane_id() == 0) wave_min[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; w++)
        if (wave_min[w] < v) v = wave_min[w];
    return v;
}

// first element of this thread in this workgroup's tile
__device__ __forceinline__ uint64_t tile_first() { return (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS; }

// loc[k] = count of the thread's element k (0 behind the end); returns their sum
template <typename S, class Count, typename C>
__device__ __forceinline__ S tile_load(const Count &count, uint64_t n, C (&loc)[SCAN_ITEMS]) {
    const uint64_t first = tile_first();
    S s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        loc[k] = first + k < n ? count(first + k) : C(0);
        s += loc[k];
    }
    return s;
}

template <typename S, class Count>
__global__ void __launch_bounds__(SCAN_BLOCK)
tile_sums_kernel(uint64_t n, Count count, S *__restrict__ sums) {
    __shared__ S wave_tot[4];
    decltype(count(0ull)) loc[SCAN_ITEMS];
    S total;
    (void)block_excl_scan(tile_load<S>(count, n, loc), wave_tot, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: the scanned tile sums; NULL = the only tile, whose total goes to *total (the only launch that passes one)
template <typename S, class Count, class Emit>
__global__ void __launch_bounds__(SCAN_BLOCK)
tile_offsets_kernel(uint64_t n, Count count, Emit emit, const S *__restrict__ sums, S *__restrict__ total) {
    __shared__ S wave_tot[4];
    decltype(count(0ull)) loc[SCAN_ITEMS];
    const S s = tile_load<S>(count, n, loc);
    S all;
    S run = block_excl_scan(s, wave_tot, &all) + (sums ? sums[blockIdx.x] : S(0));
    if (total && threadIdx.x == 0) *total = all;
    const uint64_t first = tile_first();
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (first + k < n) emit(first + k, run);
        run += loc[k];
    }
}

template <typename T> struct ScanLoad {
    const T *x;
    __device__ T operator()(uint64_t i) const { return x[i]; }
};
template <typename T> struct ScanStore {
    T *x;
    __device__ void operator()(uint64_t i, T offset) const { x[i] = offset; }
};

// ---- host -------------------------------------------------------------------------------------------------------------------
inline uint64_t scan_tiles(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

inline uint64_t scan_scratch_elems(uint64_t n) {   // the total, and the tile sums of every level down to a single tile
    uint64_t words = 1;
    do {
        n = scan_tiles(n);
        words += n;
    } while (n > 1);
    return words;
}

// n >= 1.  sums: room for the tile sums of this level and, behind them, of the levels above
template <typename S, class Count, class Emit>
void scan_levels(hipStream_t stream, uint64_t n, Count count, Emit emit, S *sums, S *total) {
    const unsigned tiles = (unsigned)scan_tiles(n);
    if (tiles == 1) {
        hipLaunchKernelGGL((tile_offsets_kernel<S, Count, Emit>), dim3(1), dim3(SCAN_BLOCK), 0, stream, n, count, emit, (const S *)nullptr, total);
        return;
    }
    hipLaunchKernelGGL((tile_sums_kernel<S, Count>), dim3(tiles), dim3(SCAN_BLOCK), 0, stream, n, count, sums);
    scan_levels(stream, tiles, ScanLoad<S>{sums}, ScanStore<S>{sums}, sums + tiles, total);
    hipLaunchKernelGGL((tile_offsets_kernel<S, Count, Emit>), dim3(tiles), dim3(SCAN_BLOCK), 0, stream, n, count, emit, (const S *)sums, (S *)nullptr);
}

// emit(i, count(0) + ... + count(i - 1)) for i in [0, n), scratch[0] = count(0) + ... + count(n - 1)
template <typename S, class Count, class Emit>
void exclusive_scan(hipStream_t stream, uint64_t n, Count count, Emit emit, S *scratch) {
    if (n == 0) (void)hipMemsetAsync(scratch, 0, sizeof(S), stream);
    else scan_levels(stream, n, count, emit, scratch + 1, scratch);
}
// x[0, n) in place
template <typename T>
void exclusive_scan_inplace(hipStream_t stream, T *x, uint64_t n, T *scratch) {
    exclusive_scan(stream, n, ScanLoad<T>{x}, ScanStore<T>{x}, scratch);
}
// For a caller with a first or a last level of its own (clist_tile_sums_kernel: two sums in one pass; draws_offsets_kernel:
// more than an offset per job): the scan's levels above the first -- the n_tiles >= 1 tile sums that the caller's kernel left
// at scratch + 1 are scanned in place, scratch[0] = their total -- between scan_tile_sums and scan_tile_offsets or its own.
template <typename S>
void scan_sums(hipStream_t stream, uint64_t n_tiles, S *scratch) {
    scan_levels(stream, n_tiles, ScanLoad<S>{scratch + 1}, ScanStore<S>{scratch + 1}, scratch + 1 + n_tiles, scratch);
}
template <typename S, class Count>
void scan_tile_sums(hipStream_t stream, uint64_t n, Count count, S *scratch) {
    hipLaunchKernelGGL((tile_sums_kernel<S, Count>), dim3((unsigned)scan_tiles(n)), dim3(SCAN_BLOCK), 0, stream, n, count, scratch + 1);
}
template <typename S, class Count, class Emit>
void scan_tile_offsets(hipStream_t stream, uint64_t n, Count count, Emit emit, S *scratch) {
    hipLaunchKernelGGL((tile_offsets_kernel<S, Count, Emit>), dim3((unsigned)scan_tiles(n)), dim3(SCAN_BLOCK), 0, stream, n, count, emit,
                       (const S *)(scratch + 1), (S *)nullptr);
}

}  // namespace pw
