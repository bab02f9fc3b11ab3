// emb_text.hip.h -- the word2vec text file written from device memory (gfx950): pw_vectors_write_text_device,
// pw_vectors_write_text, pw_selftest_format_f6.
//
// A row of the file is  name, then " " + f6(x) for every component, then "\n",  f6(x) being the characters of C's
// printf("%.6f", (double)x) = Python's "%.6f" % float(x).  Three steps, the shape of dense_build.hip.h:
//   emb_count_kernel   one wavefront per row: every component's length, summed over the row's lanes, plus the name, the
//                      separators and the newline -> the row's byte count (uint64)
//   exclusive scan     of the row counts in place, in 64 bits (the file passes 4 GB at RMAT-22): scan.hip.h
//   emb_fill_kernel    one wavefront per row, 64 components per trip: a lane decomposes its value once (F6), the scan of
//                      the lengths over the lanes gives its position in the trip's text, the lanes write their characters to
//                      the wavefront's LDS stage, and the stage leaves as 16-byte vector stores at the text's final offset
//                      (the at most 15 bytes in front of and behind the aligned body as one byte store of consecutive lanes each)
// The lengths are recomputed in the fill pass, not kept: the pass needs the decomposition of every value to print it, and
// the length falls out of that; a byte per component kept between the passes would add a write and a read of n * dim bytes
// and an allocation, and save nothing.  No atomics: every position is a function of the input alone.
//
// f6_decompose is exact: the float32 is m * 2^e with integers m < 2^24 and -149 <= e <= 104.
//   e <  0   m * 10^6 < 2^44 is shifted right by -e with the remainder compared against one half (ties to even on the exact
//            binary value): the rounded count of millionths, split into integer part (< 2^24) and six decimals.  For -e > 45 the
//            product is below one half: zero, and no tie is possible.
//   e >= 0   an integer of up to 128 bits and 39 digits: m shifted left in base 10^9 limbs; the decimals are 000000.
// One text serves the device kernels and the host (pw_selftest_format_f6 with on_device = 0); the formatter half of this file
// compiles with a plain C++ compiler as well.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PW_F6_HD __host__ __device__ __forceinline__
#else
#define PW_F6_HD inline
#endif

namespace pw {

constexpr uint32_t F6_MAX_LEN = 47;   // sign, 39 digits, '.', six digits
constexpr uint32_t F6_SLOT = 48;      // pw_selftest_format_f6's slot; also " " + the longest value inside a row

struct F6 {
    uint32_t sign;      // 1: '-' in front (not for NaN)
    uint32_t special;   // 0: finite, 1: NaN, 2: infinity
    uint32_t limb[5];   // integer part in base 10^9, limb[0] least significant
    uint32_t frac;      // the six decimals, 0 .. 999999
};

PW_F6_HD uint32_t f6_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t b;
    memcpy(&b, &x, sizeof(b));
    return b;
#endif
}

PW_F6_HD F6 f6_decompose(float x) {
    const uint32_t b = f6_bits(x), ex = (b >> 23) & 0xffu, man = b & 0x7fffffu;
    F6 f;
    f.sign = b >> 31;
    f.special = 0;
    f.limb[0] = f.limb[1] = f.limb[2] = f.limb[3] = f.limb[4] = 0;
    f.frac = 0;
    if (ex == 0xffu) {
        f.special = man ? 1u : 2u;
        return f;
    }
    const uint32_t m = ex ? (man | 0x800000u) : man;   // |x| = m * 2^e
    const int e = (int)(ex ? ex : 1u) - 150;
    if (e < 0) {
        const uint32_t k = (uint32_t)-e;
        if (k <= 45) {
            const uint64_t prod = (uint64_t)m * 1000000ull, half = 1ull << (k - 1);
            const uint64_t rem = prod & ((half << 1) - 1ull);
            uint64_t q = prod >> k;
            if (rem > half || (rem == half && (q & 1ull))) q++;
            const uint64_t ip = q / 1000000ull;
            f.limb[0] = (uint32_t)ip;
            f.frac = (uint32_t)(q - ip * 1000000ull);
        }
        return f;
    }
    f.limb[0] = m;   // (m < 2^24 < 10^9)
    for (uint32_t left = (uint32_t)e; left > 0;) {
        const uint32_t s = left < 29u ? left : 29u;   // (10^9 - 1) * 2^29 + carry < 2^59
        uint64_t carry = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uint64_t t = ((uint64_t)f.limb[i] << s) + carry;
            carry = t / 1000000000ull;
            f.limb[i] = (uint32_t)(t - carry * 1000000000ull);
        }
        left -= s;
    }
    return f;
}

PW_F6_HD uint32_t f6_digits(uint32_t v) {   // decimal digits of v < 10^9 (1 for 0)
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
         : v < 10000000u ? 7u : v < 100000000u ? 8u : 9u;
}

// the number of characters f6_emit writes
PW_F6_HD uint32_t f6_len(const F6 &f) {
    if (f.special) return f.special == 1 ? 3u : 3u + f.sign;
    uint32_t nd = f6_digits(f.limb[0]);
#pragma unroll
    for (int k = 1; k < 5; k++)
        if (f.limb[k]) nd = 9u * (uint32_t)k + f6_digits(f.limb[k]);
    return f.sign + nd + 7u;
}

PW_F6_HD void f6_put(char *out, uint32_t v, uint32_t nd) {   // the last nd decimal digits of v
    for (uint32_t i = nd; i-- > 0;) {
        const uint32_t q = v / 10u;
        out[i] = (char)('0' + (v - q * 10u));
        v = q;
    }
}

PW_F6_HD uint32_t f6_emit(const F6 &f, char *out) {
    uint32_t p = 0;
    if (f.special == 1) {
        out[0] = 'n'; out[1] = 'a'; out[2] = 'n';
        return 3;
    }
    if (f.sign) out[p++] = '-';
    if (f.special == 2) {
        out[p] = 'i'; out[p + 1] = 'n'; out[p + 2] = 'f';
        return p + 3;
    }
    bool started = false;
#pragma unroll
    for (int k = 4; k >= 0; k--) {
        const uint32_t v = f.limb[k];
        if (started) {
            f6_put(out + p, v, 9);
            p += 9;
        } else if (v || k == 0) {
            const uint32_t nd = f6_digits(v);
            f6_put(out + p, v, nd);
            p += nd;
            started = true;
        }
    }
    out[p++] = '.';
    f6_put(out + p, f.frac, 6);
    return p + 6;
}

// the characters of printf("%.6f", (double)x) at out[0 ..), at most F6_MAX_LEN of them; returns their count
PW_F6_HD uint32_t format_f6(float x, char *out) { return f6_emit(f6_decompose(x), out); }

}  // namespace pw

#if defined(__HIPCC__)
#include "scan.hip.h"

namespace pw {

// pw_selftest_format_f6(on_device = 1): one thread per value, 48-byte slots (zeroed by the caller)
__global__ void __launch_bounds__(256)
f6_selftest_kernel(const float *__restrict__ x, uint64_t n, char *__restrict__ chars, uint32_t *__restrict__ lens) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const F6 f = f6_decompose(x[i]);
    const uint32_t len = f6_emit(f, chars + i * F6_SLOT);
    lens[i] = len == f6_len(f) ? len : 0xffffffffu;   // (the count pass and the fill pass must agree)
}

// ---- row byte counts ---------------------------------------------------------------------------------------------------------
// One wavefront per row, rows strided over the wavefronts of the grid; lane l takes components l, l + 64, ...
__global__ void __launch_bounds__(256)
emb_count_kernel(const float *__restrict__ vec, uint64_t n_rows, uint32_t dim, const uint64_t *__restrict__ id_off,
                 uint64_t *__restrict__ row_bytes) {
    const int lane = lane_id();
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t row = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); row < n_rows; row += n_waves) {
        const float *__restrict__ src = vec + row * dim;
        uint64_t mine = 0;
        for (uint64_t c = (uint64_t)lane; c < dim; c += WAVE) mine += 1u + f6_len(f6_decompose(src[c]));   // " " + value
        const uint64_t incl = wave_incl_scan_u64(mine);
        if (lane == WAVE - 1) row_bytes[row] = (id_off[row + 1] - id_off[row]) + incl + 1u;   // + "\n"
    }
}

// ---- text of rows [row_lo, row_hi) at buf[row_off[row] - row_off[row_lo]] ------------------------------------------------------
// The stage of a wavefront holds one piece of a row -- up to EMB_PIECE bytes of the name, or the text of 64 components (and
// the newline behind the last) -- at the offset its destination has inside a 16-byte line, so that stage and destination
// share their alignment: the aligned body leaves as uint4 stores, the ends as byte stores of consecutive lanes.
constexpr uint32_t EMB_PIECE = WAVE * F6_SLOT;              // 3072
constexpr uint32_t EMB_STAGE = EMB_PIECE + 32;              // + 15 bytes of offset + "\n", rounded up to 16

__device__ __forceinline__ void emb_stage_out(const char *stage, uint32_t skew, uint32_t n_bytes, char *dst) {
    const uint32_t lane = (uint32_t)lane_id();
    char *line = dst - skew;   // 16-byte aligned; stage[i] belongs at line[i]
    const uint32_t begin = skew, end = skew + n_bytes;
    const uint32_t body_lo = (begin + 15u) & ~15u, body_hi = end & ~15u;
    if (body_lo >= body_hi) {   // (wave-uniform) fewer than 31 bytes, no whole line among them
        if (begin + lane < end) line[begin + lane] = stage[begin + lane];
        return;
    }
    if (begin + lane < body_lo) line[begin + lane] = stage[begin + lane];
    for (uint32_t i = body_lo + 16u * lane; i < body_hi; i += 16u * WAVE)
        *reinterpret_cast<uint4 *>(line + i) = *reinterpret_cast<const uint4 *>(stage + i);
    if (body_hi + lane < end) line[body_hi + lane] = stage[body_hi + lane];
}

// flags[0] is raised when a row's text would leave the bytes the count pass gave it (it cannot: both passes take every length
// from f6_len of the same decomposition); such a piece is not stored.
__global__ void __launch_bounds__(256)
emb_fill_kernel(const float *__restrict__ vec, uint64_t row_lo, uint64_t row_hi, uint32_t dim, const char *__restrict__ id_chars,
                const uint64_t *__restrict__ id_off, const uint64_t *__restrict__ row_off, char *__restrict__ buf,
                uint32_t *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) char s_stage[4][EMB_STAGE];
    const uint32_t lane = (uint32_t)lane_id();
    char *stage = s_stage[threadIdx.x >> 6];
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u, base = row_off[row_lo];
    for (uint64_t row = row_lo + (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); row < row_hi; row += n_waves) {
        uint64_t pos = row_off[row] - base;
        const uint64_t row_end = row_off[row + 1] - base;
        const uint64_t name_lo = id_off[row], name_len = id_off[row + 1] - name_lo;
        for (uint64_t o = 0; o < name_len; o += EMB_PIECE) {
            const uint32_t n = (uint32_t)(name_len - o < EMB_PIECE ? name_len - o : EMB_PIECE);
            const uint32_t skew = (uint32_t)((uintptr_t)(buf + pos) & 15u);
            for (uint32_t j = lane; j < n; j += WAVE) stage[skew + j] = id_chars[name_lo + o + j];
            wave_lds_fence();
            if (pos + n <= row_end) emb_stage_out(stage, skew, n, buf + pos);
            else if (lane == 0) atomicOr(flags, 1u);
            wave_lds_fence();
            pos += n;
        }
        const float *__restrict__ src = vec + row * dim;
        for (uint64_t t = 0; t < dim; t += WAVE) {
            const uint64_t c = t + lane;
            const bool active = c < dim, last = c + 1 == dim;
            F6 f;
            uint32_t len = 0;
            if (active) {
                f = f6_decompose(src[c]);
                len = 1u + f6_len(f) + (last ? 1u : 0u);
            }
            const uint32_t incl = wave_incl_scan_u32(len);
            const uint32_t total = readlane_u32(incl, WAVE - 1);
            const uint32_t skew = (uint32_t)((uintptr_t)(buf + pos) & 15u);
            if (active) {
                char *o = stage + skew + (incl - len);
                o[0] = ' ';
                const uint32_t w = f6_emit(f, o + 1);
                if (last) o[1 + w] = '\n';
            }
            wave_lds_fence();
            if (pos + total <= row_end) emb_stage_out(stage, skew, total, buf + pos);
            else if (lane == 0) atomicOr(flags, 1u);
            wave_lds_fence();
            pos += total;
        }
        if (pos != row_end && lane == 0) atomicOr(flags, 1u);
    }
}

}  // namespace pw
#endif  // __HIPCC__
