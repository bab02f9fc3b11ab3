// walk_text.hip.h -- the walk corpus file written from device memory (gfx950): pw_walks_write_text_device, pw_walks_write_text.
//
// A row r of the walk matrix uint32[n_walks, walk_length + 2] with len = r[walk_length + 1] gives one line: the names of
// r[0] .. r[len - 1] joined by single spaces, then "\n" (len == 0: just "\n").  Cells at positions >= len are never read.
// The names are gathered by node index from the blob and offsets of pw_vectors_write_text_device.  The shape of
// emb_text.hip.h, whose stage store and piece size are used as they are:
//   walk_text_count_kernel   one wavefront per row, lane l takes tokens l, l + 64, ...: the sum of name length + 1 in 64 bits.
//                            Also the validation pass: a length above walk_length + 1, or a token >= n_names among the first
//                            len cells, is compared -- never used as an index --, the row counts as 0 bytes and its number goes
//                            to found[0] (length) or found[1] (token) with an atomic minimum, so the host names the first such row
//                            whatever the order the wavefronts ran in; it launches no fill pass then.
//   exclusive scan           of the row counts in place, in 64 bits (scan.hip.h)
//   walk_text_fill_kernel    one wavefront per row, 64 tokens per trip: a lane holds its token's name offset and length, the
//                            scan of length + 1 over the lanes gives its position in the trip's text.  A trip whose text fits
//                            the stage (EMB_PIECE bytes: every trip of names up to 47 bytes) is assembled there -- a lane copies
//                            its name and the separator, ' ' or '\n' behind the row's last token -- at the destination's skew
//                            and leaves through emb_stage_out as 16-byte stores.  Otherwise (wave-uniform) the trip's tokens go
//                            one after another, name and separator in pieces of at most EMB_PIECE bytes copied by all lanes, the
//                            way emb_fill_kernel writes a long row name.
// Name lengths are read where the offsets are, id_off[token + 1] - id_off[token]: two adjacent 8-byte reads that share a
// 64-byte line seven times out of eight.  A uint32 name_len[n_names] built per call would make the count pass's gather 4
// bytes, but the fill pass needs the 8-byte offset anyway, both tables sit in the Infinity Cache side by side (32 MB + 16 MB
// at RMAT-22), and the array would add an allocation, a kernel and a pass over the offsets to every call: not built.
// The host bounds every name by WALK_NAME_MAX so that a trip's text (64 names and separators) is counted in 32 bits.
// No atomics for positions: every byte position is a function of the input alone.
#pragma once
#include "emb_text.hip.h"

namespace pw {

constexpr uint64_t WALK_NAME_MAX = (1ull << 25) - 1;   // bytes of one name: 64 * (name + 1) < 2^32

// ---- row byte counts, and the check of everything the fill pass will use as an index ----------------------------------------
// found[0] / found[1]: the lowest row with a length above walk_length + 1 / with a token >= n_names (initially all ones);
// found[2]: the tokens of all other rows (initially 0; one add per wavefront)
__global__ void __launch_bounds__(256)
walk_text_count_kernel(const uint32_t *__restrict__ walks, uint64_t n_walks, uint32_t walk_length, const uint64_t *__restrict__ id_off,
                       uint64_t n_names, uint64_t *__restrict__ row_bytes, unsigned long long *__restrict__ found) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u, width = (uint64_t)walk_length + 2u;
    uint64_t tokens = 0;
    for (uint64_t row = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); row < n_walks; row += n_waves) {
        const uint32_t *__restrict__ src = walks + row * width;
        const uint32_t len = src[walk_length + 1u];
        if (len > walk_length + 1u) {   // (wave-uniform) no cell of the row is looked at
            if (lane == 0) {
                atomicMin(found, (unsigned long long)row);
                row_bytes[row] = 0;
            }
            continue;
        }
        uint64_t mine = 0;
        bool ok = true;
        for (uint32_t c = lane; c < len; c += WAVE) {
            const uint64_t tok = src[c];
            if (tok < n_names) mine += id_off[tok + 1] - id_off[tok] + 1u;   // name + ' ' (or '\n' behind the last)
            else ok = false;
        }
        const uint64_t incl = wave_incl_scan_u64(mine);
        const bool all_ok = ballot(!ok) == 0;
        if (lane == WAVE - 1) {
            if (!all_ok) atomicMin(found + 1, (unsigned long long)row);
            row_bytes[row] = !all_ok ? 0ull : len ? incl : 1ull;
        }
        if (all_ok) tokens += len;
    }
    if (lane == 0 && tokens) atomicAdd(found + 2, (unsigned long long)tokens);
}

// ---- text of rows [row_lo, row_hi) at buf[row_off[row] - row_off[row_lo]] ------------------------------------------------------
// flags[0] is raised (by lane 0) when a row's text would leave the bytes the count pass gave it; such a piece is not stored.
// The pass repeats the count pass's two comparisons -- length cell, token < n_names -- on purpose, although the host launches
// it only behind a count pass without findings on a matrix nobody writes: they cost two compares per token, and they keep
// "nothing out of range is dereferenced" a property of this kernel alone.  A row or token they refuse writes nothing (the
// token takes no bytes, not even a separator) and raises the flag as well.
__global__ void __launch_bounds__(256)
walk_text_fill_kernel(const uint32_t *__restrict__ walks, uint64_t row_lo, uint64_t row_hi, uint32_t walk_length,
                      const char *__restrict__ id_chars, const uint64_t *__restrict__ id_off, uint64_t n_names,
                      const uint64_t *__restrict__ row_off, char *__restrict__ buf, uint32_t *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) char s_stage[4][EMB_STAGE];
    const uint32_t lane = (uint32_t)lane_id();
    char *stage = s_stage[threadIdx.x >> 6];
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u, base = row_off[row_lo], width = (uint64_t)walk_length + 2u;
    for (uint64_t row = row_lo + (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); row < row_hi; row += n_waves) {
        uint64_t pos = row_off[row] - base;
        const uint64_t row_end = row_off[row + 1] - base;
        const uint32_t *__restrict__ src = walks + row * width;
        const uint32_t len = src[walk_length + 1u];
        if (len > walk_length + 1u) {
            if (lane == 0) atomicOr(flags, 1u);
            continue;
        }
        if (len == 0) {   // the empty line
            if (pos + 1u == row_end) {
                if (lane == 0) buf[pos] = '\n';
            } else if (lane == 0) atomicOr(flags, 1u);
            continue;
        }
        for (uint32_t t = 0; t < len; t += WAVE) {
            const uint32_t c = t + lane;
            const bool active = c < len;
            const char sep = c + 1u == len ? '\n' : ' ';
            uint64_t name_lo = 0;
            uint32_t name_len = 0, text = 0;   // text: name + separator; 0 for a lane without a token
            bool refused = false;
            if (active) {
                const uint64_t tok = src[c];
                if (tok < n_names) {
                    name_lo = id_off[tok];
                    name_len = (uint32_t)(id_off[tok + 1] - name_lo);   // (<= WALK_NAME_MAX: the host's check)
                    text = name_len + 1u;
                } else refused = true;
            }
            if (ballot(refused) != 0 && lane == 0) atomicOr(flags, 1u);
            const uint32_t incl = wave_incl_scan_u32(text);
            const uint32_t total = readlane_u32(incl, WAVE - 1);
            if (total <= EMB_PIECE) {   // (wave-uniform) the common case: the trip's text through the stage at once
                const uint32_t skew = (uint32_t)((uintptr_t)(buf + pos) & 15u);
                if (text) {
                    char *o = stage + skew + (incl - text);
                    const char *__restrict__ name = id_chars + name_lo;
                    for (uint32_t j = 0; j < name_len; j++) o[j] = name[j];
                    o[name_len] = sep;
                }
                wave_lds_fence();
                if (pos + total <= row_end) emb_stage_out(stage, skew, total, buf + pos);
                else if (lane == 0) atomicOr(flags, 1u);
                wave_lds_fence();
                pos += total;
                continue;
            }
            // long names: token after token, name and separator in pieces all lanes copy
            const uint32_t n_tok = len - t < (uint32_t)WAVE ? len - t : (uint32_t)WAVE;
            for (uint32_t k = 0; k < n_tok; k++) {
                const uint64_t k_lo = readlane_u64(name_lo, (int)k);
                const uint32_t k_text = readlane_u32(text, (int)k), k_len = k_text - 1u;   // (k_text == 0: refused, no bytes)
                const char k_sep = t + k + 1u == len ? '\n' : ' ';
                for (uint32_t o = 0; o < k_text; o += EMB_PIECE) {
                    const uint32_t n = k_text - o < EMB_PIECE ? k_text - o : EMB_PIECE;
                    const uint32_t skew = (uint32_t)((uintptr_t)(buf + pos) & 15u);
                    for (uint32_t j = lane; j < n; j += WAVE) stage[skew + j] = o + j < k_len ? id_chars[k_lo + o + j] : k_sep;
                    wave_lds_fence();
                    if (pos + n <= row_end) emb_stage_out(stage, skew, n, buf + pos);
                    else if (lane == 0) atomicOr(flags, 1u);
                    wave_lds_fence();
                    pos += n;
                }
            }
        }
        if (pos != row_end && lane == 0) atomicOr(flags, 1u);
    }
}

}  // namespace pw
