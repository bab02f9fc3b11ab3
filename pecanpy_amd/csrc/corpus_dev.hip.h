// corpus_dev.hip.h -- a walk corpus FILE read in device memory (gfx950): pw_corpus_read_device, the inverse of walk_text.hip.h.
//
// The text of the file -> the walk matrix uint32[n_lines, W] that corpus.read_walks defines (a row = the numbers of the line's
// tokens, zeros, the token count in the last cell; W = the longest line's tokens, at least 1, plus 1) with the tokens numbered
// by first appearance, and the (offset, length) of every name.  The reader is optimistic the way edgelist_dev.hip.h is: it
// takes files whose bytes are all in {\t, \n, \r, 0x20 .. 0x7E} and raises a decline flag for any other byte (\v, \f, 0x1C ..
// 0x1F, NUL, 0x7F, everything from 0x80 up -- among them the Unicode white space that str.split() knows and a byte scan does
// not); the caller then reports "needs the host reader", which is no error.  Space, \t and \r separate tokens, \n ends a line.
//
// The work is parallel over BYTES and over TOKENS, never over lines: one line may be the whole file.
//
//   1. cp_count_kernel      one wavefront per 1024-byte segment, 16 bytes per lane (edgelist_dev.hip.h's segments): the byte
//                           classes, the decline flag, and per segment the newlines and the token starts (a token byte whose
//                           predecessor is a separator, a newline or the beginning of the file; a lane has its predecessor
//                           from the lane below it, lane 0 from memory)
//   2. scans of both counts (scan.hip.h)
//      cp_place_kernel      the same segments again: token start t learns its offset and its line (the newlines in front of
//                           it); line k + 1 learns its first token (the token starts in front of newline k)
//      cp_width_kernel      one thread per line: the most tokens in a line (a wavefront's maximum, one atomicMax per wavefront)
//   3. cp_tokens_kernel     one thread per token: its end, its FNV-1a hash (el_hash), the record (offset, length, hash)
//      el_insert_kernel     } edgelist_dev.hip.h's id table as it stands: open addressing over token POSITIONS keyed by the
//      el_first_kernel      } string's hash; first[p] = token p's slot holds p; the exclusive scan of first[] is the name number
//   4. cp_fill_kernel       one thread per token: out[line * W + (t - first token of line)] = the number of its slot's occupant;
//                           a first appearance also records its name's span
//      cp_lengths_kernel    one thread per line: the count cell.  The matrix is zeroed once by a memset in front of both.
//
// Determinism: every output word is a function of the text alone.  The byte passes, the scans and the token records are plain
// functions of the bytes.  For the id table the argument of edgelist_dev.hip.h holds word for word, the kernel being the
// same: a slot that is occupied stays occupied, and by the same STRING for good -- only tokens with equal bytes ever replace its
// value, and only by a smaller position.  Two tokens with equal strings walk the same probe sequence and see, slot for slot,
// either another string (for good) or a slot that ends up theirs, so they end in ONE slot; the minimum over all of them is that
// slot's final value whatever the order in which the atomics arrive, and it is the string's first appearance.  Which slot a
// string lands in does depend on the arrival order -- nothing downstream reads a slot number: name numbers are ranks of first
// appearances in token order.  The width is an atomicMax and the flags are atomicOr of values that are functions of the text.
// Every matrix cell has exactly one writer (the memset, then one token or one line).
#pragma once
#include <stdint.h>

#include "edgelist_dev.hip.h"

#if defined(__HIPCC__)
namespace pw {

constexpr int CP_SEG = EL_SEG;   // bytes per wavefront in the byte passes (16 per lane)

__device__ __forceinline__ bool cp_is_token_byte(unsigned char b) { return b >= 0x21 && b <= 0x7E; }

// ---- 1. byte classes, newline and token-start counts ------------------------------------------------------------------------
// The 16 bytes of this lane at `first` (a multiple of 16): *nl = newline mask, *ts = token-start mask (bit k = byte k),
// bad = a byte outside the accepted set.  Every lane of the wavefront calls it (a shuffle hands the predecessor byte up).
__device__ __forceinline__ bool cp_lane_bytes(const char *__restrict__ text, uint64_t n, uint64_t first, uint32_t *nl, uint32_t *ts) {
    unsigned char c[16];
    int valid = 0;
    if (first + 16 <= n) {
        const uint4 v = *(const uint4 *)(text + first);   // (first is a multiple of 16, the buffer comes from hipMalloc)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) c[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
        valid = 16;
    } else {
        valid = first < n ? (int)(n - first) : 0;
#pragma unroll
        for (int k = 0; k < 16; k++) c[k] = k < valid ? (unsigned char)text[first + k] : (unsigned char)'\n';
    }
    // the byte in front of this lane's: the lane below holds it (a lane with bytes has a full lane below it)
    uint32_t prev = (uint32_t)__shfl_up((int)c[15], 1u, WAVE);
    if (lane_id() == 0) prev = first > 0 && first <= n ? (unsigned char)text[first - 1] : (unsigned char)'\n';
    uint32_t tok = 0, newline = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const unsigned char b = c[k];
        if (k >= valid) continue;
        if (cp_is_token_byte(b)) tok |= 1u << k;
        else if (b == '\n') newline |= 1u << k;
        else if (b != ' ' && b != '\t' && b != '\r') bad = true;
    }
    *nl = newline;
    *ts = tok & ~((tok << 1) | (cp_is_token_byte((unsigned char)prev) ? 1u : 0u));
    return bad;
}

__global__ void __launch_bounds__(256)
cp_count_kernel(const char *__restrict__ text, uint64_t n, uint64_t n_seg, uint32_t *__restrict__ seg_nl, uint32_t *__restrict__ seg_ts,
                uint32_t *__restrict__ flags) {
    const uint64_t seg = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= n_seg) return;   // (wave-uniform)
    uint32_t nl, ts;
    const bool bad = cp_lane_bytes(text, n, seg * CP_SEG + (uint64_t)lane_id() * 16, &nl, &ts);
    const uint32_t n_nl = wave_sum_u32((uint32_t)__popc(nl)), n_ts = wave_sum_u32((uint32_t)__popc(ts));
    if (lane_id() == 0) {
        seg_nl[seg] = n_nl;
        seg_ts[seg] = n_ts;
    }
    if (bad) atomicOr(&flags[0], 1u);
}

// ---- 2. every token start its offset and line, every line its first token -----------------------------------------------------
// nl_rank / ts_rank: exclusive scans of seg_nl / seg_ts.  tok_off, tok_line: uint32[n_tok].  line_first: uint32[n_newlines + 2];
// line_first[k + 1] = the token starts in front of newline k, line_first[0] = 0, line_first[n_newlines + 1] = n_tok (the end of
// a last line without a newline; behind a final newline it repeats line_first[n_newlines]).
__global__ void __launch_bounds__(256)
cp_place_kernel(const char *__restrict__ text, uint64_t n, uint64_t n_seg, const uint32_t *__restrict__ nl_rank,
                const uint32_t *__restrict__ ts_rank, uint64_t n_newlines, uint64_t n_tok, uint32_t *__restrict__ tok_off,
                uint32_t *__restrict__ tok_line, uint32_t *__restrict__ line_first) {
    const uint64_t seg = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= n_seg) return;
    const uint64_t first = seg * CP_SEG + (uint64_t)lane_id() * 16;
    uint32_t nl, ts;
    (void)cp_lane_bytes(text, n, first, &nl, &ts);
    const uint32_t my_nl = (uint32_t)__popc(nl), my_ts = (uint32_t)__popc(ts);
    uint64_t line = (uint64_t)nl_rank[seg] + (wave_incl_scan_u32(my_nl) - my_nl);
    uint64_t t = (uint64_t)ts_rank[seg] + (wave_incl_scan_u32(my_ts) - my_ts);
    if (seg == 0 && lane_id() == 0) {
        line_first[0] = 0u;
        line_first[n_newlines + 1] = (uint32_t)n_tok;
    }
    uint32_t both = nl | ts;   // (no byte is both)
    while (both) {
        const int k = __ffs((int)both) - 1;
        both &= both - 1;
        if (ts >> k & 1u) {
            if (t < n_tok) {   // (always: n_tok is the scan's total)
                tok_off[t] = (uint32_t)(first + k);
                tok_line[t] = (uint32_t)line;
            }
            t++;
        } else {
            line++;
            if (line <= n_newlines) line_first[line] = (uint32_t)t;   // (always)
        }
    }
}

// max_len[0] (zeroed by the caller) = the most tokens in any of the n_lines lines
__global__ void __launch_bounds__(256)
cp_width_kernel(const uint32_t *__restrict__ line_first, uint64_t n_lines, uint32_t *__restrict__ max_len) {
    const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t v = l < n_lines ? line_first[l + 1] - line_first[l] : 0u;
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, WAVE);
        if (o > v) v = o;
    }
    if (lane_id() == 0 && v) atomicMax(&max_len[0], v);
}

// ---- 3. per-token records -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cp_tokens_kernel(const char *__restrict__ text, uint64_t n, const uint32_t *__restrict__ tok_off, uint64_t n_tok, ElToken *__restrict__ tok) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_tok) return;
    const uint32_t off = tok_off[p];
    uint64_t e = off;
    while (e < n && cp_is_token_byte((unsigned char)text[e])) e++;
    const uint32_t len = (uint32_t)(e - off);
    tok[p] = ElToken{off, len, el_hash(text, off, len)};
}

// ---- 4. the matrix -----------------------------------------------------------------------------------------------------------
// rank: exclusive scan of first[].  out: uint32[n_lines, width], zeroed.  Token p -> rank[occupant of its slot] in its line's
// row at its place in the line; a first appearance also names its number.
__global__ void __launch_bounds__(256)
cp_fill_kernel(const ElToken *__restrict__ tok, const uint32_t *__restrict__ table, const uint32_t *__restrict__ slot_of,
               const uint32_t *__restrict__ rank, const uint32_t *__restrict__ tok_line, const uint32_t *__restrict__ line_first,
               uint64_t n_tok, uint64_t n_names, uint64_t n_lines, uint32_t width, uint32_t *__restrict__ out,
               uint32_t *__restrict__ name_off, uint32_t *__restrict__ name_len, uint32_t *__restrict__ flags) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_tok) return;
    const uint32_t rep = table[slot_of[p]];
    if (rep > p) { atomicOr(&flags[0], 4u); return; }   // (cannot happen: the slot holds the minimum over its tokens)
    const uint32_t v = rank[rep];
    if (v >= n_names) { atomicOr(&flags[0], 4u); return; }   // (cannot happen: n_names is the scan's total)
    const uint64_t line = tok_line[p];
    if (line >= n_lines || line_first[line] > p) { atomicOr(&flags[0], 4u); return; }   // (cannot happen: a token's line holds it)
    const uint64_t col = p - line_first[line];
    if (col < (uint64_t)width - 1) out[line * width + col] = v;   // (always: width - 1 is the longest line)
    if (rep == (uint32_t)p) {
        name_off[v] = tok[p].off;
        name_len[v] = tok[p].len;
    }
}

__global__ void __launch_bounds__(256)
cp_lengths_kernel(const uint32_t *__restrict__ line_first, uint64_t n_lines, uint32_t width, uint32_t *__restrict__ out) {
    const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (l < n_lines) out[l * width + (width - 1)] = line_first[l + 1] - line_first[l];
}

}  // namespace pw
#endif
