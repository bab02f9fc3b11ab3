// edgelist_dev.hip.h -- an edge-list FILE parsed in device memory (gfx950): pw_edgelist_read_device.
//
// The text of the file -> (src, dst, float64 weight) per line with the reference's first-appearance vertex numbering
// (AdjlstGraph.read, graph.py:218-304), ready for the COO -> CSR build of coo_csr.hip.h.  The reader is optimistic the way
// edgelist.hpp is: it accepts a SUBSET of what read_edgelist accepts and raises a decline flag for everything else; the
// caller then reports "needs the host reader", which is no error.
//
//   1. el_count_kernel      one wavefront per 1024-byte segment, 16 bytes per lane: rejects the bytes read_edgelist rejects
//                           (>= 0x80, control bytes but \t \r \n, a \r without \n behind it) and counts the segment's newlines
//      scan of the counts   (scan.hip.h)
//      el_starts_kernel     the same segments again: line k + 1 starts behind newline k
//   2. el_lines_kernel      one thread per line: el_tokenize_line (strip, split(delimiter), the term-count rules, the stripped
//                           spans of id1 / id2, el_parse_weight) -> token records (offset, length, FNV-1a hash), float64 weight
//   3. el_insert_kernel     one thread per token (token 2 i = line i's id1, 2 i + 1 = its id2): open addressing over a table of
//                           token POSITIONS keyed by the string's hash.  An empty slot is claimed by compare-and-swap; on an
//                           occupied slot the token compares its bytes with the occupant's: equal -> atomicMin(slot, own
//                           position), different -> next slot.  Nothing is ever deleted.
//      el_first_kernel      first[p] = the slot of token p holds p; its exclusive scan is the vertex number
//      el_number_kernel     every token -> the number of its slot's occupant: src / dst (int64), and the (offset, length) of
//                           every vertex's name in first-appearance order
// Determinism: every output word is a function of the text alone.  A slot that is occupied stays occupied, and by the same
// STRING for good: only tokens with equal bytes ever replace its value, and only by a smaller position.  Two tokens with equal
// strings walk the same probe sequence and see, slot for slot, either another string (for good) or a slot that ends up theirs,
// so they end in ONE slot; the minimum over all of them is that slot's final value whatever the order in which the atomics
// arrive, and it is the string's first appearance.  Which slot a string lands in does depend on the arrival order -- nothing
// downstream reads a slot number: vertex numbers are ranks of first appearances in token order.  The flags are atomicOr /
// atomicMin of values that are functions of the text.
//
// el_parse_weight accepts exactly the literals whose float64 value one IEEE operation gives correctly rounded (Clinger's fast
// path): [+-]digits[.digits][e[+-]digits] whose significand without its leading zeros has at most 15 digits (an integer
// below 10^15 < 2^53: exact) and whose power of ten, the fraction digits taken off the exponent, lies in [-22, 22] (10^22 is
// exact in float64): the value is that integer times or divided by that power, ONE correctly rounded operation under
// -fno-fast-math -ffp-contract=off -- what strtod / Python's float() return.  Everything else is declined.
// One text serves the device kernels and the host (pw_selftest_edgelist_weight / pw_selftest_edgelist_line).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PW_EL_HD __host__ __device__ __forceinline__
#else
#define PW_EL_HD inline
#endif

namespace pw {

constexpr uint32_t EL_EMPTY = 0xffffffffu;    // a free slot of the id table
constexpr int EL_SEG = 1024;                  // bytes per wavefront in the byte passes (16 per lane)
constexpr uint32_t EL_MAX_DELIM = 16;         // delimiter bytes the line kernel takes (longer ones: the host reader)

struct ElLine {
    uint32_t n_terms;        // len(line.strip().split(delimiter))
    uint32_t off[3], len[3]; // the first three terms (unstripped), offsets into the text
    uint32_t id_off[2], id_len[2];   // terms[0].strip(), terms[1].strip()
    double weight;           // 1.0 when unweighted
};

PW_EL_HD bool el_is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// 10^k, 0 <= k <= 22: exact float64 values
PW_EL_HD double el_pow10(int k) {
    switch (k) {
    case 0: return 1e0; case 1: return 1e1; case 2: return 1e2; case 3: return 1e3; case 4: return 1e4; case 5: return 1e5;
    case 6: return 1e6; case 7: return 1e7; case 8: return 1e8; case 9: return 1e9; case 10: return 1e10; case 11: return 1e11;
    case 12: return 1e12; case 13: return 1e13; case 14: return 1e14; case 15: return 1e15; case 16: return 1e16;
    case 17: return 1e17; case 18: return 1e18; case 19: return 1e19; case 20: return 1e20; case 21: return 1e21;
    default: return 1e22;
    }
}

// The float64 value of text[0, n) after strip(), when the literal is in the class of the header; false: declined.  The sign
// is applied to the value (so "-0" is -0.0): the caller declines what is not > 0.
PW_EL_HD bool el_parse_weight(const char *t, uint32_t n, double *w) {
    while (n && el_is_space(t[0])) { t++; n--; }
    while (n && el_is_space(t[n - 1])) n--;
    if (n == 0 || n > 63) return false;   // (read_edgelist's own length limit)
    uint32_t i = 0;
    bool neg = false;
    if (t[i] == '+' || t[i] == '-') { neg = t[i] == '-'; i++; }
    uint64_t m = 0;              // the significand's digits as an integer
    uint32_t sig = 0, any = 0;   // digits behind the leading zeros; digits at all
    int frac = 0;                // digits behind the point
    for (; i < n && t[i] >= '0' && t[i] <= '9'; i++, any++)
        if (sig || t[i] != '0') {
            if (++sig > 15) return false;
            m = m * 10 + (uint64_t)(t[i] - '0');
        }
    if (i < n && t[i] == '.') {
        for (i++; i < n && t[i] >= '0' && t[i] <= '9'; i++, any++, frac++)
            if (sig || t[i] != '0') {
                if (++sig > 15) return false;
                m = m * 10 + (uint64_t)(t[i] - '0');
            }
    }
    if (any == 0) return false;
    int ex = 0;
    if (i < n && (t[i] == 'e' || t[i] == 'E')) {
        i++;
        bool eneg = false;
        if (i < n && (t[i] == '+' || t[i] == '-')) { eneg = t[i] == '-'; i++; }
        uint32_t ed = 0;
        for (; i < n && t[i] >= '0' && t[i] <= '9'; i++, ed++)
            if (ex < 1000) ex = ex * 10 + (t[i] - '0');   // (saturates: anything this large is declined below)
        if (ed == 0) return false;
        if (eneg) ex = -ex;
    }
    if (i != n) return false;
    const int p = ex - frac;   // value = m * 10^p
    if (p < -22 || p > 22) return false;
    const double v = p >= 0 ? (double)m * el_pow10(p) : (double)m / el_pow10(-p);
    *w = neg ? -v : v;
    return true;
}

// text[lo, hi) = one line without its '\n': strip(), split(delim), the term-count rules of AdjlstGraph._read_edge_line,
// the stripped ids, the weight.  false: the line needs the host reader (fewer than two terms, a weighted line without exactly
// three, a weight literal outside el_parse_weight's class, a weight <= 0).
PW_EL_HD bool el_tokenize_line(const char *text, uint64_t lo, uint64_t hi, const char *delim, uint32_t dl, bool weighted, ElLine *out) {
    while (lo < hi && el_is_space(text[lo])) lo++;
    while (hi > lo && el_is_space(text[hi - 1])) hi--;
    uint32_t n_terms = 0;
    uint64_t a = lo;
    for (;;) {
        uint64_t b = a;
        bool found = false;
        for (; b + dl <= hi; b++) {
            uint32_t k = 0;
            while (k < dl && text[b + k] == delim[k]) k++;
            if (k == dl) { found = true; break; }
        }
        if (!found) b = hi;
        if (n_terms < 3) { out->off[n_terms] = (uint32_t)a; out->len[n_terms] = (uint32_t)(b - a); }
        n_terms++;
        if (!found) break;
        a = b + dl;
    }
    out->n_terms = n_terms;
    out->weight = 1.0;
    if (n_terms < 2) return false;              // IndexError in the reference
    if (weighted && n_terms != 3) return false;   // ValueError in the reference
    for (int k = 0; k < 2; k++) {
        uint64_t s = out->off[k], e = s + out->len[k];
        while (s < e && el_is_space(text[s])) s++;
        while (e > s && el_is_space(text[e - 1])) e--;
        out->id_off[k] = (uint32_t)s;
        out->id_len[k] = (uint32_t)(e - s);
    }
    if (weighted) {
        if (!el_parse_weight(text + out->off[2], out->len[2], &out->weight)) return false;
        if (!(out->weight > 0.0)) return false;   // the reference warns ("Non-positive edge ignored")
    }
    return true;
}

PW_EL_HD uint32_t el_hash(const char *text, uint32_t off, uint32_t len) {   // FNV-1a, 64 bit, folded
    uint64_t h = 1469598103934665603ull;
    for (uint32_t i = 0; i < len; i++) h = (h ^ (unsigned char)text[off + i]) * 1099511628211ull;
    return (uint32_t)(h ^ (h >> 32));
}

}  // namespace pw

#if defined(__HIPCC__)
#include "wave.h"

namespace pw {

struct ElToken { uint32_t off, len, hash; };

// flags[0]: a byte or a line the reader does not take (any non-zero value)
// ---- 1. byte classes, newline counts, line starts -------------------------------------------------------------------------
// the 16 bytes of this lane: newline mask (bit k = byte k is '\n'); bad = a byte read_edgelist declines on
__device__ __forceinline__ uint32_t el_lane_bytes(const char *__restrict__ text, uint64_t n, uint64_t first, bool *bad) {
    uint32_t nl = 0;
    *bad = false;
    if (first >= n) return 0;
    unsigned char c[17];
    if (first + 17 <= n) {
        const uint4 v = *(const uint4 *)(text + first);   // (first is a multiple of 16, the buffer comes from hipMalloc)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < 16; k++) c[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
        c[16] = (unsigned char)text[first + 16];
    } else {
        for (int k = 0; k < 17; k++) c[k] = first + k < n ? (unsigned char)text[first + k] : (unsigned char)0;   // (0 behind the end: no '\n')
    }
    const int valid = first + 16 <= n ? 16 : (int)(n - first);
    for (int k = 0; k < 16; k++) {
        if (k >= valid) break;
        const unsigned char b = c[k];
        if (b == '\n') nl |= 1u << k;
        else if (b >= 0x80 || (b < 0x20 && b != '\t' && b != '\r')) *bad = true;
        else if (b == '\r' && c[k + 1] != '\n') *bad = true;   // a lone CR is a newline to Python's text layer
    }
    return nl;
}

__global__ void __launch_bounds__(256)
el_count_kernel(const char *__restrict__ text, uint64_t n, uint64_t n_seg, uint32_t *__restrict__ seg_count, uint32_t *__restrict__ flags) {
    const uint64_t seg = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= n_seg) return;
    bool bad;
    const uint32_t nl = el_lane_bytes(text, n, seg * EL_SEG + (uint64_t)lane_id() * 16, &bad);
    const uint32_t total = wave_sum_u32((uint32_t)__popc(nl));
    if (lane_id() == 0) seg_count[seg] = total;
    if (bad) atomicOr(&flags[0], 1u);
}

// seg_rank: exclusive scan of seg_count.  starts[0] = 0 is the caller's; starts[k + 1] = position behind newline k.
__global__ void __launch_bounds__(256)
el_starts_kernel(const char *__restrict__ text, uint64_t n, uint64_t n_seg, const uint32_t *__restrict__ seg_rank, uint64_t n_starts,
                 uint32_t *__restrict__ starts) {
    const uint64_t seg = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= n_seg) return;
    bool bad;
    const uint64_t first = seg * EL_SEG + (uint64_t)lane_id() * 16;
    uint32_t nl = el_lane_bytes(text, n, first, &bad);
    const uint32_t mine = (uint32_t)__popc(nl);
    uint64_t k = (uint64_t)seg_rank[seg] + (wave_incl_scan_u32(mine) - mine) + 1;
    while (nl) {
        const int b = __ffs((int)nl) - 1;
        nl &= nl - 1;
        if (k < n_starts) starts[k] = (uint32_t)(first + b + 1);   // (always: n_starts = newlines + 1)
        k++;
    }
}

// ---- 2. per-line records ---------------------------------------------------------------------------------------------------
// line i = text[starts[i], starts[i + 1] - 1): up to its newline; a last line without one (i + 1 == n_starts) ends at n
__global__ void __launch_bounds__(256)
el_lines_kernel(const char *__restrict__ text, uint64_t n, const uint32_t *__restrict__ starts, uint64_t n_starts, uint64_t n_lines,
                const char *__restrict__ delim, uint32_t dl, int weighted, ElToken *__restrict__ tok, double *__restrict__ w64,
                uint32_t *__restrict__ flags) {
    __shared__ char d[EL_MAX_DELIM];
    if (threadIdx.x < dl) d[threadIdx.x] = delim[threadIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_lines) return;
    const uint64_t lo = starts[i], hi = i + 1 < n_starts ? (uint64_t)starts[i + 1] - 1 : n;
    ElLine ln;
    const bool ok = lo <= hi && hi <= n && el_tokenize_line(text, lo, hi, d, dl, weighted != 0, &ln);
    if (!ok) {
        atomicOr(&flags[0], 2u);
        tok[2 * i] = ElToken{0u, 0u, 0u};
        tok[2 * i + 1] = ElToken{0u, 0u, 0u};
        if (w64) w64[i] = 1.0;
        return;
    }
    for (int k = 0; k < 2; k++) tok[2 * i + k] = ElToken{ln.id_off[k], ln.id_len[k], el_hash(text, ln.id_off[k], ln.id_len[k])};
    if (w64) w64[i] = ln.weight;
}

// ---- 3. first-appearance numbering -------------------------------------------------------------------------------------------
__device__ __forceinline__ bool el_same_string(const char *__restrict__ text, const ElToken &a, const ElToken &b) {
    if (a.len != b.len || a.hash != b.hash) return false;
    if (a.off == b.off) return true;
    for (uint32_t i = 0; i < a.len; i++)
        if (text[a.off + i] != text[b.off + i]) return false;
    return true;
}

// table: uint32[mask + 1], all EL_EMPTY; mask + 1 a power of two >= 2 n_tok (so a free slot always exists)
__global__ void __launch_bounds__(256)
el_insert_kernel(const char *__restrict__ text, const ElToken *__restrict__ tok, uint64_t n_tok, uint32_t *table, uint32_t mask,
                 uint32_t *__restrict__ slot_of) {
    const uint64_t p64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p64 >= n_tok) return;
    const uint32_t p = (uint32_t)p64;
    const ElToken me = tok[p];
    uint32_t slot = me.hash & mask;
    for (uint32_t probes = 0; probes <= mask; probes++, slot = (slot + 1) & mask) {
        uint32_t cur = __atomic_load_n(&table[slot], __ATOMIC_RELAXED);
        if (cur == EL_EMPTY) {
            cur = atomicCAS(&table[slot], EL_EMPTY, p);
            if (cur == EL_EMPTY) break;   // claimed
        }
        // occupied, by a string that stays: a stale value read above is an earlier occupant with the same bytes
        if (cur < n_tok && el_same_string(text, me, tok[cur])) {
            if (p < cur) atomicMin(&table[slot], p);   // (a value below p already: the minimum cannot be p)
            break;
        }
    }
    slot_of[p] = slot;
}

__global__ void __launch_bounds__(256)
el_first_kernel(const uint32_t *__restrict__ table, const uint32_t *__restrict__ slot_of, uint64_t n_tok, uint32_t *__restrict__ first) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n_tok) first[p] = table[slot_of[p]] == (uint32_t)p ? 1u : 0u;
    else if (p == n_tok) first[p] = 0u;   // the scan's total
}

// rank: exclusive scan of first[].  Token p -> rank[occupant of its slot]; a first appearance also names its vertex.
__global__ void __launch_bounds__(256)
el_number_kernel(const ElToken *__restrict__ tok, const uint32_t *__restrict__ table, const uint32_t *__restrict__ slot_of,
                 const uint32_t *__restrict__ rank, uint64_t n_tok, uint64_t n_nodes, int64_t *__restrict__ src, int64_t *__restrict__ dst,
                 uint32_t *__restrict__ id_off, uint32_t *__restrict__ id_len, uint32_t *__restrict__ flags) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_tok) return;
    const uint32_t rep = table[slot_of[p]];
    if (rep > p) { atomicOr(&flags[0], 4u); return; }   // (cannot happen: the slot holds the minimum over its tokens)
    const uint32_t v = rank[rep];
    if (v >= n_nodes) { atomicOr(&flags[0], 4u); return; }   // (cannot happen: n_nodes is the scan's total)
    ((p & 1) ? dst : src)[p >> 1] = (int64_t)v;
    if (rep == (uint32_t)p) {
        id_off[v] = tok[p].off;
        id_len[v] = tok[p].len;
    }
}

}  // namespace pw
#endif
