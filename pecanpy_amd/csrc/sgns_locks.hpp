// sgns_locks.hpp -- the size arithmetic of a skip-gram session's lock bits (pw_sgns_set_locks / pw_sgns_get_locks).  Host code
// only, no runtime call: tools/sgns_locks_check.cpp drives it under the host sanitizers.
//
// Row r of a matrix is bit r % 32 of word r / 32.  The packing kernel (sgns.hip.h: sgns_lock_pack_kernel) gives a wavefront 64
// rows and lets it store two words, so the array holds a whole number of word PAIRS; the launch covers the rows with
// workgroups of SGNS_LOCK_THREADS threads.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pw {

constexpr unsigned SGNS_LOCK_THREADS = 256;   // (a multiple of 64: a wavefront's 64 rows start at a multiple of 64)

// words of the bit array of n_rows rows: 2 * ceil(n_rows / 64); 0 rows -> 0 words
inline size_t sgns_lock_words(uint32_t n_rows) { return 2 * (((size_t)n_rows + 63) / 64); }
// workgroups of the pack / unpack launch over n_rows rows (n_rows < 2^32: fits an unsigned)
inline unsigned sgns_lock_blocks(uint32_t n_rows) { return (unsigned)(((uint64_t)n_rows + SGNS_LOCK_THREADS - 1) / SGNS_LOCK_THREADS); }
// the first of the two words the wavefront of thread `r` stores, or SIZE_MAX when that wavefront stores nothing (all of its
// rows lie beyond n_rows): what the kernel computes, restated for the host check that every store lands inside the array
inline size_t sgns_lock_first_word(uint64_t r, uint32_t n_rows) { return (r & ~63ull) < n_rows ? (size_t)((r & ~63ull) >> 5) : SIZE_MAX; }

}  // namespace pw
