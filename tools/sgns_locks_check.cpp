// sgns_locks_check.cpp -- the host-side size arithmetic of the skip-gram lock bits (pecanpy_amd/csrc/sgns_locks.hpp) driven on the
// CPU, for a build with the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipecanpy_amd/csrc tools/sgns_locks_check.cpp -o sgns_locks_check
//   ./sgns_locks_check
// For every row count of interest it allocates exactly sgns_lock_words(n) words and n mask bytes on the heap, walks the launch
// the driver makes (sgns_lock_blocks(n) workgroups of SGNS_LOCK_THREADS threads) thread by thread, and does what the packing
// kernel does with the indices sgns_lock_first_word names: a read of mask[r] for r < n, two word stores per wavefront that has
// a row.  An index outside either array is an AddressSanitizer report; an overflow in the arithmetic an UBSan report.  Then the
// bits are checked against the mask, the bits at and beyond n must be zero, and the unpacking must give the mask back.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sgns_locks.hpp"

static int check(uint32_t n, bool simulate) {
    const size_t words = pw::sgns_lock_words(n);
    const unsigned blocks = pw::sgns_lock_blocks(n);
    if (words != 2 * (((uint64_t)n + 63) / 64)) return 1;
    if ((uint64_t)blocks * pw::SGNS_LOCK_THREADS < n || (blocks && (uint64_t)(blocks - 1) * pw::SGNS_LOCK_THREADS >= n)) return 2;
    if (words * 32 < n || (uint64_t)words * 32 >= (uint64_t)n + 64) return 3;   // every row has a bit, less than one pair to spare
    if (!simulate) return 0;
    uint8_t *mask = (uint8_t *)malloc(n ? n : 1);
    uint32_t *w = (uint32_t *)malloc(words ? words * sizeof(uint32_t) : 1);
    if (!mask || !w) return 4;
    for (uint32_t r = 0; r < n; r++) mask[r] = (uint8_t)((r * 2654435761u >> 28) < 5 ? 1 + r % 255 : 0);
    for (size_t i = 0; i < words; i++) w[i] = 0xdeadbeefu;
    unsigned long long n_set = 0, want_set = 0;
    for (uint64_t base = 0; base < (uint64_t)blocks * pw::SGNS_LOCK_THREADS; base += 64) {   // one wavefront
        uint64_t ballot = 0;
        for (uint64_t r = base; r < base + 64; r++)
            if (r < n && mask[r] != 0) ballot |= 1ull << (r - base);
        const size_t first = pw::sgns_lock_first_word(base + 17, n);                        // (any thread of the wavefront)
        if (first != pw::sgns_lock_first_word(base, n)) return 5;
        if (first == SIZE_MAX) continue;
        w[first] = (uint32_t)ballot;
        w[first + 1] = (uint32_t)(ballot >> 32);
        n_set += (unsigned long long)__builtin_popcountll(ballot);
    }
    int rc = 0;
    for (uint64_t r = 0; r < (uint64_t)words * 32; r++) {
        const unsigned bit = w[r >> 5] >> (r & 31) & 1u;
        const unsigned want = r < n && mask[r] != 0;
        want_set += want;
        if (bit != want) rc = 6;
    }
    if (n_set != want_set) rc = 7;
    free(mask);
    free(w);
    return rc;
}

int main() {
    const uint32_t simulated[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 4095, 4097, 100003, 1u << 20};
    for (uint32_t n : simulated)
        if (int rc = check(n, true)) { printf("FAILED: n_rows = %u, check %d\n", n, rc); return 1; }
    const uint32_t arithmetic[] = {(1u << 31) - 1, 1u << 31, (1u << 31) + 1, 0xffffffc0u, 0xffffffc1u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t n : arithmetic)
        if (int rc = check(n, false)) { printf("FAILED: n_rows = %u, check %d\n", n, rc); return 1; }
    printf("sgns lock arithmetic OK: %zu simulated launches, %zu sizes up to 2^32 - 1\n", sizeof(simulated) / sizeof(*simulated),
           sizeof(arithmetic) / sizeof(*arithmetic));
    return 0;
}
