// counters.h -- layout of pw_graph::counters, the per-context array of device counters (unsigned long long each).
// The host addresses it by CTR_* (counters.p + CTR_X); a kernel is handed `stats` = counters + CTR_STATS and addresses
// the same slots by ST_* = CTR_* - CTR_STATS.
#pragma once

namespace pw {

enum : int {
    CTR_JOB = 0,            // job counter of the running kernel (work distribution); one-word flag of the dense value checks
    CTR_STATS = 1,          // `stats` of every walk kernel: [1] steps [2] overflow reads [3] clamped reads [4] dead-end walks
    CTR_STEPS = 1,
    CTR_OVERFLOW = 2,
    CTR_CLAMPED = 3,
    CTR_DEAD = 4,
    CTR_CHANGED = 5,        // compute_offsets: jobs whose stream offset changed
    CTR_REDO = 6,           // jobs a lane / dense fast kernel handed back (entries of the redo list)
    CTR_LIST_READS = 7,     // list entries read by the lane kernel
    CTR_AMBIGUOUS = 8,      // steps the lane kernel's a-priori bound left open; steps decided by the float64 chain (node2vec++)
    CTR_BAD_START = 9,      // check_starts: first job whose start is not a vertex (~0: none)
    CTR_WAVE_CHAIN = 10,    // of the ambiguous steps, those that needed the float32 chain (the per-lane chain's rounding ties)
    CTR_EAGER = 12,         // `stats` of the eager kernels: steps they decided
    CTR_EAGER_NEXT = 13,    // record counter of the eager kernels' persistent grid (zeroed before each launch)
    CTR_FIRST_CHANGED = 14, // compute_offsets: first job whose stream offset changed (~0: none)
    CTR_REWALK_STATS = 20,  // `stats` of the re-walks behind a verification mismatch ([20..23]: counted by the lane kernel already)
    CTR_PARKED = 32,        // parked walks (lane kernel's chain queue; a cache line of its own)
    CTR_VER = 40,           // records the lane kernel appended; full verification: [40..43] lanes_verify_kernel's counts per round
    CTR_VER_SAMPLE = 44,    // [44..47] lanes_verify_kernel's counts: sampled verification, FLOATS form
    N_COUNTERS = 48,
};

// lanes_verify_kernel's four counts, from CTR_VER / CTR_VER_SAMPLE
enum : int { VER_CHECKED = 0, VER_MISMATCH = 1, VER_TIES = 2, VER_BAD = 3, N_VER_COUNTS = 4 };

// the same slots as a kernel sees them, relative to its `stats` pointer
enum : int {
    ST_STEPS = CTR_STEPS - CTR_STATS,
    ST_OVERFLOW = CTR_OVERFLOW - CTR_STATS,
    ST_CLAMPED = CTR_CLAMPED - CTR_STATS,
    ST_DEAD = CTR_DEAD - CTR_STATS,
    ST_LIST_READS = CTR_LIST_READS - CTR_STATS,
    ST_AMBIGUOUS = CTR_AMBIGUOUS - CTR_STATS,
    ST_WAVE_CHAIN = CTR_WAVE_CHAIN - CTR_STATS,
};

}  // namespace pw
