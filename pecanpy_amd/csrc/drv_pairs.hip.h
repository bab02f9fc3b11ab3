#pragma once
// Host driver, pairs of row numbers (u[i], v[i]): the one text of a row number out of range (pw_logit_eval's own kernel reports
// through it too) and the one range check over lp_check_pairs_kernel (linkpred.hip.h).  No exports.  Stands on the core.
#include "drv_core.hip.h"
#include "linkpred.hip.h"

namespace {

int pair_range(const char *entry, const char *which, uint64_t i, uint32_t row, uint64_t n) {
    return fail(PW_ERR_INVALID, std::string(entry) + ": row number " + which + "[" + std::to_string(i) + "] = " + std::to_string(row) +
                                    " is outside the " + std::to_string(n) + " rows");
}

// u[i] < n_u and v[i] < n_v for every i < m, or the first pair that fails refused in `entry`'s name.  Runs on `stream` and
// waits for it: the null stream for the callers that hold pw_knn indexes, the handle's stream for those that hold a graph.
int check_pairs(hipStream_t stream, int n_cu, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, uint64_t n_u, uint64_t n_v, const char *entry) {
    DevBuf<pw::LpFound> found;
    if (int rc = dev_alloc(found, 1)) return rc;
    HIP_TRY(hipMemsetAsync(found.p, 0xff, sizeof(pw::LpFound), stream));
    hipLaunchKernelGGL(pw::lp_check_pairs_kernel, dim3(strided_grid(m, n_cu)), dim3(256), 0, stream, d_u, d_v, m, n_u, n_v, found.p);
    HIP_TRY(hipGetLastError());
    pw::LpFound h;
    HIP_TRY(hipMemcpyAsync(&h, found.p, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h.first == ~0ull) return 0;
    uint32_t ru = 0, rv = 0;
    HIP_TRY(hipMemcpy(&ru, d_u + h.first, sizeof(ru), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&rv, d_v + h.first, sizeof(rv), hipMemcpyDeviceToHost));
    return ru >= n_u ? pair_range(entry, "u", h.first, ru, n_u) : pair_range(entry, "v", h.first, rv, n_v);
}

}  // namespace
