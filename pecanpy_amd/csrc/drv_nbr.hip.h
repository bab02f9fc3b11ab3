#pragma once
// Host driver, neighbourhood link-prediction baselines (nbr_scores.hip.h): the degrees without the loop and the scores of given
// pairs on a CSR handle.  Exports pw_nbr_degrees_device, pw_nbr_scores_device, pw_nbr_scores_device_cut, pw_selftest_nbr_scores, pw_selftest_nbr_degrees.
// Stands on the core, on drv_pairs (the range check of the pairs) and on the public pw_csr_create alone.
#include "drv_core.hip.h"
#include "drv_pairs.hip.h"
#include "nbr_scores.hip.h"

namespace {

int nbr_check_kind(int kind, const void *table) {
    if (kind < 0 || kind >= pw::NBR_KINDS)
        return fail(PW_ERR_INVALID, "pw_nbr_scores: kind " + std::to_string(kind) + " is none of PW_NBR_COMMON, PW_NBR_JACCARD, PW_NBR_PREF, PW_NBR_WEIGHTED");
    if (kind == pw::NBR_WEIGHTED && !table) return fail(PW_ERR_INVALID, "pw_nbr_scores: PW_NBR_WEIGHTED needs a table");
    return 0;
}
int nbr_need_csr(const pw_graph *g, const char *what) {
    return g->gd->kind != 0 ? fail(PW_ERR_UNSUPPORTED, std::string(what) + " needs a CSR graph handle") : 0;
}

int nbr_degrees_impl(pw_graph *g, uint32_t *d_deg) {
    if (!g || !d_deg) return fail(PW_ERR_INVALID, "null pointer");
    if (int rc = nbr_need_csr(g, "pw_nbr_degrees")) return rc;
    if (set_device(g)) return PW_ERR_HIP;
    const uint32_t n_nodes = g->gd->n_nodes;
    hipLaunchKernelGGL(pw::nbr_degrees_kernel, dim3(strided_grid(n_nodes, g->n_cu)), dim3(256), 0, g->stream, (const uint32_t *)g->gd->d_indptr.p,
                       (const uint32_t *)g->gd->d_indices.p, n_nodes, d_deg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PW_OK;
}

int nbr_check_cut(int64_t short_max) {
    return short_max < -1 || short_max > (int64_t)pw::NBR_ALL_LANE ? fail(PW_ERR_INVALID, "pw_nbr_scores: short_max must be -1 or in 0 .. 2^32 - 1") : 0;
}

// short_max: the cut between the lane form and the wavefront form (-1: pw::NBR_SHORT_MAX).  No result depends on it.
// kernel_ms (may be null): the device time of the score kernel alone, between two events.
int nbr_scores_impl(pw_graph *g, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int kind, const double *d_table, double *d_score,
                    int64_t short_max, float *kernel_ms) {
    if (!g) return fail(PW_ERR_INVALID, "null pointer");
    int rc;
    if ((rc = nbr_need_csr(g, "pw_nbr_scores")) || (rc = nbr_check_kind(kind, d_table)) || (rc = nbr_check_cut(short_max))) return rc;
    if (kernel_ms) *kernel_ms = 0.f;
    if (m == 0) return PW_OK;
    if (!d_u || !d_v || !d_score) return fail(PW_ERR_INVALID, "null pointer");
    if (set_device(g)) return PW_ERR_HIP;
    const uint32_t n_nodes = g->gd->n_nodes;
    if ((rc = check_pairs(g->stream, g->n_cu, d_u, d_v, m, n_nodes, n_nodes, "pw_nbr_scores"))) return rc;
    pw::NbrArgs a;
    a.indptr = g->gd->d_indptr.p; a.indices = g->gd->d_indices.p;
    a.table = kind == pw::NBR_WEIGHTED ? d_table : nullptr;
    a.u = d_u; a.v = d_v; a.score = d_score;
    a.m = m; a.n_tiles = (m + 63) / 64;
    a.kind = (uint32_t)kind; a.short_max = short_max < 0 ? pw::NBR_SHORT_MAX : (uint32_t)short_max;
    uint64_t blocks = 0;
    if ((rc = persistent_tile_grid((const void *)pw::nbr_scores_kernel, (int)pw::NBR_THREADS, pw::NBR_WAVES, a.n_tiles, g->n_cu, 0, &blocks))) return rc;
    pw::Event ev[2];
    if (kernel_ms) {
        for (auto &e : ev) HIP_TRY(e.create(hipEventDefault));
        HIP_TRY(hipEventRecord(ev[0], g->stream));
    }
    hipLaunchKernelGGL(pw::nbr_scores_kernel, dim3((unsigned)blocks), dim3(pw::NBR_THREADS), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) HIP_TRY(hipEventRecord(ev[1], g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, ev[0], ev[1]));
    return PW_OK;
}

int nbr_check_csr_host(const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes) {
    if (!indptr || n_nodes == 0 || (indptr[n_nodes] && !indices)) return fail(PW_ERR_INVALID, "null pointer");
    return 0;
}

}  // namespace

PW_EXPORT int pw_nbr_degrees_device(pw_graph *g, uint32_t *d_deg) { return nbr_degrees_impl(g, d_deg); }

PW_EXPORT int pw_nbr_scores_device(pw_graph *g, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int kind, const double *d_table, double *d_score) {
    return nbr_scores_impl(g, d_u, d_v, m, kind, d_table, d_score, -1, nullptr);
}

PW_EXPORT int pw_nbr_scores_device_cut(pw_graph *g, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int kind, const double *d_table,
                                       double *d_score, int64_t short_max, float *kernel_ms) {
    return nbr_scores_impl(g, d_u, d_v, m, kind, d_table, d_score, short_max, kernel_ms);
}

PW_EXPORT int pw_selftest_nbr_degrees(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, uint32_t *deg) {
    if (int rc = nbr_check_csr_host(indptr, indices, n_nodes)) return rc;
    if (!deg) return fail(PW_ERR_INVALID, "null pointer");
    if (!on_device) {
        pw::nbr_host_degrees(indptr, indices, n_nodes, deg);
        return PW_OK;
    }
    pw_graph *raw = nullptr;
    int rc;
    if ((rc = pw_csr_create(indptr, indices, nullptr, n_nodes, indptr[n_nodes], device, &raw))) return rc;
    GraphOwner g(raw);   // (declared before the buffer: it goes first)
    DevBuf<uint32_t> d_deg;
    if ((rc = dev_alloc(d_deg, n_nodes)) || (rc = nbr_degrees_impl(g.get(), d_deg.p))) return rc;
    return download(deg, d_deg, n_nodes);
}

PW_EXPORT int pw_selftest_nbr_scores(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, const uint32_t *u,
                                     const uint32_t *v, uint64_t m, int kind, const double *table, int64_t short_max, double *score) {
    int rc;
    if ((rc = nbr_check_csr_host(indptr, indices, n_nodes))) return rc;
    if (m && (!u || !v || !score)) return fail(PW_ERR_INVALID, "null pointer");
    if ((rc = nbr_check_kind(kind, table))) return rc;
    if ((rc = nbr_check_cut(short_max))) return rc;
    if (!on_device) {
        std::vector<double> sc(m);   // (a refused call writes nothing)
        uint64_t where = 0;
        switch (pw::nbr_host_scores(indptr, indices, n_nodes, u, v, m, kind, table, sc.data(), &where)) {
            case pw::LP_HOST_U_RANGE: return pair_range("pw_nbr_scores", "u", where, u[where], n_nodes);
            case pw::LP_HOST_V_RANGE: return pair_range("pw_nbr_scores", "v", where, v[where], n_nodes);
            default: break;
        }
        if (m) memcpy(score, sc.data(), sizeof(double) * m);
        return PW_OK;
    }
    pw_graph *raw = nullptr;
    if ((rc = pw_csr_create(indptr, indices, nullptr, n_nodes, indptr[n_nodes], device, &raw))) return rc;
    GraphOwner g(raw);   // (declared before the buffers: they go first)
    if (m == 0) return PW_OK;
    DevBuf<uint32_t> d_u, d_v;
    DevBuf<double> d_table, d_score;
    if ((rc = upload(d_u, u, m)) || (rc = upload(d_v, v, m)) || (rc = dev_alloc(d_score, m))) return rc;
    if (kind == pw::NBR_WEIGHTED && (rc = upload(d_table, table, n_nodes))) return rc;
    if ((rc = nbr_scores_impl(g.get(), d_u.p, d_v.p, m, kind, d_table.p, d_score.p, short_max, nullptr))) return rc;
    return download(score, d_score, m);
}
