#pragma once
// Host driver, host-only ingestion: the node2vec+ thresholds (thresholds.hpp; one row: dense_build.hip.h), the host edge-list
// reader (edgelist.hpp), the host emulation of seq_scan.
// Exports pw_noise_thresholds_*, pw_selftest_thresholds_row, pw_edgelist_read / _shape / _export / _destroy, pw_selftest_seqscan_*.
#include "drv_core.hip.h"
#include "edgelist.hpp"
#include "thresholds.hpp"
#include "dense_build.hip.h"

// ---- node2vec+ thresholds (host only) -----------------------------------------------------------------
PW_EXPORT int pw_noise_thresholds_csr(const uint32_t *indptr, const float *data, uint32_t n_nodes, double gamma, float *thr) {
    if (!indptr || !thr || (!data && indptr[n_nodes] != 0)) return fail(PW_ERR_INVALID, "null pointer");
    pw::noise_thresholds_csr(indptr, data, n_nodes, gamma, thr);
    return PW_OK;
}

PW_EXPORT int pw_noise_thresholds_csr_numpy1(const uint32_t *indptr, const float *data, uint32_t n_nodes, double gamma, float *thr) {
    if (!indptr || !thr || (!data && indptr[n_nodes] != 0)) return fail(PW_ERR_INVALID, "null pointer");
    pw::noise_thresholds_csr(indptr, data, n_nodes, gamma, thr, true);
    return PW_OK;
}

PW_EXPORT int pw_noise_thresholds_csr_f64(const uint32_t *indptr, const float *data, uint32_t n_nodes, double gamma, float *thr) {
    if (!indptr || !thr) return fail(PW_ERR_INVALID, "null pointer");
    pw::noise_thresholds_csr_f64(indptr, data, n_nodes, gamma, thr);
    return PW_OK;
}

PW_EXPORT int pw_noise_thresholds_dense(const double *data, uint32_t n_nodes, double gamma, float *thr) {
    if (!data || !thr) return fail(PW_ERR_INVALID, "null pointer");
    pw::noise_thresholds_dense(data, n_nodes, gamma, thr);
    return PW_OK;
}

// ---- edge-list ingestion (host only) ----------------------------------------------------------------
PW_EXPORT int pw_selftest_thresholds_row(const double *row, uint64_t n, double gamma, float *thr) {
    if ((n && !row) || !thr) return fail(PW_ERR_INVALID, "null pointer");
    *thr = pw::threshold_row([row](uint64_t i) { return row[i]; }, n, gamma);
    return PW_OK;
}

struct pw_edgelist {
    pw::EdgeList el;
};

PW_EXPORT int pw_edgelist_read(const char *path, int weighted, int directed, const char *delimiter, pw_edgelist **out) {
    if (!path || !out) return fail(PW_ERR_INVALID, "null pointer");
    *out = nullptr;
    pw_edgelist *h = new (std::nothrow) pw_edgelist();
    if (!h) return fail(PW_ERR_NOMEM, "out of host memory");
    int st;
    try {
        st = pw::read_edgelist(path, weighted != 0, directed != 0, delimiter, h->el);
    } catch (const std::bad_alloc &) {
        delete h;
        return fail(PW_ERR_NOMEM, "out of host memory while reading the edge list");
    }
    if (st == pw::EL_OK) { *out = h; return PW_OK; }
    delete h;
    if (st == pw::EL_IO_ERROR) return fail(PW_ERR_INVALID, std::string("cannot read ") + path);
    return fail(PW_ERR_UNSUPPORTED, "edge list needs the statement-by-statement reader");
}

PW_EXPORT int pw_edgelist_shape(const pw_edgelist *e, uint64_t *n_nodes, uint64_t *nnz, uint64_t *insertions,
                                uint64_t *id_bytes) {
    if (!e) return fail(PW_ERR_INVALID, "null pointer");
    if (n_nodes) *n_nodes = e->el.indptr.size() - 1;
    if (nnz) *nnz = e->el.indices.size();
    if (insertions) *insertions = e->el.insertions;
    if (id_bytes) *id_bytes = e->el.id_chars.size();
    return PW_OK;
}

PW_EXPORT int pw_edgelist_export(const pw_edgelist *e, uint32_t *indptr, uint32_t *indices, float *data,
                                 double *data64, uint64_t *id_offsets, char *id_chars) {
    if (!e) return fail(PW_ERR_INVALID, "null pointer");
    const pw::EdgeList &el = e->el;
    if (indptr) memcpy(indptr, el.indptr.data(), sizeof(uint32_t) * el.indptr.size());
    if (indices && !el.indices.empty()) memcpy(indices, el.indices.data(), sizeof(uint32_t) * el.indices.size());
    if (data && !el.data.empty()) memcpy(data, el.data.data(), sizeof(float) * el.data.size());
    if (data64 && !el.data64.empty()) memcpy(data64, el.data64.data(), sizeof(double) * el.data64.size());
    if (id_offsets) memcpy(id_offsets, el.id_off.data(), sizeof(uint64_t) * el.id_off.size());
    if (id_chars && !el.id_chars.empty()) memcpy(id_chars, el.id_chars.data(), el.id_chars.size());
    return PW_OK;
}

PW_EXPORT void pw_edgelist_destroy(pw_edgelist *e) { delete e; }

PW_EXPORT int pw_selftest_seqscan_f32(const float *x, uint32_t n, double r, int use_target, uint32_t chunk,
                                      uint32_t *index, float *sum) {
    if (!x || !index || !sum || chunk == 0) return fail(PW_ERR_INVALID, "bad argument");
    *index = seqscan_emulate<float>(x, n, r, use_target != 0, chunk, sum);
    return PW_OK;
}

PW_EXPORT int pw_selftest_seqscan_f64(const double *x, uint32_t n, double r, int use_target, uint32_t chunk,
                                      uint32_t *index, double *sum) {
    if (!x || !index || !sum || chunk == 0) return fail(PW_ERR_INVALID, "bad argument");
    *index = seqscan_emulate<double>(x, n, r, use_target != 0, chunk, sum);
    return PW_OK;
}
