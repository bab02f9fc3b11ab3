#pragma once
// Host driver, nearest neighbours of embedding vectors (knn.hip.h): the snapshot (pw_knn) and the batched query.
// Exports pw_knn_create*, pw_knn_query_device, pw_knn_info, pw_knn_norms_get, pw_knn_destroy, pw_selftest_knn.
#include "drv_core.hip.h"
#include "knn.hip.h"

// ---- nearest neighbours of embedding vectors, exact and ordered (csrc/knn.hip.h) --------------------------------------------
struct pw_knn {
    int device = 0, n_cu = 1;
    uint64_t n = 0;
    uint32_t dim = 0;
    DevBuf<float> X;         // the snapshot: float32[n, dim]
    DevBuf<double> norms;    // float64[n]
};

namespace {

constexpr uint64_t KNN_QD_BUDGET = 256ull << 20;   // bytes of widened queries per batch

int knn_check_call(const void *queries, const void *rows, uint32_t topn, int metric, const pw_knn_tiles *tiles) {
    if ((queries != nullptr) == (rows != nullptr)) return fail(PW_ERR_INVALID, "pw_knn_query: exactly one of queries and rows must be given");
    if (topn < 1 || topn > PW_KNN_MAX_TOPN)
        return fail(PW_ERR_INVALID, "pw_knn_query: topn = " + std::to_string(topn) + " outside 1.." + std::to_string(PW_KNN_MAX_TOPN));
    if (metric != PW_KNN_DOT && metric != PW_KNN_COSINE) return fail(PW_ERR_INVALID, "pw_knn_query: metric must be PW_KNN_DOT or PW_KNN_COSINE");
    if (tiles) {
        const uint32_t r = tiles->rows_per_block, c = tiles->col_chunk;
        if ((r != 0 && r != 64 && r != 128 && r != 256) || tiles->queries_per_tile > pw::KNN_QT || tiles->grid > 65536 || (c & 3u) || c > pw::KNN_KC)
            return fail(PW_ERR_INVALID, "pw_knn_tiles: rows_per_block 64 / 128 / 256, queries_per_tile <= 8, grid <= 65536, col_chunk a multiple of 4 <= 32");
    }
    return 0;
}

int knn_check_shape(uint64_t n_rows, uint32_t dim) {
    if (n_rows < 1 || n_rows >= (1ull << 32)) return fail(PW_ERR_INVALID, "pw_knn: n_rows must be in 1 .. 2^32 - 1");
    if (dim < 1 || dim > pw::KNN_MAX_DIM) return fail(PW_ERR_INVALID, "pw_knn: dim must be in 1.." + std::to_string(pw::KNN_MAX_DIM));
    return 0;
}

int knn_bad_row(uint64_t row) { return fail(PW_ERR_INVALID, "pw_knn: row " + std::to_string(row) + " of the matrix holds a NaN or an infinity"); }
int knn_bad_query(uint64_t q) { return fail(PW_ERR_INVALID, "pw_knn_query: query " + std::to_string(q) + " holds a NaN or an infinity"); }
int knn_row_range(uint64_t q, uint32_t row, uint64_t n) {
    return fail(PW_ERR_INVALID, "pw_knn_query: row number " + std::to_string(row) + " at position " + std::to_string(q) + " is outside the " +
                                    std::to_string(n) + " rows");
}

// an index of a self test, here and in every piece that makes one
using KnnOwner = std::unique_ptr<pw_knn, Closes<pw_knn, pw_knn_destroy>>;
int knn_own(int device, const float *vectors, uint64_t n_rows, uint32_t dim, KnnOwner &k) {
    pw_knn *raw = nullptr;
    const int rc = pw_knn_create(device, vectors, n_rows, dim, &raw);
    k.reset(raw);
    return rc;
}

// the index from a matrix in device or host memory: the copy, the norms, the refusal of non-finite rows
int knn_create_impl(int device, const float *vectors, hipMemcpyKind kind, uint64_t n_rows, uint32_t dim, pw_knn **out) {
    if (!vectors || !out) return fail(PW_ERR_INVALID, "null pointer");
    *out = nullptr;
    int rc;
    if ((rc = knn_check_shape(n_rows, dim)) || (rc = check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<pw_knn> k(new (std::nothrow) pw_knn());
    if (!k) return fail(PW_ERR_NOMEM, "pw_knn: out of host memory");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    k->device = device;
    k->n_cu = std::max(1, prop.multiProcessorCount);
    k->n = n_rows;
    k->dim = dim;
    DevBuf<pw::KnnFound> found;
    if ((rc = dev_alloc(k->X, (size_t)n_rows * dim)) || (rc = dev_alloc(k->norms, n_rows)) || (rc = dev_alloc(found, 1))) return rc;
    HIP_TRY(hipMemcpy(k->X.p, vectors, sizeof(float) * (size_t)n_rows * dim, kind));
    HIP_TRY(hipMemset(found.p, 0xff, sizeof(pw::KnnFound)));
    hipLaunchKernelGGL(pw::knn_norms_kernel, dim3(strided_grid(n_rows, k->n_cu)), dim3(256), 0, nullptr, (const float *)k->X.p, n_rows, dim, k->norms.p, found.p);
    HIP_TRY(hipGetLastError());
    pw::KnnFound h;
    HIP_TRY(hipMemcpy(&h, found.p, sizeof(h), hipMemcpyDeviceToHost));
    if (h.first_bad != ~0ull) return knn_bad_row(h.first_bad);
    *out = k.release();
    return PW_OK;
}

// the query of pw_knn_query_device and of pw_selftest_knn (tiles: forced, or nullptr)
int knn_query_impl(pw_knn *k, const float *d_queries, const uint32_t *d_rows, uint64_t nq, uint32_t topn, int metric, int exclude_self,
                   uint32_t *d_idx, double *d_score, const pw_knn_tiles *tiles, pw_knn_stats *stats) {
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    if (!k) return fail(PW_ERR_INVALID, "null pointer");
    if (int rc = knn_check_call(d_queries, d_rows, topn, metric, tiles)) return rc;
    if (stats) *stats = pw_knn_stats{0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (nq == 0) return PW_OK;
    if (!d_idx || !d_score) return fail(PW_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(k->device));

    // the queries' norms; a row number out of range and a non-finite query are refused before anything is written
    DevBuf<double> qnorms, qd, part_sc;
    DevBuf<uint32_t> part_ix;
    DevBuf<pw::KnnFound> found;
    int rc;
    if ((rc = dev_alloc(qnorms, nq)) || (rc = dev_alloc(found, 1))) return rc;
    HIP_TRY(hipMemsetAsync(found.p, 0xff, sizeof(pw::KnnFound), nullptr));
    hipLaunchKernelGGL(pw::knn_query_norms_kernel, dim3(strided_grid(nq, k->n_cu)), dim3(256), 0, nullptr, d_queries, d_rows, nq, k->n, k->dim,
                       (const double *)k->norms.p, qnorms.p, found.p);
    HIP_TRY(hipGetLastError());
    pw::KnnFound h;
    HIP_TRY(hipMemcpy(&h, found.p, sizeof(h), hipMemcpyDeviceToHost));
    if (h.first_range != ~0ull) {
        uint32_t row = 0;
        HIP_TRY(hipMemcpy(&row, d_rows + h.first_range, sizeof(row), hipMemcpyDeviceToHost));
        return knn_row_range(h.first_range, row, k->n);
    }
    if (h.first_bad != ~0ull) return knn_bad_query(h.first_bad);

    // the tile: row groups x query groups of the 8 wavefronts.  Few queries: more row groups, so that no wavefront idles
    const uint32_t rg = tiles && tiles->rows_per_block ? tiles->rows_per_block / 64 : (nq <= 16 ? 4u : nq <= 32 ? 2u : 1u);
    const uint32_t qt = tiles && tiles->queries_per_tile ? tiles->queries_per_tile : pw::KNN_QT;
    const uint32_t kc = tiles && tiles->col_chunk ? tiles->col_chunk : pw::KNN_KC;
    const uint32_t qg = pw::KNN_WAVES / rg, tile_q = qg * qt, R = 64 * rg, dimp = (k->dim + 3u) & ~3u;
    const uint64_t n_blocks = (k->n + R - 1) / R;
    const size_t lds = pw::knn_score_lds_bytes(rg, topn);
    HIP_TRY(hipFuncSetAttribute((const void *)pw::knn_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    uint64_t grid = tiles ? tiles->grid : 0;
    if (grid == 0) {   // what the device holds at once
        int occ = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)pw::knn_score_kernel, (int)pw::KNN_THREADS, lds));
        grid = (uint64_t)std::max(1, occ) * k->n_cu;
    }
    // a batch: whole tiles whose widened queries stay within the budget (one tile always fits)
    const uint64_t tiles_max = std::max<uint64_t>(1, KNN_QD_BUDGET / ((uint64_t)dimp * pw::KNN_QT * sizeof(double) * qg));
    const uint64_t batch = std::min<uint64_t>(nq, std::min<uint64_t>(tiles_max, (1u << 20)) * tile_q);

    pw::Event ev[3];
    for (auto &e : ev) HIP_TRY(e.create(hipEventDefault));
    double score_ms = 0, merge_ms = 0;
    uint32_t n_batches = 0, first_grid = 0, first_parts = 0;
    for (uint64_t q0 = 0; q0 < nq; q0 += batch, n_batches++) {
        const uint32_t nqb = (uint32_t)std::min<uint64_t>(batch, nq - q0);
        const uint32_t n_tiles = (nqb + tile_q - 1) / tile_q, n_slots = n_tiles * qg;
        const uint32_t row_parts = (uint32_t)std::min<uint64_t>(n_blocks, std::max<uint64_t>(1, (grid + n_tiles - 1) / n_tiles));
        const uint32_t tile_parts = (uint32_t)std::min<uint64_t>(n_tiles, std::max<uint64_t>(1, grid / row_parts));
        const uint32_t n_lists = row_parts * rg;
        const size_t part_elems = (size_t)n_lists * nqb * topn;
        if ((rc = grow(qd, (size_t)n_slots * dimp * pw::KNN_QT)) || (rc = grow(part_sc, part_elems)) || (rc = grow(part_ix, part_elems))) return rc;
        hipLaunchKernelGGL(pw::knn_stage_queries_kernel, dim3((unsigned)(((uint64_t)n_slots * pw::KNN_QT + 255) / 256)), dim3(256), 0, nullptr,
                           (const float *)k->X.p, d_queries, d_rows, q0, nqb, qt, n_slots, k->dim, dimp, qd.p);
        pw::KnnScoreArgs a;
        a.X = k->X.p; a.xnorms = k->norms.p; a.qd = qd.p; a.qnorms = qnorms.p + q0;
        a.qself = (d_rows && exclude_self) ? d_rows + q0 : nullptr;
        a.part_sc = part_sc.p; a.part_ix = part_ix.p;
        a.n = k->n; a.n_blocks = n_blocks;
        a.dim = k->dim; a.dimp = dimp; a.nqb = nqb; a.qt = qt; a.topn = topn; a.metric = (uint32_t)metric;
        a.rg = rg; a.kc = kc; a.row_parts = row_parts; a.tile_parts = tile_parts; a.n_tiles = n_tiles;
        HIP_TRY(hipEventRecord(ev[0], nullptr));
        hipLaunchKernelGGL(pw::knn_score_kernel, dim3(row_parts * tile_parts), dim3(pw::KNN_THREADS), lds, nullptr, a);
        HIP_TRY(hipEventRecord(ev[1], nullptr));
        hipLaunchKernelGGL(pw::knn_merge_kernel, dim3((nqb + 3) / 4), dim3(256), 0, nullptr, (const double *)part_sc.p, (const uint32_t *)part_ix.p,
                           n_lists, nqb, topn, d_idx + q0 * topn, d_score + q0 * topn);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[2], nullptr));
        HIP_TRY(hipEventSynchronize(ev[2]));   // (the next batch may grow the buffers this one reads)
        float ms_score = 0, ms_merge = 0;
        HIP_TRY(hipEventElapsedTime(&ms_score, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_merge, ev[1], ev[2]));
        score_ms += ms_score;
        merge_ms += ms_merge;
        if (q0 == 0) { first_grid = row_parts * tile_parts; first_parts = row_parts; }
    }
    if (stats) {
        stats->score_ms = score_ms; stats->merge_ms = merge_ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
        stats->grid = first_grid; stats->row_parts = first_parts;
        stats->rows_per_block = R; stats->queries_per_tile = qt; stats->col_chunk = kc;
        stats->batches = n_batches;
    }
    return PW_OK;
}

}  // namespace

PW_EXPORT int pw_knn_create_device(int device, const float *d_vectors, uint64_t n_rows, uint32_t dim, pw_knn **out) {
    return knn_create_impl(device, d_vectors, hipMemcpyDeviceToDevice, n_rows, dim, out);
}

PW_EXPORT int pw_knn_create(int device, const float *vectors, uint64_t n_rows, uint32_t dim, pw_knn **out) {
    return knn_create_impl(device, vectors, hipMemcpyHostToDevice, n_rows, dim, out);
}

PW_EXPORT int pw_knn_query_device(pw_knn *k, const float *d_queries, const uint32_t *d_rows, uint64_t nq, uint32_t topn, int metric,
                                  int exclude_self, uint32_t *d_idx, double *d_score, pw_knn_stats *stats) {
    return knn_query_impl(k, d_queries, d_rows, nq, topn, metric, exclude_self, d_idx, d_score, nullptr, stats);
}

PW_EXPORT int pw_knn_info(const pw_knn *k, uint64_t *n_rows, uint32_t *dim, uint64_t *bytes) {
    if (!k) return fail(PW_ERR_INVALID, "null pointer");
    if (n_rows) *n_rows = k->n;
    if (dim) *dim = k->dim;
    if (bytes) *bytes = k->X.bytes() + k->norms.bytes();
    return PW_OK;
}

PW_EXPORT int pw_knn_norms_get(pw_knn *k, double *d_norms) {
    if (!k || !d_norms) return fail(PW_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(k->device));
    HIP_TRY(hipMemcpy(d_norms, k->norms.p, sizeof(double) * (size_t)k->n, hipMemcpyDeviceToDevice));
    return PW_OK;
}

PW_EXPORT void pw_knn_destroy(pw_knn *k) {
    if (!k) return;
    (void)hipSetDevice(k->device);
    delete k;
}

PW_EXPORT int pw_selftest_knn(int on_device, int device, const float *vectors, uint64_t n, uint32_t dim, const float *queries,
                              const uint32_t *rows, uint64_t nq, uint32_t topn, int metric, int exclude_self, const pw_knn_tiles *tiles,
                              uint32_t *idx, double *score) {
    if (!vectors || (nq && (!idx || !score))) return fail(PW_ERR_INVALID, "null pointer");
    int rc;
    if ((rc = knn_check_shape(n, dim)) || (rc = knn_check_call(queries, rows, topn, metric, tiles))) return rc;
    if (!on_device) {
        std::vector<double> norms(n), qnorms(nq);
        std::vector<uint32_t> ix((size_t)nq * topn);
        std::vector<double> sc((size_t)nq * topn);
        uint64_t where = 0;
        switch (pw::knn_host_query(vectors, n, dim, queries, rows, nq, topn, metric, exclude_self, ix.data(), sc.data(), norms.data(),
                                   qnorms.data(), &where)) {
            case pw::KNN_HOST_BAD_ROW: return knn_bad_row(where);
            case pw::KNN_HOST_BAD_QUERY: return knn_bad_query(where);
            case pw::KNN_HOST_ROW_RANGE: return knn_row_range(where, rows[where], n);
            default: break;
        }
        if (nq) {
            memcpy(idx, ix.data(), sizeof(uint32_t) * ix.size());
            memcpy(score, sc.data(), sizeof(double) * sc.size());
        }
        return PW_OK;
    }
    KnnOwner k;
    if ((rc = knn_own(device, vectors, n, dim, k))) return rc;
    if (nq == 0) return PW_OK;
    DevBuf<float> d_q;
    DevBuf<uint32_t> d_r, d_idx;
    DevBuf<double> d_score;
    if ((rc = dev_alloc(d_idx, (size_t)nq * topn)) || (rc = dev_alloc(d_score, (size_t)nq * topn))) return rc;
    if ((rc = queries ? upload(d_q, queries, (size_t)nq * dim) : upload(d_r, rows, nq))) return rc;
    if ((rc = knn_query_impl(k.get(), queries ? d_q.p : nullptr, rows ? d_r.p : nullptr, nq, topn, metric, exclude_self, d_idx.p, d_score.p, tiles,
                             nullptr)))
        return rc;
    if ((rc = download(idx, d_idx, (size_t)nq * topn)) || (rc = download(score, d_score, (size_t)nq * topn))) return rc;
    return PW_OK;
}
