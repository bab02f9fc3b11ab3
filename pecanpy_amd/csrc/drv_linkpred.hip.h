#pragma once
// Host driver, link prediction (linkpred.hip.h): the scores of given pairs over two pw_knn indexes, the exact AUC of two score
// arrays, non-edges from the seeded stream on a CSR handle.  Exports pw_knn_score_pairs_device, pw_auc_device,
// pw_sample_non_edges_device, pw_selftest_score_pairs, pw_selftest_auc, pw_selftest_sample_non_edges.  Stands on the core
// (stream_words_window of pecanpy_amd.hip through its declaration there), drv_knn, drv_pairs and the public pw_csr_create.
#include "drv_core.hip.h"
#include "drv_knn.hip.h"
#include "drv_pairs.hip.h"
#include "linkpred.hip.h"
#include "coo_csr.hip.h"   // the radix sort of pw_auc
#include "mtjump.hpp"      // mt_words_host: the host side of the self test

namespace {

constexpr uint64_t LP_BATCH_MIN = 1ull << 16, LP_BATCH_MAX = 1ull << 24;   // candidates per batch of the sampler (default form)

int lp_check_metric(int metric) {
    return metric == PW_KNN_DOT || metric == PW_KNN_COSINE ? 0 : fail(PW_ERR_INVALID, "pw_knn_score_pairs: metric must be PW_KNN_DOT or PW_KNN_COSINE");
}
int lp_dim_mismatch(uint32_t da, uint32_t db) {
    return fail(PW_ERR_INVALID, "pw_knn_score_pairs: the two indexes have dim " + std::to_string(da) + " and " + std::to_string(db));
}
int auc_check_sizes(uint64_t m, uint64_t n) {
    if (m < 1 || n < 1) return fail(PW_ERR_INVALID, "pw_auc: both arrays need at least one score");
    if (n >= (1ull << 32)) return fail(PW_ERR_INVALID, "pw_auc: n must be below 2^32");
    if ((unsigned __int128)m * n >= ((unsigned __int128)1 << 62)) return fail(PW_ERR_INVALID, "pw_auc: m * n must be below 2^62");
    return 0;
}
int auc_nan(const char *which, uint64_t i) { return fail(PW_ERR_INVALID, std::string("pw_auc: ") + which + "[" + std::to_string(i) + "] is a NaN"); }
int lp_no_non_edge(uint64_t n_nodes) {
    return fail(PW_ERR_INVALID, "pw_sample_non_edges: the graph of " + std::to_string(n_nodes) + " vertices has no off-diagonal non-edge");
}
int lp_cap_passed(uint64_t cap, uint64_t got, uint64_t m) {
    return fail(PW_ERR_INVALID, "pw_sample_non_edges: " + std::to_string(cap) + " candidates examined (the cap) gave " + std::to_string(got) + " of the " +
                                    std::to_string(m) + " non-edges asked for");
}

int score_pairs_impl(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int metric, double *d_score) {
    if (!a) return fail(PW_ERR_INVALID, "null pointer");
    if (!b) b = a;
    int rc;
    if ((rc = lp_check_metric(metric))) return rc;
    if (a->dim != b->dim) return lp_dim_mismatch(a->dim, b->dim);
    if (a->device != b->device) return fail(PW_ERR_INVALID, "pw_knn_score_pairs: the two indexes are on different devices");
    if (m == 0) return PW_OK;
    if (!d_u || !d_v || !d_score) return fail(PW_ERR_INVALID, "null pointer");
    HIP_TRY(hipSetDevice(a->device));
    if ((rc = check_pairs(nullptr, a->n_cu, d_u, d_v, m, a->n, b->n, "pw_knn_score_pairs"))) return rc;
    pw::LpScoreArgs s;
    s.A = a->X.p; s.B = b->X.p; s.anorms = a->norms.p; s.bnorms = b->norms.p;
    s.u = d_u; s.v = d_v; s.score = d_score;
    s.m = m; s.n_tiles = (m + 63) / 64;
    s.dim = a->dim; s.metric = (uint32_t)metric;
    uint64_t blocks = 0;
    if ((rc = persistent_tile_grid((const void *)pw::lp_score_pairs_kernel, (int)pw::LP_THREADS, pw::LP_WAVES, s.n_tiles, a->n_cu, 0, &blocks))) return rc;
    hipLaunchKernelGGL(pw::lp_score_pairs_kernel, dim3((unsigned)blocks), dim3(pw::LP_THREADS), 0, nullptr, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    return PW_OK;
}

int auc_impl(int device, const double *d_pos, uint64_t m, const double *d_neg, uint64_t n, uint64_t out[2]) {
    if (!out) return fail(PW_ERR_INVALID, "null pointer");
    int rc;
    if ((rc = auc_check_sizes(m, n))) return rc;
    if (!d_pos || !d_neg) return fail(PW_ERR_INVALID, "null pointer");
    if ((rc = check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int n_cu = std::max(1, prop.multiProcessorCount);
    const uint64_t n_waves = (n + pw::RADIX_SUB - 1) / pw::RADIX_SUB, hist_elems = (uint64_t)pw::RADIX_BINS * n_waves;
    DevBuf<uint64_t> pos_keys, neg_keys[2];
    DevBuf<uint32_t> hist, tmp;
    DevBuf<unsigned long long> cells;   // [0] first NaN of pos, [1] of neg, [2] wins, [3] ties
    if ((rc = dev_alloc(pos_keys, m)) || (rc = dev_alloc(neg_keys[0], n)) || (rc = dev_alloc(neg_keys[1], n)) || (rc = dev_alloc(hist, hist_elems)) ||
        (rc = dev_alloc(tmp, pw::scan_scratch_elems(hist_elems))) || (rc = dev_alloc(cells, 4)))
        return rc;
    HIP_TRY(hipMemsetAsync(cells.p, 0xff, 2 * sizeof(unsigned long long), nullptr));
    HIP_TRY(hipMemsetAsync(cells.p + 2, 0, 2 * sizeof(unsigned long long), nullptr));
    hipLaunchKernelGGL(pw::auc_keys_kernel, dim3(strided_grid(m, n_cu)), dim3(256), 0, nullptr, d_pos, m, pos_keys.p, (pw::LpFound *)(cells.p + 0));
    hipLaunchKernelGGL(pw::auc_keys_kernel, dim3(strided_grid(n, n_cu)), dim3(256), 0, nullptr, d_neg, n, neg_keys[0].p, (pw::LpFound *)(cells.p + 1));
    HIP_TRY(hipGetLastError());
    unsigned long long h[4];
    HIP_TRY(hipMemcpy(h, cells.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (h[0] != ~0ull) return auc_nan("pos", h[0]);
    if (h[1] != ~0ull) return auc_nan("neg", h[1]);
    uint64_t *keys[2] = {neg_keys[0].p, neg_keys[1].p};   // (the sort swaps the two views; the owners stay put)
    const unsigned wave_grid = (unsigned)((n_waves + 3) / 4);
    for (int shift = 0; shift < 64; shift += pw::RADIX_BITS) {
        hipLaunchKernelGGL(pw::radix_hist_kernel, dim3(wave_grid), dim3(256), 0, nullptr, (const uint64_t *)keys[0], n, shift, hist.p, n_waves);
        pw::exclusive_scan_inplace(nullptr, hist.p, hist_elems, tmp.p);
        hipLaunchKernelGGL(pw::radix_scatter_kernel<false>, dim3(wave_grid), dim3(256), 0, nullptr, (const uint64_t *)keys[0], (const uint32_t *)nullptr, keys[1],
                           (uint32_t *)nullptr, n, shift, (const uint32_t *)hist.p, n_waves);
        std::swap(keys[0], keys[1]);
    }
    hipLaunchKernelGGL(pw::auc_count_kernel, dim3(strided_grid(m, n_cu)), dim3(256), 0, nullptr, (const uint64_t *)pos_keys.p, m, (const uint64_t *)keys[0], n,
                       cells.p + 2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h + 2, cells.p + 2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    out[0] = h[2];
    out[1] = h[3];
    return PW_OK;
}

// batch: candidates per batch; 0 = by m and the share of acceptable candidates.  The output does not depend on it.
int sample_non_edges_impl(pw_graph *g, uint32_t seed, uint64_t first_candidate, uint64_t m, uint32_t *d_u, uint32_t *d_v, uint64_t *candidates_used,
                          uint64_t batch) {
    if (!g || !candidates_used || (m && (!d_u || !d_v))) return fail(PW_ERR_INVALID, "null pointer");
    if (g->gd->kind != 0) return fail(PW_ERR_UNSUPPORTED, "pw_sample_non_edges needs a CSR graph handle");
    if (m >= (1ull << 32)) return fail(PW_ERR_INVALID, "pw_sample_non_edges: m must be below 2^32");
    if (first_candidate >= (1ull << 60)) return fail(PW_ERR_INVALID, "pw_sample_non_edges: first_candidate must be below 2^60");
    if (set_device(g)) return PW_ERR_HIP;
    const uint32_t n_nodes = g->gd->n_nodes;
    const uint32_t *indptr = g->gd->d_indptr.p, *indices = g->gd->d_indices.p;
    DevBuf<unsigned long long> cells;   // [0] self loops, [1] the index of the batch's last wanted candidate
    int rc;
    if ((rc = dev_alloc(cells, 2))) return rc;
    HIP_TRY(hipMemsetAsync(cells.p, 0, 2 * sizeof(unsigned long long), g->stream));
    hipLaunchKernelGGL(pw::lp_loops_kernel, dim3(strided_grid(n_nodes, g->n_cu)), dim3(256), 0, g->stream, indptr, indices, n_nodes, cells.p);
    HIP_TRY(hipGetLastError());
    unsigned long long loops = 0;
    HIP_TRY(hipMemcpyAsync(&loops, cells.p, sizeof(loops), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    const uint64_t acceptable = pw::lp_acceptable(n_nodes, g->gd->nnz, loops);
    if (acceptable == 0) return lp_no_non_edge(n_nodes);
    if (m == 0) { *candidates_used = 0; return PW_OK; }
    const uint64_t cap = pw::lp_candidate_cap(m, n_nodes, acceptable);
    if (batch == 0) {   // what the call is expected to need and an eighth more, within the bounds
        const uint64_t expect = (cap - 64) / 16;
        batch = std::min(LP_BATCH_MAX, std::max(LP_BATCH_MIN, expect + expect / 8));
    }
    DevBuf<uint32_t> out_u, out_v, flag, tmp;   // (the outputs are written behind the last batch: a refused call writes nothing)
    if ((rc = dev_alloc(out_u, m)) || (rc = dev_alloc(out_v, m))) return rc;
    uint64_t got = 0, c0 = 0, used = 0;
    while (got < m) {
        if (c0 >= cap) return lp_cap_passed(cap, got, m);
        const uint64_t nb = std::min(batch, cap - c0);
        if (grow(flag, nb + 1) || grow(tmp, pw::scan_scratch_elems(nb + 1))) return PW_ERR_NOMEM;
        // the batch's words: candidates first_candidate + c0 .. + nb, two words each
        const uint32_t *words = nullptr;
        if ((rc = stream_words_window(g, seed, 2 * (first_candidate + c0), 2 * nb, &words))) return rc;
        hipLaunchKernelGGL(pw::lp_flag_kernel, dim3(strided_grid(nb + 1, g->n_cu)), dim3(256), 0, g->stream, indptr, indices, n_nodes, words, nb, flag.p);
        pw::exclusive_scan_inplace(g->stream, flag.p, nb + 1, tmp.p);
        const uint64_t want = m - got;
        hipLaunchKernelGGL(pw::lp_compact_kernel, dim3(strided_grid(nb, g->n_cu)), dim3(256), 0, g->stream, words, (const uint32_t *)flag.p, nb, n_nodes, want,
                           out_u.p + got, out_v.p + got, cells.p + 1);
        HIP_TRY(hipGetLastError());
        uint32_t total = 0;
        unsigned long long last = 0;
        HIP_TRY(hipMemcpyAsync(&last, cells.p + 1, sizeof(last), hipMemcpyDeviceToHost, g->stream));
        if ((rc = scan_total(g->stream, tmp.p, &total))) return rc;   // (waits for the stream: `last` is there too)
        if (total >= want) {   // the final batch, cut where acceptance number m falls
            used = c0 + last + 1;
            got = m;
        } else {
            got += total;
            c0 += nb;
        }
    }
    HIP_TRY(hipMemcpyAsync(d_u, out_u.p, sizeof(uint32_t) * m, hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(d_v, out_v.p, sizeof(uint32_t) * m, hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    *candidates_used = used;
    return PW_OK;
}

}  // namespace

PW_EXPORT int pw_knn_score_pairs_device(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, uint64_t m, int metric, double *d_score) {
    return score_pairs_impl(a, b, d_u, d_v, m, metric, d_score);
}

PW_EXPORT int pw_auc_device(int device, const double *d_pos, uint64_t m, const double *d_neg, uint64_t n, uint64_t out[2]) {
    return auc_impl(device, d_pos, m, d_neg, n, out);
}

PW_EXPORT int pw_sample_non_edges_device(pw_graph *g, uint32_t seed, uint64_t first_candidate, uint64_t m, uint32_t *d_u, uint32_t *d_v,
                                         uint64_t *candidates_used) {
    return sample_non_edges_impl(g, seed, first_candidate, m, d_u, d_v, candidates_used, 0);
}

PW_EXPORT int pw_selftest_score_pairs(int on_device, int device, const float *a, uint64_t na, const float *b, uint64_t nb, uint32_t dim, uint32_t dim_b,
                                      const uint32_t *u, const uint32_t *v, uint64_t m, int metric, double *score) {
    if (!a || (m && (!u || !v || !score))) return fail(PW_ERR_INVALID, "null pointer");
    int rc;
    if ((rc = knn_check_shape(na, dim)) || (b && (rc = knn_check_shape(nb, dim_b))) || (rc = lp_check_metric(metric))) return rc;
    if (!on_device) {
        std::vector<double> an(na), bn(b ? nb : 0);
        uint64_t where = 0;
        if (pw::knn_host_norms(a, na, dim, an.data(), &where) || (b && pw::knn_host_norms(b, nb, dim_b, bn.data(), &where))) return knn_bad_row(where);
        if (b && dim_b != dim) return lp_dim_mismatch(dim, dim_b);
        std::vector<double> sc(m);
        const uint64_t rows_b = b ? nb : na;
        switch (pw::lp_host_score_pairs(a, an.data(), na, b ? b : a, b ? bn.data() : an.data(), rows_b, dim, u, v, m, metric, sc.data(), &where)) {
            case pw::LP_HOST_U_RANGE: return pair_range("pw_knn_score_pairs", "u", where, u[where], na);
            case pw::LP_HOST_V_RANGE: return pair_range("pw_knn_score_pairs", "v", where, v[where], rows_b);
            default: break;
        }
        if (m) memcpy(score, sc.data(), sizeof(double) * m);
        return PW_OK;
    }
    KnnOwner ka, kb;
    if ((rc = knn_own(device, a, na, dim, ka)) || (b && (rc = knn_own(device, b, nb, dim_b, kb)))) return rc;
    DevBuf<uint32_t> d_u, d_v;
    DevBuf<double> d_score;
    if (m && ((rc = upload(d_u, u, m)) || (rc = upload(d_v, v, m)) || (rc = dev_alloc(d_score, m)))) return rc;
    if ((rc = score_pairs_impl(ka.get(), kb.get(), d_u.p, d_v.p, m, metric, d_score.p))) return rc;
    return m ? download(score, d_score, m) : PW_OK;
}

PW_EXPORT int pw_selftest_auc(int on_device, int device, const double *pos, uint64_t m, const double *neg, uint64_t n, uint64_t out[2]) {
    if (!out) return fail(PW_ERR_INVALID, "null pointer");
    int rc;
    if ((rc = auc_check_sizes(m, n))) return rc;
    if (!pos || !neg) return fail(PW_ERR_INVALID, "null pointer");
    if (!on_device) {
        std::vector<uint64_t> keys(std::max(m, n));
        uint64_t where = 0;
        if (pw::auc_host_keys(pos, m, keys.data(), &where)) return auc_nan("pos", where);
        if (pw::auc_host_keys(neg, n, keys.data(), &where)) return auc_nan("neg", where);
        std::sort(keys.begin(), keys.begin() + n);
        pw::auc_host_count(pos, m, keys.data(), n, out);
        return PW_OK;
    }
    if ((rc = check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> d_pos, d_neg;
    if ((rc = upload(d_pos, pos, m)) || (rc = upload(d_neg, neg, n))) return rc;
    return auc_impl(device, d_pos.p, m, d_neg.p, n, out);
}

PW_EXPORT int pw_selftest_sample_non_edges(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, uint32_t n_nodes, uint32_t seed,
                                           uint64_t first_candidate, uint64_t m, uint64_t batch, uint32_t *u, uint32_t *v, uint64_t *candidates_used) {
    if (!indptr || !candidates_used || (m && (!u || !v)) || n_nodes == 0 || (indptr[n_nodes] && !indices)) return fail(PW_ERR_INVALID, "null pointer");
    if (m >= (1ull << 32)) return fail(PW_ERR_INVALID, "pw_sample_non_edges: m must be below 2^32");
    if (first_candidate >= (1ull << 60)) return fail(PW_ERR_INVALID, "pw_sample_non_edges: first_candidate must be below 2^60");
    if (!on_device) {
        const uint64_t acceptable = pw::lp_acceptable(n_nodes, indptr[n_nodes], pw::lp_host_loops(indptr, indices, n_nodes));
        if (acceptable == 0) return lp_no_non_edge(n_nodes);
        if (m == 0) { *candidates_used = 0; return PW_OK; }
        const uint64_t cap = pw::lp_candidate_cap(m, n_nodes, acceptable);
        std::vector<uint32_t> hu(m), hv(m), words;
        uint64_t have0 = 0;   // words holds the words of the candidates have0 .. have0 + words.size() / 2
        auto more = [&](uint64_t c) {
            if (c >= have0 + words.size() / 2) {
                have0 = c;
                words.resize(2 * std::min<uint64_t>(1u << 16, cap - c));
                pw::mt_words_host(seed, 2 * (first_candidate + c), words.size(), words.data());
            }
            return words.data() + 2 * (c - have0);
        };
        uint64_t used = 0;
        if (pw::lp_host_sample(indptr, indices, n_nodes, m, cap, more, hu.data(), hv.data(), &used) == pw::LP_HOST_CAP) {
            uint64_t got = 0;   // (counted again for the message: the refused call's arrays are not the caller's)
            for (uint64_t c = 0; c < cap; c++) {
                const uint32_t *w = more(c);
                got += pw::lp_accept(indptr, indices, pw::lp_candidate(w[0], n_nodes), pw::lp_candidate(w[1], n_nodes)) ? 1 : 0;
            }
            return lp_cap_passed(cap, got, m);
        }
        memcpy(u, hu.data(), sizeof(uint32_t) * m);
        memcpy(v, hv.data(), sizeof(uint32_t) * m);
        *candidates_used = used;
        return PW_OK;
    }
    pw_graph *raw = nullptr;
    int rc;
    if ((rc = pw_csr_create(indptr, indices, nullptr, n_nodes, indptr[n_nodes], device, &raw))) return rc;
    GraphOwner g(raw);   // (declared before the buffers: they go first)
    DevBuf<uint32_t> d_u, d_v;
    if (m && ((rc = dev_alloc(d_u, m)) || (rc = dev_alloc(d_v, m)))) return rc;
    uint64_t used = 0;
    if ((rc = sample_non_edges_impl(g.get(), seed, first_candidate, m, d_u.p, d_v.p, &used, batch))) return rc;
    if (m && ((rc = download(u, d_u, m)) || (rc = download(v, d_v, m)))) return rc;
    *candidates_used = used;
    return PW_OK;
}
