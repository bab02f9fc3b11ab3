#pragma once
// Host driver, edges held out by the seeded stream (holdout.hip.h): the train CSR and the held-out pairs of a CSR handle.
// Exports pw_holdout_edges_device, pw_holdout_dev_shape, pw_holdout_dev_fill, pw_holdout_dev_destroy, pw_selftest_holdout_edges.
// Stands on the core (stream_words_window of pecanpy_amd.hip through its declaration there) and the public pw_csr_create / pw_csr_dev_export.
#include "drv_core.hip.h"
#include "holdout.hip.h"
#include "mtjump.hpp"   // mt_words_host: the host side of the self test

struct pw_holdout_dev {
    int device = 0;
    uint64_t held = 0, units = 0, protected_units = 0;
    DevBuf<uint32_t> d_u, d_v;
    DevBuf<float> d_w;
};

PW_EXPORT void pw_holdout_dev_destroy(pw_holdout_dev *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

namespace {

constexpr uint64_t HO_BATCH = 1ull << 24;   // words expanded at a time (default form): 64 MiB of stream words

using HoldoutOwner = std::unique_ptr<pw_holdout_dev, Closes<pw_holdout_dev, pw_holdout_dev_destroy>>;

int ho_missing_mate(uint64_t e) {
    return fail(PW_ERR_INVALID, "pw_holdout_edges: the CSR is not symmetric: the entry at position " + std::to_string(e) +
                                    " has no mate (pass directed = 1 for a directed graph)");
}
int ho_check_args(uint64_t first_word) {
    return first_word >= (1ull << 60) ? fail(PW_ERR_INVALID, "pw_holdout_edges: first_word must be below 2^60") : 0;
}

// batch: words expanded at a time; 0 = HO_BATCH.  The outputs do not depend on it.  stage_ms (may be NULL): the wall clock of the word
// expansion (its buffer's growth too), the flag kernels, the scans with the compaction -- each ended by a stream synchronise, for tools/holdout_bench.py
int holdout_edges_impl(pw_graph *g, int directed, uint32_t seed, uint64_t first_word, uint32_t threshold, int protect, uint64_t batch,
                       pw_csr_dev **train, pw_holdout_dev **held, double *stage_ms) {
    if (!g || !train || !held) return fail(PW_ERR_INVALID, "null pointer");
    if (g->gd->kind != 0) return fail(PW_ERR_UNSUPPORTED, "pw_holdout_edges needs a CSR graph handle");
    int rc;
    if ((rc = ho_check_args(first_word))) return rc;
    if (set_device(g)) return PW_ERR_HIP;
    const uint32_t n_nodes = g->gd->n_nodes, nnz = g->gd->nnz;
    const uint32_t *indptr = g->gd->d_indptr.p, *indices = g->gd->d_indices.p;
    const float *data = (const float *)g->gd->d_data.p;
    if (batch == 0) batch = HO_BATCH;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double ms[3] = {0, 0, 0};

    DevBuf<uint8_t> flags;
    DevBuf<uint32_t> pos, tmp;
    DevBuf<pw::HoCells> cells;
    if ((rc = dev_alloc(flags, (size_t)nnz + 1)) || (rc = dev_alloc(cells, 1))) return rc;
    HIP_TRY(hipMemsetAsync(flags.p, 0, (size_t)nnz + 1, g->stream));
    HIP_TRY(hipMemsetAsync(cells.p, 0xff, sizeof(unsigned long long), g->stream));
    HIP_TRY(hipMemsetAsync(&cells.p->units, 0, 2 * sizeof(unsigned long long), g->stream));
    for (uint64_t e0 = 0; e0 < nnz; e0 += batch) {
        const uint64_t nb = std::min<uint64_t>(batch, nnz - e0);
        double t0 = now();
        const uint32_t *words = nullptr;   // the batch's words: w[first_word + e0 .. + nb)
        if ((rc = stream_words_window(g, seed, first_word + e0, nb, &words))) return rc;
        if (stage_ms) { HIP_TRY(hipStreamSynchronize(g->stream)); ms[0] += (now() - t0) * 1e3; t0 = now(); }
        hipLaunchKernelGGL(pw::ho_flag_kernel, dim3(strided_grid(nb, g->n_cu)), dim3(256), 0, g->stream, indptr, indices, n_nodes, directed ? 1 : 0,
                           protect ? 1 : 0, threshold, words, (uint32_t)e0, (uint32_t)nb, flags.p, cells.p);
        HIP_TRY(hipGetLastError());
        if (stage_ms) { HIP_TRY(hipStreamSynchronize(g->stream)); ms[1] += (now() - t0) * 1e3; }
    }
    pw::HoCells h;
    HIP_TRY(hipMemcpyAsync(&h, cells.p, sizeof(h), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (h.missing != ~0ull) return ho_missing_mate(h.missing);

    const double t0 = now();
    CsrDevOwner c(new pw_csr_dev());
    HoldoutOwner ho(new pw_holdout_dev());
    c->device = ho->device = g->device;
    c->n_nodes = n_nodes;
    ho->units = h.units;
    ho->protected_units = h.prot;
    if ((rc = dev_alloc(c->d_indptr, (size_t)n_nodes + 1))) return rc;
    if (nnz == 0) {   // (no entry: no scan to launch)
        HIP_TRY(hipMemsetAsync(c->d_indptr.p, 0, sizeof(uint32_t) * ((size_t)n_nodes + 1), g->stream));
        if ((rc = dev_alloc(c->d_indices, 0)) || (rc = dev_alloc(ho->d_u, 0)) || (rc = dev_alloc(ho->d_v, 0)) || (rc = dev_alloc(ho->d_w, 0))) return rc;
        HIP_TRY(hipStreamSynchronize(g->stream));
        *train = c.release();
        *held = ho.release();
        return PW_OK;
    }
    const uint64_t cells_n = (uint64_t)nnz + 1;
    if ((rc = dev_alloc(pos, cells_n)) || (rc = dev_alloc(tmp, pw::scan_scratch_elems(cells_n)))) return rc;
    uint32_t total = 0;
    pw::exclusive_scan(g->stream, cells_n, pw::HoBitCount{flags.p, nnz, pw::HO_KEEP}, pw::ScanStore<uint32_t>{pos.p}, tmp.p);
    HIP_TRY(hipGetLastError());
    if ((rc = scan_total(g->stream, tmp.p, &total))) return rc;
    c->nnz = total;
    if ((rc = dev_alloc(c->d_indices, total)) || (data && (rc = dev_alloc(c->d_data, total)))) return rc;
    hipLaunchKernelGGL(pw::ho_compact_kernel, dim3(strided_grid(nnz, g->n_cu)), dim3(256), 0, g->stream, indices, data, (const uint8_t *)flags.p,
                       (const uint32_t *)pos.p, nnz, c->d_indices.p, c->d_data.p);
    hipLaunchKernelGGL(pw::ho_indptr_kernel, dim3(strided_grid((uint64_t)n_nodes + 1, g->n_cu)), dim3(256), 0, g->stream, indptr, (const uint32_t *)pos.p, n_nodes,
                       c->d_indptr.p);
    pw::exclusive_scan(g->stream, cells_n, pw::HoBitCount{flags.p, nnz, pw::HO_HELD}, pw::ScanStore<uint32_t>{pos.p}, tmp.p);
    HIP_TRY(hipGetLastError());
    if ((rc = scan_total(g->stream, tmp.p, &total))) return rc;
    ho->held = total;
    if ((rc = dev_alloc(ho->d_u, total)) || (rc = dev_alloc(ho->d_v, total)) || (rc = dev_alloc(ho->d_w, total))) return rc;
    hipLaunchKernelGGL(pw::ho_held_kernel, dim3(strided_grid(nnz, g->n_cu)), dim3(256), 0, g->stream, indptr, indices, data, n_nodes, (const uint8_t *)flags.p,
                       (const uint32_t *)pos.p, nnz, ho->d_u.p, ho->d_v.p, ho->d_w.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g->stream));
    ms[2] = (now() - t0) * 1e3;
    if (stage_ms) { stage_ms[0] = ms[0]; stage_ms[1] = ms[1]; stage_ms[2] = ms[2]; }
    *train = c.release();
    *held = ho.release();
    return PW_OK;
}

}  // namespace

PW_EXPORT int pw_holdout_edges_device(pw_graph *g, int directed, uint32_t seed, uint64_t first_word, uint32_t threshold, int protect,
                                      pw_csr_dev **train, pw_holdout_dev **held, double stage_ms[3]) {
    return holdout_edges_impl(g, directed, seed, first_word, threshold, protect, 0, train, held, stage_ms);
}

PW_EXPORT int pw_holdout_dev_shape(const pw_holdout_dev *h, uint64_t *held, uint64_t *units, uint64_t *protected_units) {
    if (!h) return fail(PW_ERR_INVALID, "null pointer");
    if (held) *held = h->held;
    if (units) *units = h->units;
    if (protected_units) *protected_units = h->protected_units;
    return PW_OK;
}

PW_EXPORT int pw_holdout_dev_fill(const pw_holdout_dev *h, uint32_t *d_u, uint32_t *d_v, float *d_weight) {
    if (!h || (h->held && (!d_u || !d_v || !d_weight))) return fail(PW_ERR_INVALID, "null pointer");
    if (!h->held) return PW_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy(d_u, h->d_u.p, sizeof(uint32_t) * h->held, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(d_v, h->d_v.p, sizeof(uint32_t) * h->held, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(d_weight, h->d_w.p, sizeof(float) * h->held, hipMemcpyDeviceToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return PW_OK;
}

PW_EXPORT int pw_selftest_holdout_edges(int on_device, int device, const uint32_t *indptr, const uint32_t *indices, const float *data, uint32_t n_nodes,
                                        int directed, uint32_t seed, uint64_t first_word, uint32_t threshold, int protect, uint64_t batch,
                                        uint32_t *out_indptr, uint32_t *out_indices, float *out_data, uint32_t *u, uint32_t *v, float *weight,
                                        uint64_t counts[4]) {
    if (!indptr || !out_indptr || !counts || n_nodes == 0) return fail(PW_ERR_INVALID, "null pointer");
    const uint32_t nnz = indptr[n_nodes];
    if (nnz && (!indices || !out_indices || !u || !v || !weight)) return fail(PW_ERR_INVALID, "null pointer");
    int rc;
    if ((rc = ho_check_args(first_word))) return rc;
    if (!on_device) {
        if (indptr[0] != 0) return fail(PW_ERR_INVALID, "indptr[0] != 0");
        for (uint32_t r = 0; r < n_nodes; r++)
            if (indptr[r + 1] < indptr[r]) return fail(PW_ERR_INVALID, "indptr not monotone");
        for (uint32_t r = 0; r < n_nodes; r++)
            for (uint32_t e = indptr[r]; e < indptr[r + 1]; e++)
                if (indices[e] >= n_nodes || (e > indptr[r] && indices[e] <= indices[e - 1]))
                    return fail(PW_ERR_INVALID, "pw_holdout_edges: column indices must be below n_nodes and strictly ascending within a row");
        std::vector<uint32_t> words(nnz), t_indptr((size_t)n_nodes + 1), t_indices(nnz), hu(nnz), hv(nnz);
        std::vector<float> t_data(nnz), hw(nnz);
        if (nnz) pw::mt_words_host(seed, first_word, nnz, words.data());
        uint64_t where = 0, cnt[4];
        if (pw::ho_host_split(indptr, indices, data, n_nodes, directed, protect, threshold, [&](uint32_t e) { return words[e]; }, t_indptr.data(),
                              t_indices.data(), t_data.data(), hu.data(), hv.data(), hw.data(), cnt, &where) == pw::HO_HOST_MISSING)
            return ho_missing_mate(where);
        memcpy(out_indptr, t_indptr.data(), sizeof(uint32_t) * ((size_t)n_nodes + 1));
        if (cnt[0]) memcpy(out_indices, t_indices.data(), sizeof(uint32_t) * cnt[0]);
        if (cnt[0] && out_data) memcpy(out_data, t_data.data(), sizeof(float) * cnt[0]);
        if (cnt[1]) {
            memcpy(u, hu.data(), sizeof(uint32_t) * cnt[1]);
            memcpy(v, hv.data(), sizeof(uint32_t) * cnt[1]);
            memcpy(weight, hw.data(), sizeof(float) * cnt[1]);
        }
        memcpy(counts, cnt, sizeof(cnt));
        return PW_OK;
    }
    pw_graph *raw = nullptr;
    if ((rc = pw_csr_create(indptr, indices, data, n_nodes, nnz, device, &raw))) return rc;
    GraphOwner g(raw);   // (declared before the results: they go first)
    pw_csr_dev *c_raw = nullptr;
    pw_holdout_dev *h_raw = nullptr;
    if ((rc = holdout_edges_impl(g.get(), directed, seed, first_word, threshold, protect, batch, &c_raw, &h_raw, nullptr))) return rc;
    CsrDevOwner c(c_raw);
    HoldoutOwner ho(h_raw);
    if ((rc = pw_csr_dev_export(c.get(), out_indptr, out_indices, out_data))) return rc;
    if (ho->held && ((rc = download(u, ho->d_u, ho->held)) || (rc = download(v, ho->d_v, ho->held)) || (rc = download(weight, ho->d_w, ho->held)))) return rc;
    counts[0] = c->nnz; counts[1] = ho->held; counts[2] = ho->units; counts[3] = ho->protected_units;
    return PW_OK;
}
