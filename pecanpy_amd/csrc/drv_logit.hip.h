#pragma once
// Host driver, exact logistic regression on embedding rows and pair operators (logit.hip.h): one evaluation of the loss, the
// gradient and the decision values over two pw_knn indexes.  Exports pw_logit_eval_device, pw_logit_eval_device_grid,
// pw_selftest_logit, pw_selftest_logit_math.  Stands on the core, drv_knn (pw_knn, KnnOwner, knn_check_shape) and drv_pairs (pair_range).
#include "drv_core.hip.h"
#include "drv_knn.hip.h"
#include "drv_pairs.hip.h"
#include "logit.hip.h"

namespace {

constexpr int LG_MAX_BLOCKS = 65536;

int lg_bad_label(uint64_t i, uint32_t y) {
    return fail(PW_ERR_INVALID, "pw_logit_eval: label y[" + std::to_string(i) + "] = " + std::to_string(y) + " is neither 0 nor 1");
}
int lg_bad_z(uint64_t i) { return fail(PW_ERR_INVALID, "pw_logit_eval: the decision value z[" + std::to_string(i) + "] is not finite"); }

// what needs no data, in the definition's order
int lg_check_args(int op, uint32_t dim_a, uint32_t dim_b, bool one_device, uint64_t m, const double *theta, double l2, int blocks) {
    if (!pw::lg_op_known(op))
        return fail(PW_ERR_INVALID, "pw_logit_eval: op " + std::to_string(op) +
                                        " is none of PW_LOGIT_ROW, PW_LOGIT_AVERAGE, PW_LOGIT_HADAMARD, PW_LOGIT_L1, PW_LOGIT_L2");
    if (dim_a != dim_b) return fail(PW_ERR_INVALID, "pw_logit_eval: the two indexes have dim " + std::to_string(dim_a) + " and " + std::to_string(dim_b));
    if (!one_device) return fail(PW_ERR_INVALID, "pw_logit_eval: the two indexes are on different devices");
    if (dim_a > pw::LG_MAX_DIM)
        return fail(PW_ERR_UNSUPPORTED, "pw_logit_eval: dim " + std::to_string(dim_a) + " is above the trainer's cap of " + std::to_string(pw::LG_MAX_DIM));
    if (m < 1 || m >= pw::LG_MAX_M) return fail(PW_ERR_INVALID, "pw_logit_eval: m must be in 1 .. 2^40 - 1");
    if (!pw::lg_l2_valid(l2)) return fail(PW_ERR_INVALID, "pw_logit_eval: l2 must be finite and >= 0");
    if (!theta) return fail(PW_ERR_INVALID, "null pointer");
    const uint32_t bad = pw::lg_host_theta_bad(theta, dim_a);
    if (bad <= dim_a) return fail(PW_ERR_INVALID, "pw_logit_eval: theta[" + std::to_string(bad) + "] is not finite");
    if (blocks != -1 && (blocks < 1 || blocks > LG_MAX_BLOCKS)) return fail(PW_ERR_INVALID, "pw_logit_eval: blocks must be -1 or in 1 .. 65536");
    return 0;
}

template <int OP> const void *lg_grad_fn(uint32_t nj) {
    switch (nj) {
        case 1: return (const void *)pw::lg_grad_kernel<OP, 1>;
        case 2: return (const void *)pw::lg_grad_kernel<OP, 2>;
        case 3: return (const void *)pw::lg_grad_kernel<OP, 3>;
        default: return (const void *)pw::lg_grad_kernel<OP, 4>;
    }
}
const void *lg_forward_fn(int op) {
    switch (op) {
        case pw::LG_ROW: return (const void *)pw::lg_forward_kernel<pw::LG_ROW>;
        case pw::LG_AVERAGE: return (const void *)pw::lg_forward_kernel<pw::LG_AVERAGE>;
        case pw::LG_HADAMARD: return (const void *)pw::lg_forward_kernel<pw::LG_HADAMARD>;
        case pw::LG_L1: return (const void *)pw::lg_forward_kernel<pw::LG_L1>;
        default: return (const void *)pw::lg_forward_kernel<pw::LG_L2>;
    }
}
const void *lg_grad_fn(int op, uint32_t nj) {
    switch (op) {
        case pw::LG_ROW: return lg_grad_fn<pw::LG_ROW>(nj);
        case pw::LG_AVERAGE: return lg_grad_fn<pw::LG_AVERAGE>(nj);
        case pw::LG_HADAMARD: return lg_grad_fn<pw::LG_HADAMARD>(nj);
        case pw::LG_L1: return lg_grad_fn<pw::LG_L1>(nj);
        default: return lg_grad_fn<pw::LG_L2>(nj);
    }
}

// blocks: the grid of both kernels (-1: what the device holds at once).  No result depends on it.
// kernel_ms (may be null): the device time of the forward, gradient and reduce kernels, between two events.
int logit_eval_impl(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, const uint8_t *d_y, uint64_t m, int op, const double *theta,
                    double l2, double *loss, double *grad, double *d_z, int blocks, float *kernel_ms) {
    if (!a) return fail(PW_ERR_INVALID, "null pointer");
    if (!b) b = a;
    int rc;
    if ((rc = lg_check_args(op, a->dim, b->dim, a->device == b->device, m, theta, l2, blocks))) return rc;
    if (!d_u || (op != pw::LG_ROW && !d_v) || (d_y ? (!loss || !grad) : !d_z)) return fail(PW_ERR_INVALID, "null pointer");
    if (kernel_ms) *kernel_ms = 0.f;
    HIP_TRY(hipSetDevice(a->device));
    const uint32_t dim = a->dim, n_cols = dim + 2;
    const uint64_t n_chunks = (m + pw::LG_CHUNK - 1) / pw::LG_CHUNK;

    DevBuf<pw::LgFound> found;
    DevBuf<double> theta_dev, z_tmp, r_tmp, l_tmp, part, totals;
    if ((rc = dev_alloc(found, 1)) || (rc = dev_alloc(theta_dev, dim + 1)) || (d_z && (rc = dev_alloc(z_tmp, m)))) return rc;
    if (d_y && ((rc = dev_alloc(r_tmp, m)) || (rc = dev_alloc(l_tmp, m)) || (rc = dev_alloc(part, (size_t)n_chunks * n_cols)) ||
                (rc = dev_alloc(totals, n_cols))))
        return rc;
    HIP_TRY(hipMemsetAsync(found.p, 0xff, sizeof(pw::LgFound), nullptr));
    HIP_TRY(hipMemcpyAsync(theta_dev.p, theta, sizeof(double) * (dim + 1), hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(pw::lg_check_kernel, dim3(strided_grid(m, a->n_cu)), dim3(256), 0, nullptr, d_u, d_v, d_y, m, a->n, b->n, op, found.p);
    HIP_TRY(hipGetLastError());
    pw::LgFound h;
    HIP_TRY(hipMemcpy(&h, found.p, sizeof(h), hipMemcpyDeviceToHost));
    if (h.row != ~0ull) {
        uint32_t ru = 0, rv = 0;
        HIP_TRY(hipMemcpy(&ru, d_u + h.row, sizeof(ru), hipMemcpyDeviceToHost));
        if (ru >= a->n) return pair_range("pw_logit_eval", "u", h.row, ru, a->n);
        HIP_TRY(hipMemcpy(&rv, d_v + h.row, sizeof(rv), hipMemcpyDeviceToHost));
        return pair_range("pw_logit_eval", "v", h.row, rv, b->n);
    }
    if (h.label != ~0ull) {
        uint8_t y = 0;
        HIP_TRY(hipMemcpy(&y, d_y + h.label, sizeof(y), hipMemcpyDeviceToHost));
        return lg_bad_label(h.label, y);
    }

    pw::LgFwdArgs f;
    f.A = a->X.p; f.B = b->X.p; f.u = d_u; f.v = d_v; f.y = d_y; f.theta = theta_dev.p;
    f.z = z_tmp.p; f.r = r_tmp.p; f.ell = l_tmp.p; f.found = found.p;
    f.m = m; f.n_tiles = (m + 63) / 64; f.dim = dim;
    const void *fwd = lg_forward_fn(op);
    uint64_t fwd_blocks = 0, grad_blocks = 0;   // (the occupancy is asked for with a forced grid too, as it always was)
    if ((rc = persistent_tile_grid(fwd, (int)pw::LG_FWD_THREADS, pw::LG_FWD_WAVES, f.n_tiles, a->n_cu, 0, &fwd_blocks))) return rc;
    if (blocks > 0) fwd_blocks = (uint64_t)blocks;
    pw::Event ev[2];
    if (kernel_ms) {
        for (auto &e : ev) HIP_TRY(e.create(hipEventDefault));
        HIP_TRY(hipEventRecord(ev[0], nullptr));
    }
    {
        void *args[] = {(void *)&f};
        HIP_TRY(hipLaunchKernel(fwd, dim3((unsigned)fwd_blocks), dim3(pw::LG_FWD_THREADS), args, 0, nullptr));
    }
    if (d_y) {
        pw::LgGradArgs g;
        g.A = a->X.p; g.B = b->X.p; g.u = d_u; g.v = d_v; g.r = r_tmp.p; g.ell = l_tmp.p; g.part = part.p;
        g.m = m; g.n_chunks = n_chunks; g.dim = dim;
        const void *gk = lg_grad_fn(op, (dim + pw::LG_COLS - 1) / pw::LG_COLS);
        if ((rc = persistent_tile_grid(gk, (int)pw::LG_GRAD_THREADS, pw::LG_GRAD_WAVES, n_chunks, a->n_cu, 0, &grad_blocks))) return rc;
        if (blocks > 0) grad_blocks = (uint64_t)blocks;
        void *args[] = {(void *)&g};
        HIP_TRY(hipLaunchKernel(gk, dim3((unsigned)grad_blocks), dim3(pw::LG_GRAD_THREADS), args, 0, nullptr));
        hipLaunchKernelGGL(pw::lg_reduce_kernel, dim3((n_cols + 63) / 64), dim3(64), 0, nullptr, (const double *)part.p, n_chunks, n_cols, totals.p);
        HIP_TRY(hipGetLastError());
    }
    if (kernel_ms) HIP_TRY(hipEventRecord(ev[1], nullptr));
    HIP_TRY(hipMemcpy(&h, found.p, sizeof(h), hipMemcpyDeviceToHost));   // (the null stream: behind the kernels)
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, ev[0], ev[1]));
    if (h.z != ~0ull) return lg_bad_z(h.z);
    if (d_y) {
        std::vector<double> G(n_cols), out(dim + 1);
        HIP_TRY(hipMemcpy(G.data(), totals.p, sizeof(double) * n_cols, hipMemcpyDeviceToHost));
        double value = 0.0;
        pw::lg_finish(G.data(), dim, m, theta, l2, &value, out.data());
        *loss = value;
        memcpy(grad, out.data(), sizeof(double) * (dim + 1));
    }
    if (d_z) HIP_TRY(hipMemcpy(d_z, z_tmp.p, sizeof(double) * m, hipMemcpyDeviceToDevice));
    return PW_OK;
}

}  // namespace

PW_EXPORT int pw_logit_eval_device(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, const uint8_t *d_y, uint64_t m, int op,
                                   const double *theta, double l2, double *loss, double *grad, double *d_z) {
    return logit_eval_impl(a, b, d_u, d_v, d_y, m, op, theta, l2, loss, grad, d_z, -1, nullptr);
}

PW_EXPORT int pw_logit_eval_device_grid(pw_knn *a, const pw_knn *b, const uint32_t *d_u, const uint32_t *d_v, const uint8_t *d_y, uint64_t m, int op,
                                        const double *theta, double l2, double *loss, double *grad, double *d_z, int blocks, float *kernel_ms) {
    return logit_eval_impl(a, b, d_u, d_v, d_y, m, op, theta, l2, loss, grad, d_z, blocks, kernel_ms);
}

PW_EXPORT int pw_selftest_logit(int on_device, int device, const float *a, uint64_t na, const float *b, uint64_t nb, uint32_t dim, const uint32_t *u,
                                const uint32_t *v, const uint8_t *y, uint64_t m, int op, const double *theta, double l2, int blocks, double *loss,
                                double *grad, double *z) {
    if (!a) return fail(PW_ERR_INVALID, "null pointer");
    int rc;
    if ((rc = knn_check_shape(na, dim)) || (b && (rc = knn_check_shape(nb, dim)))) return rc;
    if ((rc = lg_check_args(op, dim, dim, true, m, theta, l2, blocks))) return rc;
    if (!u || (op != pw::LG_ROW && !v) || (y ? (!loss || !grad) : !z)) return fail(PW_ERR_INVALID, "null pointer");
    if (!on_device) {
        std::vector<double> norms(std::max<uint64_t>(na, b ? nb : 0));
        uint64_t where = 0;
        if (pw::knn_host_norms(a, na, dim, norms.data(), &where) || (b && pw::knn_host_norms(b, nb, dim, norms.data(), &where))) return knn_bad_row(where);
        const uint64_t rows_b = b ? nb : na;
        switch (pw::lg_host_eval(a, na, b ? b : a, rows_b, dim, u, v, y, m, op, theta, l2, loss, grad, z, &where)) {
            case pw::LG_HOST_U_RANGE: return pair_range("pw_logit_eval", "u", where, u[where], na);
            case pw::LG_HOST_V_RANGE: return pair_range("pw_logit_eval", "v", where, v[where], rows_b);
            case pw::LG_HOST_LABEL: return lg_bad_label(where, y[where]);
            case pw::LG_HOST_Z: return lg_bad_z(where);
            default: break;
        }
        return PW_OK;
    }
    KnnOwner ka, kb;
    if ((rc = knn_own(device, a, na, dim, ka)) || (b && (rc = knn_own(device, b, nb, dim, kb)))) return rc;
    DevBuf<uint32_t> d_u, d_v;
    DevBuf<uint8_t> d_y;
    DevBuf<double> d_z;
    if ((rc = upload(d_u, u, m)) || (v && (rc = upload(d_v, v, m))) || (y && (rc = upload(d_y, y, m))) || (z && (rc = dev_alloc(d_z, m)))) return rc;
    if ((rc = logit_eval_impl(ka.get(), kb.get(), d_u.p, d_v.p, d_y.p, m, op, theta, l2, loss, grad, d_z.p, blocks, nullptr))) return rc;
    return z ? download(z, d_z, m) : PW_OK;
}

PW_EXPORT int pw_selftest_logit_math(int which, const double *x, uint64_t n, double *out) {
    if (which != 0 && which != 1) return fail(PW_ERR_INVALID, "pw_selftest_logit_math: which must be 0 (lg_exp) or 1 (lg_log1p)");
    if (n && (!x || !out)) return fail(PW_ERR_INVALID, "null pointer");
    for (uint64_t i = 0; i < n; i++) out[i] = which == 0 ? pw::lg_exp(x[i]) : pw::lg_log1p(x[i]);
    return PW_OK;
}
