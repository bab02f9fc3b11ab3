#pragma once
// Host driver, self tests of the decision routines of seqscan.h: the exact-arithmetic decision on the host, and the lane
// kernel's per-thread routines on the host and -- in the two kernels defined here -- on the device.
// Exports pw_selftest_exact_decision*, pw_selftest_lane*.
#include "drv_core.hip.h"
#include "seqscan.h"

// ---- host self test of the exact-arithmetic decision ---------------------------------------------------
PW_EXPORT int pw_selftest_exact_decision(const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r,
                                         uint32_t n_r, uint32_t *chain, uint32_t *exact) {
    if (!cls || !r || !chain || !exact || n == 0) return fail(PW_ERR_INVALID, "bad argument");
    auto pow2 = [](float w) { int e = 0; return std::frexp(w, &e) == 0.5f; };
    if (!pow2(w_out) || !pow2(w_prev)) return fail(PW_ERR_UNSUPPORTED, "biases must be powers of two");
    uint32_t cnt[3] = {0, 0, 0};
    for (uint32_t k = 0; k < n; k++) {
        if (cls[k] > 2) return fail(PW_ERR_INVALID, "class must be 0 (out), 1 (common) or 2 (prev)");
        cnt[cls[k]]++;
    }
    if (cnt[2] > 1) return fail(PW_ERR_INVALID, "at most one prev");
    // same set-up as sample_step_unit_lazy (walk_sparse.hip.h)
    float u = 1.0f;
    if (cnt[0] && w_out < u) u = w_out;
    if (cnt[2] && w_prev < u) u = w_prev;
    const double td = (double)cnt[1] + (double)cnt[0] * (double)w_out + (double)cnt[2] * (double)w_prev;
    if (!(td <= 16777216.0 * (double)u)) return fail(PW_ERR_UNSUPPORTED, "row total not exact in float32");
    const float tot = (float)td;
    const float x_in = 1.0f / tot, x_out = x_in * w_out, x_prev = x_in * w_prev;
    const double units = td / (double)u;
    const uint32_t w_units[3] = {cnt[0] ? (uint32_t)(w_out / u) : 1u, (uint32_t)(1.0f / u), cnt[2] ? (uint32_t)(w_prev / u) : 1u};
    const uint32_t wmax = std::max(w_units[0], std::max(w_units[1], w_units[2]));
    std::vector<uint32_t> E(n);
    uint32_t acc = 0;
    for (uint32_t k = 0; k < n; k++) { acc += w_units[cls[k]]; E[k] = acc; }
    for (uint32_t i = 0; i < n_r; i++) {
        // the reference: np.searchsorted(np.cumsum(float32 values), r), sequential float32 additions
        float c = 0.0f;
        uint32_t kc = n;
        for (uint32_t k = 0; k < n; k++) {
            c = c + (cls[k] == 1 ? x_in : (cls[k] == 0 ? x_out : x_prev));
            if ((double)c >= r[i]) { kc = k; break; }
        }
        chain[i] = kc;
        const pw::ExactThresholds th = pw::exact_thresholds_f32(r[i] * units, n, wmax);
        const uint32_t k1 = (uint32_t)(std::lower_bound(E.begin(), E.end(), th.lo) - E.begin());
        exact[i] = (k1 < n && E[k1] >= th.hi) ? k1 : 0xffffffffu;
    }
    return PW_OK;
}

PW_EXPORT int pw_selftest_exact_decision_f64(const uint8_t *cls, uint32_t n, double w_out, double w_prev,
                                             const double *r, uint32_t n_r, uint32_t *chain, uint32_t *exact) {
    if (!cls || !r || !chain || !exact || n == 0) return fail(PW_ERR_INVALID, "bad argument");
    auto pow2 = [](double w) { int e = 0; return std::frexp(w, &e) == 0.5; };
    if (!pow2(w_out) || !pow2(w_prev)) return fail(PW_ERR_UNSUPPORTED, "biases must be powers of two");
    uint64_t cnt[3] = {0, 0, 0};
    for (uint32_t k = 0; k < n; k++) {
        if (cls[k] > 2) return fail(PW_ERR_INVALID, "class must be 0 (out), 1 (common) or 2 (prev)");
        cnt[cls[k]]++;
    }
    if (cnt[2] > 1) return fail(PW_ERR_INVALID, "at most one prev");
    // same set-up as walk_dense_bits_kernel (walk_dense.hip.h)
    double u = 1.0;
    if (cnt[0] && w_out < u) u = w_out;
    if (cnt[2] && w_prev < u) u = w_prev;
    const double tot = (double)cnt[1] + (double)cnt[0] * w_out + (double)cnt[2] * w_prev;
    const double S = tot / u, wi = 1.0 / u, wo = w_out / u, wp = w_prev / u;
    const double wmax = std::max(wi, std::max(wo, wp));
    if (!(S <= 1099511627776.0 && wmax + 2.0 <= 1048576.0)) return fail(PW_ERR_UNSUPPORTED, "row outside the exact range");
    const double x[3] = {w_out / tot, 1.0 / tot, w_prev / tot};
    const uint64_t w_units[3] = {(uint64_t)wo, (uint64_t)wi, (uint64_t)wp};
    std::vector<uint64_t> E(n);
    uint64_t acc = 0;
    for (uint32_t k = 0; k < n; k++) { acc += w_units[cls[k]]; E[k] = acc; }
    for (uint32_t i = 0; i < n_r; i++) {
        double c = 0.0;
        uint32_t kc = n;
        for (uint32_t k = 0; k < n; k++) {
            c = c + x[cls[k]];
            if (c >= r[i]) { kc = k; break; }
        }
        chain[i] = kc;
        const pw::ExactThresholds64 th = pw::exact_thresholds_f64(r[i] * S, (double)n, wmax);
        const uint32_t k1 = (uint32_t)(std::lower_bound(E.begin(), E.end(), th.lo) - E.begin());
        exact[i] = (k1 < n && E[k1] >= th.hi) ? k1 : 0xffffffffu;
    }
    return PW_OK;
}

// ---- self tests of the lane kernel's per-thread routines (seqscan.h: lane_decide, lane_tight, lane_chain) ----------
// One row given by its classes (0 out, 1 common, 2 prev), many targets.  The same routine runs on the host and -- in
// lane_selftest_kernel, one thread per target -- on the DEVICE, where the compiler's code generation and the hardware's
// arithmetic (v_rcp_f32 in lane_tight, -ffp-contract=off adds) are what the walk kernels actually execute.
namespace {

struct LaneRow {
    std::vector<uint16_t> cl16;
    std::vector<uint32_t> cl32;
    uint32_t n_cl = 0, pp = 0xffffffffu, wide = 0;
    uint32_t piv_off = 0;   // element offset of the list's pivots inside cl16 / cl32 (0: none) -- as the index build lays them out
    float tot = 0, x_in = 0, x_out = 0, x_prev = 0;
    pw::ListView view() const { return pw::list_view_of(wide ? (const void *)cl32.data() : (const void *)cl16.data(), wide, n_cl, piv_off); }
};

int lane_row_setup(const uint8_t *cls, uint32_t n, float w_out, float w_prev, LaneRow &row, bool need_pow2 = true) {
    auto pow2 = [](float w) { int e = 0; return std::frexp(w, &e) == 0.5f; };
    if (need_pow2 && (!pow2(w_out) || !pow2(w_prev))) return fail(PW_ERR_UNSUPPORTED, "biases must be powers of two");
    if (!(w_out > 0.0f) || !(w_prev > 0.0f)) return fail(PW_ERR_INVALID, "biases must be positive");
    uint32_t cnt[3] = {0, 0, 0};
    row.wide = n > 65536u ? 1u : 0u;   // positions of rows up to 65536 entries are uint16 (walk_lanes.hip.h)
    for (uint32_t k = 0; k < n; k++) {
        if (cls[k] > 2) return fail(PW_ERR_INVALID, "class must be 0 (out), 1 (common) or 2 (prev)");
        cnt[cls[k]]++;
        if (cls[k] == 1) { if (row.wide) row.cl32.push_back(k); else row.cl16.push_back((uint16_t)k); }
        if (cls[k] == 2) row.pp = k;
    }
    if (cnt[2] > 1) return fail(PW_ERR_INVALID, "at most one prev");
    row.n_cl = cnt[1];
    row.cl16.resize(row.cl16.size() + 8, 0xffffu);       // a list window may read past the end of the list
    row.cl32.resize(row.cl32.size() + 8, 0xffffffffu);
    if (pw::list_has_pivots(row.wide, row.n_cl) && !getenv("PW_SELFTEST_NO_PIVOTS")) {   // pivots, as eline_pivots_kernel writes them
        const uint32_t np = pw::list_pivot_count(row.wide), step = pw::list_pivot_step(row.wide, row.n_cl);
        row.piv_off = (uint32_t)(row.wide ? row.cl32.size() : row.cl16.size());
        for (uint32_t k = 0; k < np; k++) {
            if (row.wide) row.cl32.push_back(row.cl32[(size_t)(k + 1) * step]);
            else row.cl16.push_back(row.cl16[(size_t)(k + 1) * step]);
        }
    }
    row.tot = (float)((double)cnt[1] + (double)cnt[0] * (double)w_out + (double)cnt[2] * (double)w_prev);
    row.x_in = 1.0f / row.tot;
    row.x_out = row.x_in * w_out;
    row.x_prev = row.x_in * w_prev;
    return 0;
}

}  // namespace

namespace pw {
// lane_decide -> lane_tight -> lane_chain for one target; out = { lane, kmax, tight, chain_lane }
PW_HD void lane_selftest_one(uint32_t n, const ListView &cl, uint32_t n_cl, uint32_t pp, float w_out, float w_prev, double r,
                             uint32_t *out) {
    LaneStep ls{0.0f, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t lane = lane_decide(n, n_cl, pp, r, w_out, w_prev, cl, ls);
    out[0] = lane;
    out[1] = lane == LANE_AMBIGUOUS ? ls.kmax : 0u;
    out[2] = lane == LANE_AMBIGUOUS ? lane_tight(n, pp, r, w_out, w_prev, ls) : lane;
    // the per-thread float chain: over the ambiguous prefix, or the whole row when decided
    if (lane == LANE_REDO) { out[3] = LANE_REDO; return; }
    const uint32_t kend = lane == LANE_AMBIGUOUS ? ls.kmax : n;
    const float x_in = 1.0f / ls.tot;
    uint32_t reads = 0;
    out[3] = lane_chain(kend, n_cl, pp, r, x_in, x_in * w_out, x_in * w_prev, cl, reads);
}

__global__ void __launch_bounds__(256)
lane_selftest_kernel(const uint8_t *cls, uint32_t n, const void *cl, uint32_t wide, uint32_t piv_off, uint32_t n_cl, uint32_t pp, float w_out,
                     float w_prev, const double *r, uint32_t n_r, uint32_t *chain, uint32_t *out4) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_r) return;
    // the reference: sequential float32 cumsum + searchsorted (pecanpy.py:556-557), by this thread
    uint32_t cnt_in = 0, cnt_out = 0, cnt_pv = 0;
    for (uint32_t k = 0; k < n; k++) { const uint8_t c = cls[k]; cnt_in += c == 1; cnt_out += c == 0; cnt_pv += c == 2; }
    const float tot = (float)((double)cnt_in + (double)cnt_out * (double)w_out + (double)cnt_pv * (double)w_prev);
    const float x_in = 1.0f / tot, x_out = x_in * w_out, x_prev = x_in * w_prev;
    float c = 0.0f;
    uint32_t kc = n;
    for (uint32_t k = 0; k < n; k++) {
        c = c + (cls[k] == 1 ? x_in : (cls[k] == 0 ? x_out : x_prev));
        if ((double)c >= r[i]) { kc = k; break; }
    }
    chain[i] = kc;
    uint32_t o[4];
    lane_selftest_one(n, list_view_of(cl, wide, n_cl, piv_off), n_cl, pp, w_out, w_prev, r[i], o);
    out4[4 * i] = o[0]; out4[4 * i + 1] = o[1]; out4[4 * i + 2] = o[2]; out4[4 * i + 3] = o[3];
}
}  // namespace pw

namespace pw {
// the FLOATS form of the lane kernel for one target: row total by lane_chain(r = +inf), then the search over w / tot
PW_HD void lane_floats_one(uint32_t n, const ListView &cl, uint32_t n_cl, uint32_t pp, float w_out, float w_prev, double r,
                           uint32_t *choice, float *tot) {
    uint32_t reads = 0;
    float rowsum = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
#else
    const double inf = INFINITY;
#endif
    uint32_t res = lane_chain<true>(n, n_cl, pp, inf, 1.0f, w_out, w_prev, cl, reads, &rowsum);
    *tot = rowsum;
    if (res != LANE_CHAIN_END) { *choice = res; return; }   // (LANE_TIE)
    // round 5: the float64-bounded decision first (what the kernel does with the total from its table), the chain over
    // w / tot only where that leaves the step open
    uint32_t probes = 0, ks = 0;
    const uint32_t b = lane_decide_unit_bounded(n, n_cl, pp, r, rowsum, w_out, w_prev, cl, probes, ks);
    if (b <= n) { *choice = b == n ? LANE_CHAIN_END : b; return; }
    *choice = lane_chain<true>(n, n_cl, pp, r, 1.0f / rowsum, w_out / rowsum, w_prev / rowsum, cl, reads);
}

__global__ void __launch_bounds__(256)
lane_floats_selftest_kernel(const uint8_t *cls, uint32_t n, const void *cl, uint32_t wide, uint32_t piv_off, uint32_t n_cl, uint32_t pp, float w_out,
                            float w_prev, const double *r, uint32_t n_r, uint32_t *chain, uint32_t *lane, float *tots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_r) return;
    float tot = 0.0f;   // the reference: sequential float32 w.sum(), w / tot, cumsum, searchsorted -- by this thread
    for (uint32_t k = 0; k < n; k++) tot = tot + (cls[k] == 1 ? 1.0f : (cls[k] == 0 ? w_out : w_prev));
    const float x_in = 1.0f / tot, x_out = w_out / tot, x_prev = w_prev / tot;
    float c = 0.0f;
    uint32_t kc = n;
    for (uint32_t k = 0; k < n; k++) {
        c = c + (cls[k] == 1 ? x_in : (cls[k] == 0 ? x_out : x_prev));
        if ((double)c >= r[i]) { kc = k; break; }
    }
    chain[i] = kc;
    float tl = 0.0f;
    uint32_t ch = 0;
    lane_floats_one(n, list_view_of(cl, wide, n_cl, piv_off), n_cl, pp, w_out, w_prev, r[i], &ch, &tl);
    lane[i] = ch;
    tots[2 * i] = tot;
    tots[2 * i + 1] = tl;
}
}  // namespace pw

// The FLOATS form of a lane-kernel step (1/p or 1/q not a power of two: arbitrary float32 row values): chain[i] = the
// reference's position for draw r[i] (sequential float32 w.sum(), w / tot, cumsum, searchsorted), lane[i] = the same by
// two closed-form chains of one thread (0xfffffffb: never reached, 0xfffffffa: tie budget), tots[2 i], tots[2 i + 1] =
// the sequential row total and the thread's.  on_device: one GPU thread per target.
PW_EXPORT int pw_selftest_lane_floats(int on_device, int device, const uint8_t *cls, uint32_t n, float w_out, float w_prev,
                                      const double *r, uint32_t n_r, uint32_t *chain, uint32_t *lane, float *tots) {
    if (!cls || !r || !chain || !lane || !tots || n == 0) return fail(PW_ERR_INVALID, "bad argument");
    LaneRow row;
    int rc = lane_row_setup(cls, n, w_out, w_prev, row, false);
    if (rc) return rc;
    if (!on_device) {
        float tot = 0.0f;
        for (uint32_t k = 0; k < n; k++) tot = tot + (cls[k] == 1 ? 1.0f : (cls[k] == 0 ? w_out : w_prev));
        const float x_in = 1.0f / tot, x_out = w_out / tot, x_prev = w_prev / tot;
        std::vector<float> c(n);
        float acc = 0.0f;
        for (uint32_t k = 0; k < n; k++) { acc = acc + (cls[k] == 1 ? x_in : (cls[k] == 0 ? x_out : x_prev)); c[k] = acc; }
        for (uint32_t i = 0; i < n_r; i++) {
            uint32_t lo = 0, hi = n;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((double)c[mid] >= r[i]) hi = mid; else lo = mid + 1; }
            chain[i] = lo;
            float tl = 0.0f;
            pw::lane_floats_one(n, row.view(), row.n_cl, row.pp, w_out, w_prev, r[i], &lane[i], &tl);
            tots[2 * (size_t)i] = tot;
            tots[2 * (size_t)i + 1] = tl;
        }
        return PW_OK;
    }
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint8_t> d_cls;
    DevBuf<void> d_cl;
    DevBuf<double> d_r;
    DevBuf<uint32_t> d_chain, d_lane;
    DevBuf<float> d_tots;
    const size_t cl_bytes = row.wide ? row.cl32.size() * sizeof(uint32_t) : row.cl16.size() * sizeof(uint16_t);
    const void *cl_host = row.wide ? (const void *)row.cl32.data() : (const void *)row.cl16.data();
    const size_t nr = n_r ? n_r : 1;
    hipError_t e = d_cls.alloc(n);
    if (e == hipSuccess) e = d_cl.alloc(cl_bytes);
    if (e == hipSuccess) e = d_r.alloc(nr);
    if (e == hipSuccess) e = d_chain.alloc(nr);
    if (e == hipSuccess) e = d_lane.alloc(nr);
    if (e == hipSuccess) e = d_tots.alloc(2 * nr);
    if (e == hipSuccess) e = hipMemcpy(d_cls.p, cls, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cl.p, cl_host, cl_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_r) e = hipMemcpy(d_r.p, r, sizeof(double) * (size_t)n_r, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_r) {
        hipLaunchKernelGGL(pw::lane_floats_selftest_kernel, dim3((n_r + 255) / 256), dim3(256), 0, 0, d_cls.p, n, d_cl.p, row.wide, row.piv_off, row.n_cl,
                           row.pp, w_out, w_prev, d_r.p, n_r, d_chain.p, d_lane.p, d_tots.p);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(chain, d_chain.p, sizeof(uint32_t) * (size_t)n_r, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(lane, d_lane.p, sizeof(uint32_t) * (size_t)n_r, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(tots, d_tots.p, sizeof(float) * 2 * (size_t)n_r, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_selftest_lane_floats: ") + hipGetErrorString(e));
    return PW_OK;
}

// The bounded decision of the FLOATS form alone (host): lane[i] = lane_decide_unit_bounded's verdict for draw r[i] given the
// row's sequential float32 total -- the position, n (never reached) or 0xfffffffd (left open) -- and chain[i] = the
// reference's position (sequential float32 w.sum(), w / tot, cumsum, searchsorted; n: never reached).
PW_EXPORT int pw_selftest_lane_unit_bounded(const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r, uint32_t n_r,
                                            uint32_t *chain, uint32_t *lane) {
    if (!cls || !r || !chain || !lane || n == 0) return fail(PW_ERR_INVALID, "bad argument");
    LaneRow row;
    int rc = lane_row_setup(cls, n, w_out, w_prev, row, false);
    if (rc) return rc;
    float tot = 0.0f;
    for (uint32_t k = 0; k < n; k++) tot = tot + (cls[k] == 1 ? 1.0f : (cls[k] == 0 ? w_out : w_prev));
    const float x_in = 1.0f / tot, x_out = w_out / tot, x_prev = w_prev / tot;
    std::vector<float> c(n);
    float acc = 0.0f;
    for (uint32_t k = 0; k < n; k++) { acc = acc + (cls[k] == 1 ? x_in : (cls[k] == 0 ? x_out : x_prev)); c[k] = acc; }
    for (uint32_t i = 0; i < n_r; i++) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((double)c[mid] >= r[i]) hi = mid; else lo = mid + 1; }
        chain[i] = lo;
        uint32_t probes = 0, ks = 0;
        lane[i] = pw::lane_decide_unit_bounded(n, row.n_cl, row.pp, r[i], tot, w_out, w_prev, row.view(), probes, ks);
        if (lane[i] > n && lane[i] != pw::LANE_AMBIGUOUS) return fail(PW_ERR_INVALID, "unexpected verdict");
        if (ks > lo) return fail(PW_ERR_INVALID, "k_safe beyond the reference's position");
    }
    return PW_OK;
}

// The FLOATS step with the interval decision in front of the chain (round 6): lane[i] = lane_decide_unit_bounded's verdict,
// tight[i] = that verdict when it is one, else lane_tight_values' (position, or 0xfffffffd: left to the float chain).
PW_EXPORT int pw_selftest_lane_unit_tight(const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r, uint32_t n_r,
                                          uint32_t *chain, uint32_t *lane, uint32_t *tight) {
    if (!cls || !r || !chain || !lane || !tight || n == 0) return fail(PW_ERR_INVALID, "bad argument");
    LaneRow row;
    int rc = lane_row_setup(cls, n, w_out, w_prev, row, false);
    if (rc) return rc;
    float tot = 0.0f;
    for (uint32_t k = 0; k < n; k++) tot = tot + (cls[k] == 1 ? 1.0f : (cls[k] == 0 ? w_out : w_prev));
    const float x_in = 1.0f / tot, x_out = w_out / tot, x_prev = w_prev / tot;
    std::vector<float> c(n);
    float acc = 0.0f;
    for (uint32_t k = 0; k < n; k++) { acc = acc + (cls[k] == 1 ? x_in : (cls[k] == 0 ? x_out : x_prev)); c[k] = acc; }
    for (uint32_t i = 0; i < n_r; i++) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((double)c[mid] >= r[i]) hi = mid; else lo = mid + 1; }
        chain[i] = lo;
        uint32_t probes = 0, ks = 0;
        pw::BoundedAmb amb;
        lane[i] = pw::lane_decide_unit_bounded(n, row.n_cl, row.pp, r[i], tot, w_out, w_prev, row.view(), probes, ks, &amb);
        if (lane[i] > n && lane[i] != pw::LANE_AMBIGUOUS) return fail(PW_ERR_INVALID, "unexpected verdict");
        if (ks > lo) return fail(PW_ERR_INVALID, "k_safe beyond the reference's position");
        tight[i] = lane[i];
        if (lane[i] == pw::LANE_AMBIGUOUS && ks > 0) tight[i] = pw::lane_tight_values(n, row.pp, r[i], x_in, x_out, x_prev, ks, amb.f, amb.p_next, amb.z_abs);
    }
#if !defined(__HIP_DEVICE_COMPILE__)
    if (getenv("PW_TIGHT_STATS")) {
        fprintf(stderr, "tight bail reasons:");
        for (int k = 1; k < 24; k++) if (pw::g_tight_reason[k]) fprintf(stderr, " [%d]=%llu", k, (unsigned long long)pw::g_tight_reason[k]);
        fprintf(stderr, "\n");
    }
#endif
    return PW_OK;
}

PW_EXPORT int pw_selftest_lane(int on_device, int device, const uint8_t *cls, uint32_t n, float w_out, float w_prev, const double *r,
                               uint32_t n_r, uint32_t *chain, uint32_t *lane, uint32_t *kmax, uint32_t *tight,
                               uint32_t *chain_lane) {
    if (!cls || !r || !chain || !lane || !kmax || !tight || n == 0) return fail(PW_ERR_INVALID, "bad argument");
    LaneRow row;
    int rc = lane_row_setup(cls, n, w_out, w_prev, row);
    if (rc) return rc;
    if (!on_device) {
        // the chain once: prefix sums, then one binary search per draw (the sums are non-decreasing)
        std::vector<float> c(n);
        float acc = 0.0f;
        for (uint32_t k = 0; k < n; k++) {
            acc = acc + (cls[k] == 1 ? row.x_in : (cls[k] == 0 ? row.x_out : row.x_prev));
            c[k] = acc;
        }
        for (uint32_t i = 0; i < n_r; i++) {
            uint32_t lo = 0, hi = n;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((double)c[mid] >= r[i]) hi = mid; else lo = mid + 1; }
            chain[i] = lo;
            uint32_t o[4];
            pw::lane_selftest_one(n, row.view(), row.n_cl, row.pp, w_out, w_prev, r[i], o);
            lane[i] = o[0]; kmax[i] = o[1]; tight[i] = o[2];
            if (chain_lane) chain_lane[i] = o[3];
        }
#if !defined(__HIP_DEVICE_COMPILE__)
        if (getenv("PW_TIGHT_STATS")) {
            fprintf(stderr, "tight bail reasons:");
            for (int k = 1; k < 24; k++) if (pw::g_tight_reason[k]) fprintf(stderr, " [%d]=%llu", k, (unsigned long long)pw::g_tight_reason[k]);
            fprintf(stderr, "\n");
        }
#endif
        return PW_OK;
    }
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint8_t> d_cls;
    DevBuf<void> d_cl;
    DevBuf<double> d_r;
    DevBuf<uint32_t> d_chain, d_out;
    const size_t cl_bytes = row.wide ? row.cl32.size() * sizeof(uint32_t) : row.cl16.size() * sizeof(uint16_t);
    const void *cl_host = row.wide ? (const void *)row.cl32.data() : (const void *)row.cl16.data();
    hipError_t e = d_cls.alloc(n);
    if (e == hipSuccess) e = d_cl.alloc(cl_bytes);
    if (e == hipSuccess) e = d_r.alloc(n_r);
    if (e == hipSuccess) e = d_chain.alloc(n_r);
    if (e == hipSuccess) e = d_out.alloc(4 * (size_t)n_r);
    if (e == hipSuccess) e = hipMemcpy(d_cls.p, cls, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cl.p, cl_host, cl_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_r) e = hipMemcpy(d_r.p, r, sizeof(double) * (size_t)n_r, hipMemcpyHostToDevice);
    std::vector<uint32_t> out4((size_t)4 * n_r);
    if (e == hipSuccess && n_r) {
        hipLaunchKernelGGL(pw::lane_selftest_kernel, dim3((n_r + 255) / 256), dim3(256), 0, 0, d_cls.p, n, d_cl.p, row.wide, row.piv_off, row.n_cl, row.pp,
                           w_out, w_prev, d_r.p, n_r, d_chain.p, d_out.p);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(chain, d_chain.p, sizeof(uint32_t) * (size_t)n_r, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(out4.data(), d_out.p, sizeof(uint32_t) * 4 * (size_t)n_r, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_selftest_lane: ") + hipGetErrorString(e));
    for (uint32_t i = 0; i < n_r; i++) {
        lane[i] = out4[4 * (size_t)i]; kmax[i] = out4[4 * (size_t)i + 1]; tight[i] = out4[4 * (size_t)i + 2];
        if (chain_lane) chain_lane[i] = out4[4 * (size_t)i + 3];
    }
    return PW_OK;
}

// The weighted-row decision of the lane kernel (seqscan.h: lane_decide_weighted) on a host row, beside the reference's
// sequential float32 chain.  vals[k] = the step's value of neighbour k before normalisation, base[k] = its base value
// (what it would be as a plain "out" neighbour), cls[k] = 0 other (vals == base) / 1 common neighbour / 2 prev.
PW_EXPORT int pw_selftest_lane_weighted(const float *vals, const float *base, const uint8_t *cls, uint32_t n, const double *r,
                                        uint32_t n_r, uint32_t *chain, uint32_t *lane) {
    if (!vals || !base || !cls || !r || !chain || !lane || n == 0) return fail(PW_ERR_INVALID, "bad argument");
    float tot = 0.0f;
    for (uint32_t k = 0; k < n; k++) tot = tot + vals[k];                     // sequential float32 w.sum()
    std::vector<float> c(n);
    float acc = 0.0f;
    for (uint32_t k = 0; k < n; k++) { acc = acc + vals[k] / tot; c[k] = acc; }   // cumsum of fl32(w / tot)
    std::vector<pw::PrefixPair> pq(n);
    std::vector<double> dl;
    double trun = 0.0;
    bool any_pos = false, any_neg = false;
    std::vector<uint16_t> cl16;
    std::vector<uint32_t> cl32;
    const uint32_t wide = n > 65536u ? 1u : 0u;
    double run = 0.0, drun = 0.0, dprev = 0.0;
    uint32_t pp = 0xffffffffu;
    for (uint32_t k = 0; k < n; k++) {
        run += (double)base[k];
        trun += run;
        pq[k] = pw::PrefixPair{run, trun};
        if (cls[k] == 1) {
            if (vals[k] > base[k]) any_pos = true;
            if (vals[k] < base[k]) any_neg = true;
            drun += (double)vals[k] - (double)base[k];
            dl.push_back(drun);
            if (wide) cl32.push_back(k); else cl16.push_back((uint16_t)k);
        } else if (cls[k] == 2) {
            if (pp != 0xffffffffu) return fail(PW_ERR_INVALID, "at most one prev");
            pp = k;
            dprev = (double)vals[k] - (double)base[k];
        } else if (cls[k] != 0 || vals[k] != base[k]) return fail(PW_ERR_INVALID, "class 0 elements carry their base value");
    }
    const uint32_t n_cl = (uint32_t)dl.size();
    cl16.resize(cl16.size() + 8, 0xffffu);
    cl32.resize(cl32.size() + 8, 0xffffffffu);
    uint32_t piv_off = 0;
    if (pw::list_has_pivots(wide, n_cl)) {
        const uint32_t np = pw::list_pivot_count(wide), step = pw::list_pivot_step(wide, n_cl);
        piv_off = (uint32_t)(wide ? cl32.size() : cl16.size());
        for (uint32_t k = 0; k < np; k++) { if (wide) cl32.push_back(cl32[(size_t)(k + 1) * step]); else cl16.push_back(cl16[(size_t)(k + 1) * step]); }
    }
    dl.push_back(0.0);
    const pw::ListView view = pw::list_view_of(wide ? (const void *)cl32.data() : (const void *)cl16.data(), wide, n_cl, piv_off);
    if (any_pos && any_neg) return fail(PW_ERR_INVALID, "the common neighbours' differences must share one sign (that of q - 1)");
    const pw::WeightedRow wr{pq.data(), dl.data(), dprev, !any_neg};
    for (uint32_t i = 0; i < n_r; i++) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((double)c[mid] >= r[i]) hi = mid; else lo = mid + 1; }
        chain[i] = lo;
        uint32_t probes = 0, k_safe = 0;
        lane[i] = pw::lane_decide_weighted(n, n_cl, pp, r[i], tot, wr, view, probes, k_safe);
        if (k_safe > chain[i]) return fail(PW_ERR_INVALID, "lane_decide_weighted: k_safe beyond the chain's position");
    }
    return PW_OK;
}
