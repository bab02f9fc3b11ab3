// logit.hip.h -- exact binary logistic regression on embedding rows and pair operators (gfx950): one evaluation of the loss, its
// gradient and the decision values.  pw_logit_eval_device, pw_logit_eval_device_grid, pw_selftest_logit, pw_selftest_logit_math.
//
// THE DEFINITION (the whole contract; DESIGN.md 4.12 repeats it).
//
//   inputs      A float32[na, dim] and B float32[nb, dim] (B = A when no second index is given): two pw_knn indexes, so every
//               value is finite.  u, v uint32[m]; y uint8[m], every value 0 or 1; op; theta float64[dim + 1] = (w[0] ..
//               w[dim - 1], bias); l2 finite and >= 0.  1 <= m < 2^40.  1 <= dim <= 512 (LG_MAX_DIM, the trainer's cap: the
//               gradient kernel keeps a chunk's partial row in registers); a larger dim is PW_ERR_UNSUPPORTED.
//
//   feature     f = feat(op, a, b), a = A[u[i]][k], b = B[v[i]][k], in float64 on the float32 values widened:
//                   row       a                    (v is ignored, not even range-checked)      no rounding
//                   average   (a + b) * 0.5                                                    one rounding
//                   hadamard  a * b                                                            none: the product is exact
//                   l1        fabs(a - b)                                                      one
//                   l2        (a - b) * (a - b)                                                two
//
//   decision    z[i] = (((bias + w[0] f[0]) + w[1] f[1]) + ...), k ascending; every product and every sum rounded on its own
//               (no fused multiply-add, on the device either: w is a double, so the product is not exact).  A z that is no
//               finite number is refused, naming the first such sample.
//
//   functions   from + - * /, rint and a power of two built from the exponent bits alone, each operation rounded separately
//               (libm's and the device's exp / log1p do not agree in the last bit; these do, by construction):
//               lg_exp(x), x in [-708, 0]:  k = rint(x * log2e);  r = (x - k * ln2_hi) - k * ln2_lo  (fdlibm's split of ln 2);
//                   p = the Taylor polynomial of e^r of degree 13 by Horner, the coefficients 1/n! as literals;  p * 2^k.
//                   x < -708 gives +0.0.  (k >= -1021 and p >= 0.7: the result is a normal number.)
//               lg_log1p(t), t in [0, 1]:  s = t / (2 + t);  w = s * s;  (2 s) * (1 + w/3 + w^2/5 + ... + w^15/31) by Horner,
//                   the coefficients 1.0 / (2 n + 1).  SIXTEEN terms (LG_LOG1P_TERMS): at t = 1, s = 1/3, the terms left out
//                   add up to 1.22e-17 = 0.22 of half an ulp of ln 2 (2^-54); fifteen would leave 2.1 half ulps.
//
//   sample      x = y[i] ? -z[i] : z[i]  (= -(2 y - 1) z);  t = lg_exp(-fabs(x));
//               q = x >= 0 ? 1 / (1 + t) : t / (1 + t)      the probability of the WRONG label: no 1 - p cancellation
//               r[i] = y[i] ? -q : q                        (= -(2 y - 1) q: d loss / d z)
//               l[i] = (x > 0 ? x : +0.0) + lg_log1p(t)
//
//   sums        LG_CHUNK = 1024 is part of the definition.  Chunk c is the samples [1024 c, min(m, 1024 (c + 1))).  Inside a
//               chunk, from +0.0, i ascending:  P[c][k] += r[i] * f[i][k] (the product rounded, then the sum),
//               P[c][dim] += r[i],  PL[c] += l[i].  The totals G[k], Lsum: the chunks' values added with c ascending from +0.0.
//
//   outputs     grad[k] = G[k] / (double)m + l2 * w[k] for k < dim;  grad[dim] = G[dim] / (double)m (the bias is not penalised);
//               loss = Lsum / (double)m + (0.5 * l2) * (((0 + w[0] w[0]) + w[1] w[1]) + ...).  Optionally z[m].  Without y the
//               call computes z alone: scoring with a trained model.
//
//   refusals    everything is checked before anything is written, in this order: an unknown op; dims or devices of A and B
//               that differ; dim above the cap; m out of range; l2 negative or NaN or infinite; the first non-finite theta
//               entry; the first position with a row number out of range (u before v at one position); the first label that
//               is neither 0 nor 1; the first z that is not finite.
// No result depends on the grid, the tiling, the number of wavefronts, or which form ran.
//
// The definition is written once -- lg_feat, lg_zstep, lg_exp, lg_log1p, lg_sample, lg_finish -- for host and device; lg_host_*
// run it with plain loops (pw_selftest_logit with on_device = 0), and that half of the file compiles with a plain C++ compiler.
//
// The device form (no floating-point atomic anywhere):
//   lg_check_kernel     the lowest position with a row number out of range and the lowest with a bad label, by integer
//                       atomic minima
//   lg_forward_kernel   lp_score_pairs_kernel's shape: a WAVEFRONT takes 64 samples and owns a piece of LDS, no workgroup
//                       barrier; it stages both rows of each sample 32 columns at a time (36-float stride) and each lane runs
//                       its own sample's chain.  w is wavefront-uniform and arrives by scalar loads.  Writes z[i], r[i], l[i];
//                       an integer atomic minimum records the first z that is not finite.
//   lg_grad_kernel      a wavefront takes one chunk at a time, persistent over the chunks of its grid stride.  A lane owns the
//                       columns 2 lane + 128 j and 2 lane + 1 + 128 j (j < 4: eight per lane at dim 512).  The row numbers,
//                       r[i] and l[i] of the chunk are wavefront-uniform (scalar loads); per sample the lanes read both rows
//                       coalesced, the loads of LG_AHEAD samples issued ahead of the accumulation (the kernel is gather
//                       bound), which itself runs in sample order.  The partial rows go to a scratch [n_chunks, dim + 2]:
//                       columns dim and dim + 1 hold the sum of r and PL[c].
//   lg_reduce_kernel    one lane per column of the scratch, c ascending.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

#include "knn.hip.h"
#include "linkpred.hip.h"

namespace pw {

constexpr int LG_ROW = 0, LG_AVERAGE = 1, LG_HADAMARD = 2, LG_L1 = 3, LG_L2 = 4, LG_OPS = 5;   // PW_LOGIT_*
constexpr uint32_t LG_MAX_DIM = 512;
constexpr uint32_t LG_CHUNK = 1024;
constexpr uint64_t LG_MAX_M = 1ull << 40;   // m < LG_MAX_M
constexpr int LG_LOG1P_TERMS = 16;

// ---- the definition --------------------------------------------------------------------------------------------------
PW_KNN_HD double lg_feat(int op, float a32, float b32) {
    const double a = (double)a32, b = (double)b32;
    switch (op) {
        case LG_ROW: return a;
        case LG_AVERAGE: return (a + b) * 0.5;
        case LG_HADAMARD: return a * b;
        case LG_L1: return fabs(a - b);
        default: { const double d = a - b; return d * d; }
    }
}

// one step of the decision value's chain: the product rounded, then the sum
PW_KNN_HD double lg_zstep(double acc, double w, double f) {
    const double p = w * f;
    return acc + p;
}

PW_KNN_HD double lg_pow2(int k) {   // 2^k for -1022 <= k <= 1023, from the exponent bits
    const uint64_t b = (uint64_t)(k + 1023) << 52;
    double d;
    __builtin_memcpy(&d, &b, sizeof(d));
    return d;
}

PW_KNN_HD double lg_exp(double x) {
    if (x < -708.0) return 0.0;
    const double k = rint(x * 1.4426950408889634);
    const double hi = k * 6.93147180369123816490e-01, lo = k * 1.90821492927058770002e-10;
    const double r = (x - hi) - lo;
    double p = 1.6059043836821613e-10;          // 1/13!
    p = p * r + 2.08767569878681e-09;           // 1/12!
    p = p * r + 2.505210838544172e-08;          // 1/11!
    p = p * r + 2.755731922398589e-07;          // 1/10!
    p = p * r + 2.7557319223985893e-06;         // 1/9!
    p = p * r + 2.48015873015873e-05;           // 1/8!
    p = p * r + 0.0001984126984126984;          // 1/7!
    p = p * r + 0.001388888888888889;           // 1/6!
    p = p * r + 0.008333333333333333;           // 1/5!
    p = p * r + 0.041666666666666664;           // 1/4!
    p = p * r + 0.16666666666666666;            // 1/3!
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * lg_pow2((int)k);
}

PW_KNN_HD double lg_log1p(double t) {
    const double s = t / (2.0 + t), w = s * s;
    double q = 1.0 / 31.0;
    q = q * w + 1.0 / 29.0;
    q = q * w + 1.0 / 27.0;
    q = q * w + 1.0 / 25.0;
    q = q * w + 1.0 / 23.0;
    q = q * w + 1.0 / 21.0;
    q = q * w + 1.0 / 19.0;
    q = q * w + 1.0 / 17.0;
    q = q * w + 1.0 / 15.0;
    q = q * w + 1.0 / 13.0;
    q = q * w + 1.0 / 11.0;
    q = q * w + 1.0 / 9.0;
    q = q * w + 1.0 / 7.0;
    q = q * w + 1.0 / 5.0;
    q = q * w + 1.0 / 3.0;
    q = q * w + 1.0;
    return (2.0 * s) * q;
}

// the residual r = d loss / d z and the loss of one sample with label y (0 / 1) and decision value z
PW_KNN_HD void lg_sample(double z, uint32_t y, double *r, double *ell) {
    const double x = y ? -z : z;
    const double t = lg_exp(-fabs(x));
    const double den = 1.0 + t;
    const double q = x >= 0.0 ? 1.0 / den : t / den;
    *r = y ? -q : q;
    *ell = (x > 0.0 ? x : 0.0) + lg_log1p(t);
}

// G: the totals, dim + 2 of them (columns, the sum of r, the sum of the losses)
inline void lg_finish(const double *G, uint32_t dim, uint64_t m, const double *theta, double l2, double *loss, double *grad) {
    const double dm = (double)m;
    double pen = 0.0;
    for (uint32_t k = 0; k < dim; k++) {
        const double pull = l2 * theta[k], sq = theta[k] * theta[k];
        grad[k] = G[k] / dm + pull;
        pen = pen + sq;
    }
    grad[dim] = G[dim] / dm;
    const double reg = (0.5 * l2) * pen;
    *loss = G[dim + 1] / dm + reg;
}

// ---- the host forms: plain loops over the definition --------------------------------------------------------------
enum LgHostResult { LG_HOST_OK = 0, LG_HOST_U_RANGE = 1, LG_HOST_V_RANGE = 2, LG_HOST_LABEL = 3, LG_HOST_Z = 4 };

PW_KNN_HD bool lg_op_known(int op) { return op >= 0 && op < LG_OPS; }
PW_KNN_HD bool lg_l2_valid(double l2) { return knn_finite(l2) && l2 >= 0.0; }

// the first non-finite entry of theta[0, dim]; dim + 1: none
inline uint32_t lg_host_theta_bad(const double *theta, uint32_t dim) {
    for (uint32_t k = 0; k <= dim; k++)
        if (!knn_finite(theta[k])) return k;
    return dim + 1;
}

// rows first (the first position, u before v), then labels (y may be null: decision values alone)
inline int lg_host_check(const uint32_t *u, const uint32_t *v, const uint8_t *y, uint64_t m, uint64_t na, uint64_t nb, int op, uint64_t *where) {
    for (uint64_t i = 0; i < m; i++) {
        if (u[i] >= na) { *where = i; return LG_HOST_U_RANGE; }
        if (op != LG_ROW && v[i] >= nb) { *where = i; return LG_HOST_V_RANGE; }
    }
    for (uint64_t i = 0; y && i < m; i++)
        if (y[i] > 1) { *where = i; return LG_HOST_LABEL; }
    return LG_HOST_OK;
}

inline double lg_host_z(const float *a, const float *b, uint32_t dim, int op, const double *theta) {
    double z = theta[dim];
    for (uint32_t k = 0; k < dim; k++) z = lg_zstep(z, theta[k], lg_feat(op, a[k], op == LG_ROW ? 0.f : b[k]));
    return z;
}

// op, l2, theta, dim and m are the caller's to check (they need no data).  y null: z alone (z must be given then); otherwise
// loss, grad[dim + 1] and, when z is given, z[m].  Nothing is written on a refusal.
inline int lg_host_eval(const float *A, uint64_t na, const float *B, uint64_t nb, uint32_t dim, const uint32_t *u, const uint32_t *v, const uint8_t *y,
                        uint64_t m, int op, const double *theta, double l2, double *loss, double *grad, double *z, uint64_t *where) {
    if (int rc = lg_host_check(u, v, y, m, na, nb, op, where)) return rc;
    std::vector<double> zs(m);
    for (uint64_t i = 0; i < m; i++) {
        zs[i] = lg_host_z(A + (uint64_t)u[i] * dim, op == LG_ROW ? nullptr : B + (uint64_t)v[i] * dim, dim, op, theta);
        if (!knn_finite(zs[i])) { *where = i; return LG_HOST_Z; }
    }
    if (y) {
        std::vector<double> G(dim + 2, 0.0), P(dim + 2);
        for (uint64_t i0 = 0; i0 < m; i0 += LG_CHUNK) {
            const uint64_t i1 = i0 + LG_CHUNK < m ? i0 + LG_CHUNK : m;
            for (auto &p : P) p = 0.0;
            for (uint64_t i = i0; i < i1; i++) {
                double r, ell;
                lg_sample(zs[i], y[i], &r, &ell);
                const float *a = A + (uint64_t)u[i] * dim, *b = op == LG_ROW ? nullptr : B + (uint64_t)v[i] * dim;
                for (uint32_t k = 0; k < dim; k++) {
                    const double prod = r * lg_feat(op, a[k], op == LG_ROW ? 0.f : b[k]);
                    P[k] = P[k] + prod;
                }
                P[dim] = P[dim] + r;
                P[dim + 1] = P[dim + 1] + ell;
            }
            for (uint32_t k = 0; k < dim + 2; k++) G[k] = G[k] + P[k];
        }
        lg_finish(G.data(), dim, m, theta, l2, loss, grad);
    }
    if (z)
        for (uint64_t i = 0; i < m; i++) z[i] = zs[i];
    return LG_HOST_OK;
}

}  // namespace pw

// ---- the device form -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "wave.h"

namespace pw {

constexpr uint32_t LG_FWD_WAVES = 2;                     // wavefronts of a forward workgroup, each with its own 64 samples
constexpr uint32_t LG_FWD_THREADS = LG_FWD_WAVES * WAVE;
constexpr uint32_t LG_GRAD_WAVES = 4;                    // wavefronts of a gradient workgroup, each with its own chunk
constexpr uint32_t LG_GRAD_THREADS = LG_GRAD_WAVES * WAVE;
constexpr uint32_t LG_COLS = 2 * WAVE;                   // columns a wavefront covers per j
constexpr int LG_AHEAD = 8;                              // samples whose rows are in flight before the accumulation

struct LgFound {   // what the check passes report, by integer atomics; ~0: none
    unsigned long long row, label, z;
};

__global__ __launch_bounds__(256) void lg_check_kernel(const uint32_t *__restrict__ u, const uint32_t *__restrict__ v, const uint8_t *__restrict__ y,
                                                       uint64_t m, uint64_t na, uint64_t nb, int op, LgFound *found) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        if (u[i] >= na || (op != LG_ROW && v[i] >= nb)) atomicMin(&found->row, (unsigned long long)i);
        if (y && y[i] > 1) atomicMin(&found->label, (unsigned long long)i);
    }
}

struct LgFwdArgs {
    const float *A, *B;          // [na, dim], [nb, dim]
    const uint32_t *u, *v;       // [m], checked (v unused by LG_ROW)
    const uint8_t *y;            // [m], checked; null: z alone
    const double *theta;         // [dim + 1] in device memory
    double *z, *r, *ell;         // [m] each; z may be null when y is given, r / ell are null when it is not
    LgFound *found;
    uint64_t m, n_tiles;         // samples; tiles of 64 samples
    uint32_t dim;
};

template <int OP>
__global__ __launch_bounds__(LG_FWD_THREADS) void lg_forward_kernel(const LgFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float rows_lds[LG_FWD_WAVES][2 * WAVE * LP_STRIDE];
    __shared__ uint32_t idx_lds[LG_FWD_WAVES][2 * WAVE];
    constexpr uint32_t N_ROWS = OP == LG_ROW ? WAVE : 2 * WAVE;   // staged rows of a tile
    const uint32_t w = readfirst_u32(threadIdx.x >> 6), lane = (uint32_t)lane_id();
    float *tile = rows_lds[w];
    uint32_t *idx = idx_lds[w];
    const bool vec4 = (a.dim & 3u) == 0;   // (A and B are the indexes' own allocations: 16-byte aligned)
    const float *my_u = tile + (size_t)lane * LP_STRIDE, *my_v = tile + (size_t)(WAVE + lane) * LP_STRIDE;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LG_FWD_WAVES + w, n_waves = (uint64_t)gridDim.x * LG_FWD_WAVES;
    sptr<double> th = as_scalar<double>((uint64_t)a.theta);

    for (uint64_t t = wave0; t < a.n_tiles; t += n_waves) {   // (wavefront-uniform)
        const uint64_t i = t * WAVE + lane;
        const bool valid = i < a.m;
        const uint32_t ru = valid ? a.u[i] : 0u, rv = (valid && OP != LG_ROW) ? a.v[i] : 0u;   // (row 0 exists: n >= 1)
        wave_lds_fence();   // the tile before has been read
        idx[lane] = ru;
        idx[WAVE + lane] = rv;
        double acc = th[a.dim];
        for (uint32_t k0 = 0; k0 < a.dim; k0 += LP_KC) {
            const uint32_t kcur = min(LP_KC, a.dim - k0), kc4 = (kcur + 3) >> 2;
            wave_lds_fence();   // the chunk before has been read; the row numbers are in place
            for (uint32_t e = lane; e < N_ROWS * kc4; e += WAVE) {
                const uint32_t r = e / kc4, c = (e - r * kc4) << 2;
                const uint32_t col = k0 + c;
                const float *src = (r < WAVE ? a.A : a.B) + (uint64_t)idx[r] * a.dim + col;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (vec4) {
                    x = *(const float4 *)src;
                } else {
                    x.x = src[0];
                    if (col + 1 < a.dim) x.y = src[1];
                    if (col + 2 < a.dim) x.z = src[2];
                    if (col + 3 < a.dim) x.w = src[3];
                }
                *(float4 *)(tile + (size_t)r * LP_STRIDE + c) = x;
            }
            wave_lds_fence();
            sptr<double> wk = th + k0;
            for (uint32_t kk = 0; kk < kc4; kk++) {   // (a padded column takes no step: z + 0 would turn a -0.0 into +0.0)
                const uint32_t c = kk << 2;
                const float4 x = *(const float4 *)(my_u + c);
                float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
                if (OP != LG_ROW) y = *(const float4 *)(my_v + c);
                acc = lg_zstep(acc, wk[c], lg_feat(OP, x.x, y.x));
                if (c + 1 < kcur) acc = lg_zstep(acc, wk[c + 1], lg_feat(OP, x.y, y.y));
                if (c + 2 < kcur) acc = lg_zstep(acc, wk[c + 2], lg_feat(OP, x.z, y.z));
                if (c + 3 < kcur) acc = lg_zstep(acc, wk[c + 3], lg_feat(OP, x.w, y.w));
            }
        }
        if (valid) {
            if (!knn_finite(acc)) atomicMin(&a.found->z, (unsigned long long)i);
            if (a.z) a.z[i] = acc;
            if (a.y) {
                double r, ell;
                lg_sample(acc, a.y[i], &r, &ell);
                a.r[i] = r;
                a.ell[i] = ell;
            }
        }
    }
}

struct LgGradArgs {
    const float *A, *B;
    const uint32_t *u, *v;       // [m]
    const double *r, *ell;       // [m], what the forward kernel wrote
    double *part;                // [n_chunks, dim + 2]
    uint64_t m, n_chunks;
    uint32_t dim;
};

// NJ = ceil(dim / 128) column pairs per lane
template <int OP, int NJ>
__global__ __launch_bounds__(LG_GRAD_THREADS) void lg_grad_kernel(const LgGradArgs a) {
    constexpr int AHEAD = NJ > 2 ? LG_AHEAD / 2 : LG_AHEAD;
    const uint32_t w = readfirst_u32(threadIdx.x >> 6), lane = (uint32_t)lane_id();
    const uint64_t wave0 = (uint64_t)blockIdx.x * LG_GRAD_WAVES + w, n_waves = (uint64_t)gridDim.x * LG_GRAD_WAVES;
    const bool even = (a.dim & 1u) == 0;   // (rows start 8-byte aligned: 8-byte loads)
    const uint32_t stride = a.dim + 2;
    sptr<uint32_t> su = as_scalar<uint32_t>((uint64_t)a.u), sv = as_scalar<uint32_t>((uint64_t)a.v);
    sptr<double> sr = as_scalar<double>((uint64_t)a.r), sl = as_scalar<double>((uint64_t)a.ell);
    bool has0[NJ], has1[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const uint32_t col = 2 * lane + LG_COLS * j;
        has0[j] = col < a.dim;
        has1[j] = col + 1 < a.dim;
    }

    for (uint64_t c = wave0; c < a.n_chunks; c += n_waves) {   // (wavefront-uniform)
        const uint64_t i0 = c * LG_CHUNK;
        const uint32_t n = (uint32_t)min((uint64_t)LG_CHUNK, a.m - i0);
        double acc0[NJ], acc1[NJ], acc_r = 0.0, acc_l = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; j++) acc0[j] = acc1[j] = 0.0;
        for (uint32_t s = 0; s < n; s += AHEAD) {
            float2 xa[AHEAD][NJ], xb[AHEAD][NJ];
#pragma unroll
            for (int b = 0; b < AHEAD; b++) {
                if (s + b < n) {   // (wavefront-uniform)
                    const uint64_t i = i0 + s + b;
                    const float *pa = a.A + (uint64_t)su[i] * a.dim + 2 * lane;
                    const float *pb = OP != LG_ROW ? a.B + (uint64_t)sv[i] * a.dim + 2 * lane : nullptr;
#pragma unroll
                    for (int j = 0; j < NJ; j++) {
                        float2 x = make_float2(0.f, 0.f), y = make_float2(0.f, 0.f);
                        if (even) {
                            if (has0[j]) {
                                x = *(const float2 *)(pa + LG_COLS * j);
                                if (OP != LG_ROW) y = *(const float2 *)(pb + LG_COLS * j);
                            }
                        } else {
                            if (has0[j]) { x.x = pa[LG_COLS * j]; if (OP != LG_ROW) y.x = pb[LG_COLS * j]; }
                            if (has1[j]) { x.y = pa[LG_COLS * j + 1]; if (OP != LG_ROW) y.y = pb[LG_COLS * j + 1]; }
                        }
                        xa[b][j] = x;
                        xb[b][j] = y;
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < AHEAD; b++) {
                if (s + b < n) {
                    const uint64_t i = i0 + s + b;
                    const double r = sr[i];
#pragma unroll
                    for (int j = 0; j < NJ; j++) {   // (columns past dim hold zeros and are never written)
                        const double p0 = r * lg_feat(OP, xa[b][j].x, xb[b][j].x), p1 = r * lg_feat(OP, xa[b][j].y, xb[b][j].y);
                        acc0[j] = acc0[j] + p0;
                        acc1[j] = acc1[j] + p1;
                    }
                    acc_r = acc_r + r;
                    acc_l = acc_l + sl[i];
                }
            }
        }
        double *out = a.part + c * stride;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const uint32_t col = 2 * lane + LG_COLS * j;
            if (has0[j]) out[col] = acc0[j];
            if (has1[j]) out[col + 1] = acc1[j];
        }
        if (lane == 0) {
            out[a.dim] = acc_r;
            out[a.dim + 1] = acc_l;
        }
    }
}

// totals[t] = the chunks' part[c][t] added with c ascending from +0.0, one lane per column t < n_cols
__global__ __launch_bounds__(64) void lg_reduce_kernel(const double *__restrict__ part, uint64_t n_chunks, uint32_t n_cols, double *__restrict__ totals) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cols) return;
    double acc = 0.0;
    uint64_t c = 0;
    for (; c + 8 <= n_chunks; c += 8) {
        double x[8];
#pragma unroll
        for (int b = 0; b < 8; b++) x[b] = part[(c + b) * n_cols + t];
#pragma unroll
        for (int b = 0; b < 8; b++) acc = acc + x[b];
    }
    for (; c < n_chunks; c++) acc = acc + part[c * n_cols + t];
    totals[t] = acc;
}

}  // namespace pw
#endif
