// walk_sparse_pp.hip.h -- node2vec++ on a CSR graph (PW_MODE_SPARSE_NODE2VEC_PLUSPLUS): the dense kernel's float64-bounded
// decision with a sparse source for data[prev, x] (gfx950).
//
// The contract: walks, probabilities and steps equal the reference's experimental.Node2vecPlusPlus run on
// A.toarray().astype(np.float64).  That dense reference walks the non-zeros of cur's row in column order, which is CSR order,
// so the step is walk_dense_weighted_kernel<DW_N2VPP>'s step (walk_dense_w.hip.h) with three sources replaced:
//   * cur's row: kf[e] = { column, filter word } (walk_sparse.hip.h, CsrDev::kf) and the float32 weight, widened in registers.
//   * data[prev, x]: the dense kernel tests bit x of prev's packed row in LDS (N / 8 bytes: impossible at N = 10^6) and
//     gathers by rank.  Here prev's membership filter (one 8-byte word, rows' words ordered like the keys) rejects most
//     non-neighbours; a survivor is looked up in prev's adjacency index (slots: one probe, rarely two), and its position
//     gives the float32 weight of prev's row.  vrec[prev] names all three in one 16-byte load.  A column whose threshold is
//     not > 0 (or NaN) is never an out edge: no lookup at all.
//     (A cooperative merge of the two sorted rows was considered: it reads all of prev's row every step -- a hub prev costs
//     its whole degree for each of its low-degree neighbours -- where the filter reads one word per element of cur's row.)
//   * the block prefixes: a fixed LDS array of SPP_PCAP entries.  A row of more than SPP_PCAP blocks groups SB consecutive
//     blocks into one super-block and keeps the prefixes of the super-blocks; the decision scans the super-block that holds
//     the target (SB blocks instead of one).  No row length is too long, and the LDS does not grow with the degree.
// The bias, the two loops and the bound are the dense kernel's (DenseWStep::pp_value, dw_chain_decide).  With super-blocks
// the block scan adds at most SB * B - 1 chunk sums instead of B - 1, so the bound of walk_dense_w.hip.h becomes
//     E = (2 n + 2 nblk + (SB + 2) B + 20) u (1 + 2^-20)   (SB = 1: the dense kernel's E)
// and the decision is exact for the same reasons: every finite value is >= 0, non-finite values and partial sums inside
// [T (1 - E), T (1 + E)) go to the reference's two loops in place, a draw no partial sum reaches takes the last neighbour.
//
// Declared bytes per step: 12 d(cur) (kf + weight) + 4 d(cur) (thresholds) + 8 d(cur) (prev's filter words)
// + 12 x (index probe + prev's weight) per filter survivor + 32 (two vrec records) + 8 (draw) + 4 (output).
#pragma once
#include "walk_dense_w.hip.h"

namespace pw {

#ifndef PW_SPB
#define PW_SPB 2       // 64-element iterations per block (the lookups behind the key load make the step latency bound, as node2vec+ dense)
#endif
#ifndef PW_SPP_PCAP
#define PW_SPP_PCAP 512   // block prefixes in LDS per wavefront (4 KB); rows of more than 512 blocks use super-blocks
#endif
constexpr uint32_t SPP_PCAP = PW_SPP_PCAP;

struct SparsePPArgs {
    const uint4 *__restrict__ vrec;           // { indptr[v], degree(v), foff[v], tab_off[v] / 2 }
    const uint2 *__restrict__ kf;             // { column, filter word } per CSR entry
    const float *__restrict__ data;           // float32 weights (nullptr: unit-weight handle)
    const uint64_t *__restrict__ fbits;
    const uint64_t *__restrict__ slots;
    const float *__restrict__ thr;            // dense-formula thresholds (pw_noise_thresholds_csr_f64)
    uint32_t n;
    double p, q;
    uint32_t L;
    uint64_t n_jobs;
    const uint32_t *__restrict__ starts;
    const uint64_t *__restrict__ stream_off;
    const uint32_t *__restrict__ job_list;
    uint64_t n_list;
    const double *__restrict__ rng;
    uint64_t rng_base;
    uint32_t *out;
    unsigned long long *job_counter;
    unsigned long long *stats;
    uint32_t exact_every;                     // tests: steps with (job + step) % k == 0 skip the bounded decision
};

// One biased value of cur's row: DenseWStep's node2vec++ arithmetic, data[prev, x] from prev's filter and index.
template <bool UNIT> struct SparsePPStep {
    DenseWStep<UNIT ? DW_N2VPP_UNIT : DW_N2VPP> c;   // constants, has_prev, prev, pp_value (pb / pr / pdata unused)
    const float *__restrict__ pdata;                 // prev's weights
    const uint64_t *__restrict__ pfb;                // prev's filter words
    const uint64_t *__restrict__ ptab;               // prev's adjacency index
    uint32_t pnw_mask, ptmask;
    bool prow;                                       // prev has out-edges (always in a walk; pw_step / pw_probs may name a sink)

    __device__ __forceinline__ void set_prev(const SparsePPArgs &a, uint32_t prev) {
        const uint4 rec = a.vrec[prev];
        const uint32_t dp = uni(rec.y);   // >= 1 in a walk (prev -> cur is an edge); 0: a row without filter or index
        prow = dp != 0;
        pdata = UNIT ? nullptr : a.data + uni(rec.x);
        pfb = a.fbits + uni(rec.z);
        pnw_mask = filter_mask_for_degree(dp);
        ptab = a.slots + 2ull * (uint64_t)uni(rec.w);
        ptmask = index_mask_for_degree(dp);
    }

    __device__ __forceinline__ double value(uint2 kv, double w, bool valid) const {
        if (!valid) return 0.0;
        if (!c.has_prev) return w;
        const uint32_t col = kv.x;
        const double thx = (double)c.thr[col];
        if (col == c.prev) return c.div_p(w);             // experimental.py:80, 94
        double w_px = 0.0;                                // data[prev, col]: zero for a non-neighbour
        if (thx > 0.0 && prow) {                          // (otherwise w_px < thx is false for any w_px >= 0: no lookup)
            const uint64_t word = pfb[filter_word(kv.y, pnw_mask)];
            if (filter_pass(word, kv.y)) {
                const uint32_t pos = adj_lookup(ptab, ptmask, col, true);
                if (pos != 0xffffffffu) {
                    if constexpr (UNIT) w_px = 1.0;
                    else w_px = (double)pdata[pos];
                }
            }
        }
        return c.pp_value(w, w_px, thx);
    }
};

template <bool UNIT>
__device__ __forceinline__ void spp_setup(SparsePPStep<UNIT> &sv, const SparsePPArgs &a) {
    dw_setup<UNIT ? DW_N2VPP_UNIT : DW_N2VPP>(sv.c, a, nullptr, nullptr);
    sv.pdata = nullptr;
    sv.pfb = nullptr;
    sv.ptab = nullptr;
    sv.pnw_mask = sv.ptmask = 0;
    sv.prow = false;
}

template <bool UNIT>
__global__ void __launch_bounds__(WAVE)
walk_sparse_pp_kernel(SparsePPArgs a) {
    constexpr int DWB = PW_SPB;
    constexpr uint32_t BLK = DWB * WAVE;                 // elements per block
    __shared__ double P[SPP_PCAP + 1];                   // prefixes of the (super-)blocks
    const int lane = lane_id();
    const uint32_t L = a.L, n = a.n;
    const uint64_t W = (uint64_t)L + 2;
    const uint64_t n_work = a.job_list ? a.n_list : a.n_jobs;
    unsigned long long st_steps = 0, st_dead = 0, st_exact = 0, st_clamp = 0;

    SparsePPStep<UNIT> sv;
    spp_setup<UNIT>(sv, a);

    for (;;) {
        unsigned long long widx = 0;
        if (lane == 0) widx = atomicAdd(a.job_counter, 1ull);
        widx = readfirst_u64(widx);
        if (widx >= n_work) break;
        const uint64_t job = a.job_list ? (uint64_t)uni(a.job_list[widx]) : (uint64_t)widx;
        uint32_t *row = a.out + job * W;
        const uint32_t start = uni(a.starts[job]);
        const uint64_t soff = readfirst_u64(a.stream_off[job]) - a.rng_base;
        uint32_t cur = start, prev = 0;
        uint32_t len_out = L + 1;
        double rbuf = 0.0;
        bool dead = false;
        uint32_t j = 1;
        for (; j <= L; j++) {
            const uint4 crec = a.vrec[cur];
            const uint32_t rs = uni(crec.x), d = uni(crec.y);
            if (d == 0) { len_out = j; dead = j > 1; break; }
            const uint32_t jr = (j - 1) & (WAVE - 1);
            if (jr == 0) {
                const uint32_t idx = (j - 1) + (uint32_t)lane;
                rbuf = idx < L ? a.rng[soff + idx] : 0.0;
            }
            const double r = readlane_f64(rbuf, (int)jr);
            const bool has_prev = j >= 2;
            const uint2 *__restrict__ krow = a.kf + rs;
            const float *__restrict__ wrow = UNIT ? nullptr : a.data + rs;
            auto key = [&](uint32_t k) -> uint2 { return k < d ? krow[k] : make_uint2(0u, 0u); };
            auto wt = [&](uint32_t k) -> double {   // (unit handles keep no values: every weight is 1.0)
                if constexpr (UNIT) return k < d ? 1.0 : 0.0;
                else return k < d ? (double)wrow[k] : 0.0;
            };
            const uint32_t nblk = (d + BLK - 1) / BLK;
            const uint32_t SB = (nblk + SPP_PCAP - 1) / SPP_PCAP;     // blocks per super-block (1 up to SPP_PCAP * BLK elements)
            const uint32_t nsb = (nblk + SB - 1) / SB;

            // first block's loads in flight while prev's record is read
            uint2 k_nx[DWB];
            double w_nx[DWB];
#pragma unroll
            for (int i = 0; i < DWB; i++) {
                const uint32_t k = (uint32_t)i * WAVE + (uint32_t)lane;
                k_nx[i] = key(k);
                w_nx[i] = wt(k);
            }
            sv.c.has_prev = has_prev;
            sv.c.prev = prev;
            if (has_prev) sv.set_prev(a, prev);
            wave_lds_fence();   // (the previous step's readers of P are done)
            if (lane == 0) P[0] = 0.0;

            // ---- the one pass: block sums, (super-)block prefixes into LDS ----
            double run = 0.0;
            bool bad = false;
            for (uint32_t blk = 0; blk < nblk; blk++) {
                uint2 k_cu[DWB];
                double w_cu[DWB];
#pragma unroll
                for (int i = 0; i < DWB; i++) { k_cu[i] = k_nx[i]; w_cu[i] = w_nx[i]; }
                if (blk + 1 < nblk) {
#pragma unroll
                    for (int i = 0; i < DWB; i++) {
                        const uint32_t k = (blk + 1) * BLK + (uint32_t)i * WAVE + (uint32_t)lane;
                        k_nx[i] = key(k);
                        w_nx[i] = wt(k);
                    }
                }
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < DWB; i++) {
                    const uint32_t k = blk * BLK + (uint32_t)i * WAVE + (uint32_t)lane;
                    const double e = sv.value(k_cu[i], w_cu[i], k < d);
                    bad |= !(e >= 0.0);
                    acc += e;
                }
                run += dw_wave_sum(acc);
                if (lane == 0) P[blk / SB + 1] = run;   // (the last block of a super-block writes its prefix)
            }
            wave_lds_fence();
            const double TOT = run;
            // ---- thresholds of the bounded decision (header; walk_dense_w.hip.h) ----
            const double E = ((2.0 * (double)d + 2.0 * (double)nblk + (double)((SB + 2) * DWB + 20)) * 0x1p-53) * (1.0 + 0x1p-20) + 8.0 * 0x1p-53;
            const double T = r * TOT;
            const double Tl = T - T * E, Th = T + T * E;
            const bool ok = ballot(bad) == 0ull && TOT > 0.0 && TOT < 0x1p1000;
            uint32_t nxt = NOT_FOUND;
            const bool force_exact = a.exact_every && (job + j) % a.exact_every == 0;   // (test switch)
            if (ok && !force_exact) {
                uint32_t tb = NOT_FOUND;
                for (uint32_t b0 = 0; b0 < nsb && tb == NOT_FOUND; b0 += WAVE) {
                    const uint32_t b = b0 + (uint32_t)lane;
                    const uint64_t m = ballot(b < nsb && P[b + 1] >= Tl);
                    if (m) tb = b0 + (uint32_t)__builtin_ctzll(m);
                }
                if (tb != NOT_FOUND) {
                    double base = P[tb];
                    const uint32_t k_lo = tb * SB * BLK;
                    const uint32_t k_hi = k_lo + SB * BLK < d ? k_lo + SB * BLK : d;
#pragma unroll 1
                    for (uint32_t k0 = k_lo; k0 < k_hi; k0 += WAVE) {
                        const uint32_t k = k0 + (uint32_t)lane;
                        const uint2 kv = key(k);
                        const double sc = wave_incl_scan_f64(sv.value(kv, wt(k), k < d));
                        const double S = base + sc;
                        const uint64_t m = ballot(k < d && S >= Tl);
                        if (m) {
                            const int l = __builtin_ctzll(m);
                            const double Sk = readlane_f64(S, l);
                            const bool first = k0 == 0 && l == 0;
                            const bool low_ok = l > 0 || first || base < Tl;
                            if (low_ok && Sk >= Th) nxt = readlane_u32(kv.x, l);
                            break;
                        }
                        base = base + readlane_f64(sc, WAVE - 1);
                    }
                }
            }
            if (nxt == NOT_FOUND) {
                // ---- a partial sum inside the bound's interval, a non-finite value or the test switch: the reference's two
                //      loops themselves, in their order
                auto at = [&](uint32_t k, uint32_t &col) -> double {
                    const uint2 kv = key(k);
                    col = kv.x;
                    return sv.value(kv, wt(k), k < d);
                };
                uint32_t pos_unused = 0;
                nxt = dw_chain_decide<true>(at, d, r, &pos_unused, nullptr);
                st_exact++;
            }
            if (nxt == NOT_FOUND) {   // no partial sum reaches r: the reference reads past the row -- clamped
                nxt = uni(krow[d - 1].x);
                st_clamp++;
            }
            if (lane == 0) row[j] = nxt < n ? nxt : 0u;
            prev = cur;
            cur = nxt < n ? nxt : 0u;
        }
        st_steps += (unsigned long long)(j <= L ? j - 1 : L);
        if (dead) st_dead++;
        if (lane == 0) { row[0] = start; row[L + 1] = len_out; }
        for (uint32_t z = j + lane; z <= L; z += WAVE) row[z] = 0;
    }
    if (lane == 0) {
        if (st_steps) atomicAdd(&a.stats[ST_STEPS], st_steps);
        if (st_dead) atomicAdd(&a.stats[ST_DEAD], st_dead);
        if (st_exact) atomicAdd(&a.stats[ST_AMBIGUOUS], st_exact);   // (pw_stats.ambiguous_steps: steps decided by the float64 chain itself)
        if (st_clamp) { atomicAdd(&a.stats[ST_OVERFLOW], st_clamp); atomicAdd(&a.stats[ST_CLAMPED], st_clamp); }   // (overflow + clamped reads)
    }
}

// ---- one step of one (cur, prev) for pw_step / pw_probs: ONE wavefront, the walk kernel's value() and its two loops (the
// probabilities are exactly the values the walk samples from)
template <bool UNIT>
__global__ void __launch_bounds__(WAVE)
sparse_pp_probe_kernel(SparsePPArgs a, const ProbeArgs *pa) {
    const uint32_t cur = uni(pa->cur), prev = uni(pa->prev);
    const bool has_prev = uni(pa->has_prev) != 0u;
    const uint4 crec = a.vrec[cur];
    const uint32_t rs = uni(crec.x), d = uni(crec.y);
    if (lane_id() == 0) pa->out[2] = d;
    if (d == 0) return;
    SparsePPStep<UNIT> sv;
    spp_setup<UNIT>(sv, a);
    sv.c.has_prev = has_prev;
    sv.c.prev = prev;
    if (has_prev) sv.set_prev(a, prev);
    const uint2 *__restrict__ krow = a.kf + rs;
    const float *__restrict__ wrow = UNIT ? nullptr : a.data + rs;
    auto at = [&](uint32_t k, uint32_t &col) -> double {
        const uint2 kv = k < d ? krow[k] : make_uint2(0u, 0u);
        col = kv.x;
        double w = 0.0;
        if constexpr (UNIT) w = k < d ? 1.0 : 0.0;
        else w = k < d ? (double)wrow[k] : 0.0;
        return sv.value(kv, w, k < d);
    };
    uint32_t pos = d;
    uint32_t nxt = dw_chain_decide<true>(at, d, uni(pa->r), &pos, uni(pa->want_probs) ? (double *)pa->probs : nullptr);
    if (nxt == NOT_FOUND) nxt = uni(krow[d - 1].x);   // (clamped, as the walk kernel does)
    if (lane_id() == 0) {
        pa->out[0] = pos;
        pa->out[1] = nxt;
    }
}

// flag = 1 when some stored weight is 0.0f (node2vec++ on CSR: the dense reference would not see such an entry at all)
__global__ void __launch_bounds__(256)
csr_zero_weight_kernel(const float *__restrict__ data, uint64_t nnz, unsigned long long *flag) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz && data[e] == 0.0f) *flag = 1ull;
}

}  // namespace pw
