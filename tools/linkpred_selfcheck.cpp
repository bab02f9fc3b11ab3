// linkpred_selfcheck.cpp -- the host form of the link-prediction definitions (csrc/linkpred.hip.h) as a stand-alone program
// for the sanitizers: no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/linkpred_selfcheck.cpp -o /tmp/linkpred_selfcheck && /tmp/linkpred_selfcheck
//
// The three definitions on fixed inputs against answers written out here: pair scores of small integer vectors (every sum
// exact), the AUC of six numbers and of signed zeros and infinities, and the sampler on a path of four vertices fed with
// words chosen by hand, with its cap and its refusals.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../pecanpy_amd/csrc/linkpred.hip.h"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

void check_scores() {
    // A: 4 rows of dim 3; B: 2 rows
    const std::vector<float> A = {1, 2, 2, 0, 0, 0, 3, 0, 4, -1, -2, -2}, B = {0, 3, 4, 2, 1, 2};
    std::vector<double> an(4), bn(2);
    uint64_t where = 99;
    expect(pw::knn_host_norms(A.data(), 4, 3, an.data(), &where) == 0 && pw::knn_host_norms(B.data(), 2, 3, bn.data(), &where) == 0, "norms");
    expect(an[0] == 3 && an[1] == 0 && an[2] == 5 && an[3] == 3 && bn[0] == 5 && bn[1] == 3, "norms written out");
    const std::vector<uint32_t> u = {0, 0, 1, 2, 3, 3, 0}, v = {0, 3, 2, 2, 0, 0, 0};
    std::vector<double> s(7, 7.0);
    expect(pw::lp_host_score_pairs(A.data(), an.data(), 4, A.data(), an.data(), 4, 3, u.data(), v.data(), 7, pw::KNN_DOT, s.data(), &where) == 0, "dot accepted");
    const double dot[7] = {9, -9, 0, 25, -9, -9, 9};
    for (int i = 0; i < 7; i++) expect(s[i] == dot[i], "dot");
    expect(pw::lp_host_score_pairs(A.data(), an.data(), 4, A.data(), an.data(), 4, 3, u.data(), v.data(), 7, pw::KNN_COSINE, s.data(), &where) == 0, "cosine accepted");
    const double cosine[7] = {1, -1, 0, 1, -1, -1, 1};
    for (int i = 0; i < 7; i++) expect(s[i] == cosine[i] && !(s[i] == 0 && __builtin_signbit(s[i])), "cosine");
    // against B: (0, 0) = 14 / 15, (2, 1) = 14 / 15, (1, 1) = +0.0
    const std::vector<uint32_t> ub = {0, 2, 1}, vb = {0, 1, 1};
    expect(pw::lp_host_score_pairs(A.data(), an.data(), 4, B.data(), bn.data(), 2, 3, ub.data(), vb.data(), 3, pw::KNN_COSINE, s.data(), &where) == 0, "second matrix");
    expect(s[0] == 14.0 / 15.0 && s[1] == 14.0 / 15.0 && s[2] == 0.0, "cosine against a second matrix");
    // refusals: the first offending position, u before v, nothing written
    std::vector<double> keep(3, 7.0);
    const std::vector<uint32_t> bad_u = {0, 4, 9}, bad_v = {2, 0, 0}, bad_both = {0, 4, 0}, bad_v2 = {0, 2, 2};
    expect(pw::lp_host_score_pairs(A.data(), an.data(), 4, B.data(), bn.data(), 2, 3, bad_u.data(), bad_v.data(), 3, 0, keep.data(), &where) == pw::LP_HOST_V_RANGE &&
               where == 0, "v out of range named");
    expect(pw::lp_host_score_pairs(A.data(), an.data(), 4, B.data(), bn.data(), 2, 3, bad_both.data(), bad_v2.data(), 3, 0, keep.data(), &where) ==
               pw::LP_HOST_U_RANGE && where == 1, "u named before v");
    expect(keep[0] == 7.0 && keep[1] == 7.0 && keep[2] == 7.0, "nothing written by a refused call");
    expect(pw::lp_host_score_pairs(A.data(), an.data(), 4, A.data(), an.data(), 4, 3, nullptr, nullptr, 0, 0, nullptr, &where) == 0, "m = 0");
}

void auc(const std::vector<double> &pos, const std::vector<double> &neg, uint64_t wins, uint64_t ties, const char *what) {
    std::vector<uint64_t> keys(neg.size());
    uint64_t where = 99, out[2] = {77, 77};
    expect(pw::auc_host_keys(neg.data(), neg.size(), keys.data(), &where) == 0, what);
    std::sort(keys.begin(), keys.end());
    pw::auc_host_count(pos.data(), pos.size(), keys.data(), neg.size(), out);
    expect(out[0] == wins && out[1] == ties, what);
    uint64_t w = 0, t = 0;   // the plain count
    for (double p : pos) for (double q : neg) { w += p > q; t += p == q; }
    expect(w == wins && t == ties, what);
}

void check_auc() {
    const double inf = __builtin_huge_val(), tiny = 4.9406564584124654e-324;
    auc({0.1, 0.4, 0.35, 0.8}, {0.1, 0.35}, 5, 2, "six numbers");
    auc({0.0, -0.0, tiny, -tiny}, {-0.0, 0.0, -tiny}, 1 + 1 + 3 + 0, 2 + 2 + 0 + 1, "signed zeros and subnormals");
    auc({inf, -inf, 1.0}, {inf, -inf, -inf, 2.0}, 3 + 0 + 2, 1 + 2 + 0, "infinities");
    auc({2.0}, {2.0}, 0, 1, "one against one");
    expect(pw::auc_key(-0.0) == pw::auc_key(0.0) && pw::auc_key(-tiny) < pw::auc_key(0.0) && pw::auc_key(0.0) < pw::auc_key(tiny) &&
               pw::auc_key(-inf) < pw::auc_key(-1e308) && pw::auc_key(1e308) < pw::auc_key(inf), "key order");
    const std::vector<double> bad = {1.0, __builtin_nan(""), 2.0, __builtin_nan("")};
    std::vector<uint64_t> keys(4);
    uint64_t where = 99;
    expect(pw::auc_host_keys(bad.data(), 4, keys.data(), &where) == 1 && where == 1, "first NaN named");
}

void check_sampler() {
    // the path 0 - 1 - 2 - 3, both directions: N = 4, nnz = 6, acceptable = 12 - 6 = 6
    const std::vector<uint32_t> indptr = {0, 1, 3, 5, 6}, indices = {1, 0, 2, 1, 3, 2};
    expect(pw::lp_host_loops(indptr.data(), indices.data(), 4) == 0 && pw::lp_acceptable(4, 6, 0) == 6, "acceptable pairs");
    expect(pw::lp_candidate_cap(1, 4, 6) == 16 * 3 + 64 && pw::lp_candidate_cap(3, 4, 6) == 16 * 8 + 64 && pw::lp_candidate_cap(1, 16, 1) == 4160, "cap");
    expect(pw::lp_candidate_cap(1ull << 40, 1u << 31, 1) == pw::LP_CAP_MAX, "cap saturates");
    // a word w gives vertex (w * 4) >> 32 = w >> 30
    auto word = [](uint32_t vertex) { return (vertex << 30) | 12345u; };
    // candidates: (0,0) loop, (0,1) edge, (0,2) ok, (3,2) edge, (3,0) ok, (1,1) loop, (0,2) ok again, (2,0) ok
    const uint32_t cand[8][2] = {{0, 0}, {0, 1}, {0, 2}, {3, 2}, {3, 0}, {1, 1}, {0, 2}, {2, 0}};
    std::vector<uint32_t> words;
    for (auto &c : cand) { words.push_back(word(c[0])); words.push_back(word(c[1])); }
    auto more = [&](uint64_t c) { return words.data() + 2 * c; };
    std::vector<uint32_t> u(4, 77), v(4, 77);
    uint64_t used = 99;
    expect(pw::lp_host_sample(indptr.data(), indices.data(), 4, 3, 8, more, u.data(), v.data(), &used) == 0 && used == 7, "three non-edges in seven candidates");
    expect(u[0] == 0 && v[0] == 2 && u[1] == 3 && v[1] == 0 && u[2] == 0 && v[2] == 2 && u[3] == 77, "the pairs, one of them twice");
    expect(pw::lp_host_sample(indptr.data(), indices.data(), 4, 1, 8, more, u.data(), v.data(), &used) == 0 && used == 3, "one non-edge in three candidates");
    expect(pw::lp_host_sample(indptr.data(), indices.data(), 4, 0, 8, more, u.data(), v.data(), &used) == 0 && used == 0, "m = 0");
    expect(pw::lp_host_sample(indptr.data(), indices.data(), 4, 4, 8, more, u.data(), v.data(), &used) == 0 && used == 8, "the last candidate");
    used = 99;
    expect(pw::lp_host_sample(indptr.data(), indices.data(), 4, 4, 7, more, u.data(), v.data(), &used) == pw::LP_HOST_CAP && used == 99, "the cap ends the call");
    // a loop in the CSR counts once: the triangle with a loop at 1 is complete off the diagonal
    const std::vector<uint32_t> tp = {0, 2, 5, 7}, ti = {1, 2, 0, 1, 2, 0, 1};
    expect(pw::lp_host_loops(tp.data(), ti.data(), 3) == 1 && pw::lp_acceptable(3, 7, 1) == 0, "no off-diagonal non-edge");
}

}  // namespace

int main() {
    check_scores();
    check_auc();
    check_sampler();
    printf(failures ? "linkpred_selfcheck: %d failures\n" : "linkpred_selfcheck: ok\n", failures);
    return failures ? 1 : 0;
}
