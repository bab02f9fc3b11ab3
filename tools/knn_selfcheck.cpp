// knn_selfcheck.cpp -- the host form of the nearest-neighbour definition (csrc/knn.hip.h) as a stand-alone program for the
// sanitizers: no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/knn_selfcheck.cpp -o /tmp/knn_selfcheck && /tmp/knn_selfcheck
//
// A few shapes around the list length (topn 1, n, n + 1, 128), planted ties, a zero row, queries by row and by vector, and
// the three refusals, each against a sort of all candidates written here in the plainest way.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../pecanpy_amd/csrc/knn.hip.h"

namespace {

uint32_t g_state = 12345u;
float next_value() {   // small integers and halves: many exact ties
    g_state = g_state * 1664525u + 1013904223u;
    return (float)((int)((g_state >> 24) % 9u) - 4) * 0.5f;
}

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

void check(uint64_t n, uint32_t dim, uint64_t nq, uint32_t topn, int metric, bool by_row) {
    std::vector<float> X(n * dim), Q(nq * dim);
    for (auto &v : X) v = next_value();
    for (auto &v : Q) v = next_value();
    if (n > 2) for (uint32_t k = 0; k < dim; k++) { X[2 * dim + k] = 0.f; X[(n - 1) * dim + k] = 2.f * X[k]; }
    std::vector<uint32_t> rows(nq);
    for (uint64_t q = 0; q < nq; q++) rows[q] = (uint32_t)((q * 7) % n);
    std::vector<uint32_t> idx(nq * topn);
    std::vector<double> score(nq * topn), norms(n), qnorms(nq);
    uint64_t where = 0;
    const int rc = pw::knn_host_query(X.data(), n, dim, by_row ? nullptr : Q.data(), by_row ? rows.data() : nullptr, nq, topn, metric, 1,
                                      idx.data(), score.data(), norms.data(), qnorms.data(), &where);
    expect(rc == pw::KNN_HOST_OK, "valid call accepted");
    for (uint64_t q = 0; q < nq; q++) {
        const float *qv = by_row ? &X[rows[q] * dim] : &Q[q * dim];
        struct Cand { double s; uint32_t r; };
        std::vector<Cand> all;
        for (uint64_t i = 0; i < n; i++) {
            if (by_row && i == rows[q]) continue;
            const double nx = sqrt(pw::knn_dot(&X[i * dim], &X[i * dim], dim)), nqv = sqrt(pw::knn_dot(qv, qv, dim));
            all.push_back({pw::knn_score(pw::knn_dot(qv, &X[i * dim], dim), nqv, nx, metric), (uint32_t)i});
        }
        std::sort(all.begin(), all.end(), [](const Cand &a, const Cand &b) { return a.s > b.s || (a.s == b.s && a.r < b.r); });
        for (uint32_t e = 0; e < topn; e++) {
            const bool have = e < all.size();
            expect(idx[q * topn + e] == (have ? all[e].r : pw::KNN_NONE), "idx");
            expect(score[q * topn + e] == (have ? all[e].s : pw::knn_neg_inf()), "score");
        }
    }
}

}  // namespace

int main() {
    for (int metric : {pw::KNN_DOT, pw::KNN_COSINE})
        for (bool by_row : {false, true}) {
            check(1, 1, 1, 1, metric, by_row);
            check(2, 3, 2, 128, metric, by_row);
            check(65, 37, 9, 64, metric, by_row);
            check(65, 37, 9, 65, metric, by_row);
            check(130, 5, 3, 128, metric, by_row);
            check(300, 4, 8, 10, metric, by_row);
        }
    // the refusals: nothing is written
    std::vector<float> X(4 * 3, 1.f), Q(2 * 3, 1.f);
    std::vector<uint32_t> idx(2, 77u), rows = {0, 4};
    std::vector<double> score(2, 7.0), norms(4), qnorms(2);
    uint64_t where = 99;
    X[2 * 3 + 1] = NAN;
    expect(pw::knn_host_query(X.data(), 4, 3, Q.data(), nullptr, 2, 1, 0, 0, idx.data(), score.data(), norms.data(), qnorms.data(), &where) ==
                   pw::KNN_HOST_BAD_ROW && where == 2, "NaN row named");
    X[2 * 3 + 1] = 1.f;
    Q[3] = INFINITY;
    expect(pw::knn_host_query(X.data(), 4, 3, Q.data(), nullptr, 2, 1, 0, 0, idx.data(), score.data(), norms.data(), qnorms.data(), &where) ==
                   pw::KNN_HOST_BAD_QUERY && where == 1, "infinite query named");
    expect(pw::knn_host_query(X.data(), 4, 3, nullptr, rows.data(), 2, 1, 0, 1, idx.data(), score.data(), norms.data(), qnorms.data(), &where) ==
                   pw::KNN_HOST_ROW_RANGE && where == 1, "row number out of range named");
    expect(idx[0] == 77u && idx[1] == 77u && score[0] == 7.0 && score[1] == 7.0, "nothing written by a refused call");
    printf(failures ? "knn_selfcheck: %d failures\n" : "knn_selfcheck: ok\n", failures);
    return failures ? 1 : 0;
}
