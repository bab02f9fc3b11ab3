// nbr_selfcheck.cpp -- the host form of the neighbourhood baselines (csrc/nbr_scores.hip.h) as a stand-alone program for the
// sanitizers: no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/nbr_selfcheck.cpp -o /tmp/nbr_selfcheck && /tmp/nbr_selfcheck
//
// The definition on one graph written out by hand -- loops on u, on v and on a common neighbour, an empty row, a last row that
// ends where the arrays end -- against answers written out here, every kind, both orders of each pair, and the two refusals of a
// row number.  The arrays are exactly as long as the definition says they must be, so that a read or a write past an end is the
// sanitizer's to find.
#include <stdio.h>

#include <vector>

#include "../pecanpy_amd/csrc/nbr_scores.hip.h"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

}  // namespace

int main() {
    // row 0: 0 1 2 4 5 | row 1: 0 1 2 5 6 | row 2: 2 | row 3: (empty) | row 4: 5 | row 5: 0 | row 6: 1 2 3 4 5 6
    const std::vector<uint32_t> indptr = {0, 5, 10, 11, 11, 12, 13, 19};
    const std::vector<uint32_t> indices = {0, 1, 2, 4, 5, 0, 1, 2, 5, 6, 2, 5, 0, 1, 2, 3, 4, 5, 6};
    const uint32_t n = 7;
    const std::vector<double> table = {1e30, 1.0, -1e30, 3.0, 0.25, 1e-3, 7.0};

    std::vector<uint32_t> deg(n, 77);
    pw::nbr_host_degrees(indptr.data(), indices.data(), n, deg.data());
    expect(deg == std::vector<uint32_t>({4, 4, 0, 0, 1, 1, 5}), "degrees without the loops");

    // C(0, 1) = {2, 5} (0 and 1 are in both rows and are no common neighbours); C(0, 6) = {1, 2, 4, 5}; C(6, 6) = N(6)
    const std::vector<uint32_t> u = {0, 1, 0, 6, 6, 3, 2, 4}, v = {1, 0, 6, 0, 6, 0, 2, 1};
    const uint64_t m = u.size();
    std::vector<double> score(m, -1.0);
    uint64_t where = 99;
    expect(pw::nbr_host_scores(indptr.data(), indices.data(), n, u.data(), v.data(), m, pw::NBR_COMMON, nullptr, score.data(), &where) == pw::LP_HOST_OK,
           "common neighbours run");
    expect(score == std::vector<double>({2, 2, 4, 4, 5, 0, 0, 1}), "common neighbours");
    pw::nbr_host_scores(indptr.data(), indices.data(), n, u.data(), v.data(), m, pw::NBR_JACCARD, nullptr, score.data(), &where);
    expect(score == std::vector<double>({2.0 / 6.0, 2.0 / 6.0, 4.0 / 5.0, 4.0 / 5.0, 1.0, 0.0, 0.0, 1.0 / 4.0}), "jaccard, +0.0 on an empty union");
    pw::nbr_host_scores(indptr.data(), indices.data(), n, u.data(), v.data(), m, pw::NBR_PREF, nullptr, score.data(), &where);
    expect(score == std::vector<double>({16, 16, 20, 20, 25, 0, 0, 4}), "preferential attachment");
    pw::nbr_host_scores(indptr.data(), indices.data(), n, u.data(), v.data(), m, pw::NBR_WEIGHTED, table.data(), score.data(), &where);
    // ascending: ((0 + -1e30) + 1e-3) = -1e30;  (((0 + 1) + -1e30) + 0.25) + 1e-3 = -1e30;  ((((0 + 1) + -1e30) + 3) + 0.25) + 1e-3 = -1e30
    expect(score == std::vector<double>({-1e30, -1e30, -1e30, -1e30, -1e30, 0.0, 0.0, 1e-3}), "the table summed in ascending order");
    expect(pw::nbr_pref(0xFFFFFFFFu, 0xFFFFFFFFu) == 18446744065119617025.0, "the product of two 32-bit degrees is exact before its one rounding");

    std::vector<uint32_t> bu = u, bv = v;
    bv[2] = 7;
    bu[5] = 9;
    std::vector<double> untouched(m, -1.0);
    expect(pw::nbr_host_scores(indptr.data(), indices.data(), n, bu.data(), bv.data(), m, pw::NBR_COMMON, nullptr, untouched.data(), &where) ==
                   pw::LP_HOST_V_RANGE && where == 2 && untouched == std::vector<double>(m, -1.0),
           "v out of range: named, nothing written");
    bu[2] = 7;
    expect(pw::nbr_host_scores(indptr.data(), indices.data(), n, bu.data(), bv.data(), m, pw::NBR_COMMON, nullptr, untouched.data(), &where) ==
                   pw::LP_HOST_U_RANGE && where == 2,
           "both out of range at one position: u is named");
    expect(pw::nbr_host_scores(indptr.data(), indices.data(), n, nullptr, nullptr, 0, pw::NBR_JACCARD, nullptr, nullptr, &where) == pw::LP_HOST_OK,
           "m = 0 does nothing");

    printf(failures ? "%d checks FAILED\n" : "nbr_selfcheck: all checks passed\n", failures);
    return failures ? 1 : 0;
}
