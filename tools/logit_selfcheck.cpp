// logit_selfcheck.cpp -- the host form of the exact logistic regression (csrc/logit.hip.h) as a stand-alone program for the
// sanitizers: no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/logit_selfcheck.cpp -o /tmp/logit_selfcheck && /tmp/logit_selfcheck
//
// The definition at dim 2 on values chosen so that every decision value and every gradient entry is exact and written out here
// by hand: each operator, the second matrix, z alone, 1025 samples (two chunks, the second of one sample), the saturated
// branches, and the four refusals that need data.  The arrays are exactly as long as the definition says they must be, so that a
// read or a write past an end is the sanitizer's to find.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../pecanpy_amd/csrc/logit.hip.h"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

}  // namespace

int main() {
    const uint32_t dim = 2;
    const std::vector<float> A = {1.f, 2.f, 0.5f, -1.f, 0.f, 0.f};   // rows (1, 2), (0.5, -1), (0, 0)
    const std::vector<float> B = {4.f, 0.25f};                       // one row
    const std::vector<double> theta = {1.0, -2.0, 0.5};              // w = (1, -2), bias 0.5
    const std::vector<double> zero = {0.0, 0.0, 0.0};
    uint64_t where = 99;

    // the pair (0, 1) under every operator: f and z = 0.5 + f0 - 2 f1 by hand
    const std::vector<uint32_t> u1 = {0}, v1 = {1};
    const double want_z[pw::LG_OPS] = {
        -2.5,     // row       f = (1, 2)
        0.25,     // average   f = (0.75, 0.5)
        5.0,      // hadamard  f = (0.5, -2)
        -5.0,     // l1        f = (0.5, 3)
        -17.25,   // l2        f = (0.25, 9)
    };
    for (int op = 0; op < pw::LG_OPS; op++) {
        std::vector<double> z(1, -1.0);
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, u1.data(), op == pw::LG_ROW ? nullptr : v1.data(), nullptr, 1, op, theta.data(), 0.0, nullptr,
                                nullptr, z.data(), &where) == pw::LG_HOST_OK && z[0] == want_z[op],
               "z of the pair (0, 1)");
    }
    {   // the second matrix: hadamard of A[0] = (1, 2) and B[0] = (4, 0.25): f = (4, 0.5), z = 0.5 + 4 - 1 = 3.5
        const std::vector<uint32_t> u = {0}, v = {0};
        std::vector<double> z(1, -1.0);
        expect(pw::lg_host_eval(A.data(), 3, B.data(), 1, dim, u.data(), v.data(), nullptr, 1, pw::LG_HADAMARD, theta.data(), 0.0, nullptr, nullptr,
                                z.data(), &where) == pw::LG_HOST_OK && z[0] == 3.5,
               "second matrix");
    }
    {   // theta = 0: z = 0, t = 1, q = 1/2.  Samples (0, 1) with y = 1: r = -1/2, f = (0.5, -2); (2, 2) with y = 0: r = +1/2, f = (0, 0).
        // G = (-0.25, 1, 0); grad = G / 2 + l2 * 0 = (-0.125, 0.5, 0); loss = lg_log1p(1) = ln 2 to an ulp or two
        const std::vector<uint32_t> u = {0, 2}, v = {1, 2};
        const std::vector<uint8_t> y = {1, 0};
        std::vector<double> grad(dim + 1, -1.0), z(2, -1.0);
        double loss = -1.0;
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, u.data(), v.data(), y.data(), 2, pw::LG_HADAMARD, zero.data(), 0.5, &loss, grad.data(),
                                z.data(), &where) == pw::LG_HOST_OK,
               "two samples accepted");
        expect(grad[0] == -0.125 && grad[1] == 0.5 && grad[2] == 0.0 && z[0] == 0.0 && z[1] == 0.0, "gradient at theta = 0");
        expect(fabs(loss - 0.6931471805599453) < 1e-15, "loss at theta = 0");
    }
    {   // 1025 copies of the sample (0, 1), y = 1, theta = 0: two chunks.  G0 = 1025 * -0.25 exactly, grad = (-0.25, 1, -0.5)
        const uint64_t m = 1025;
        const std::vector<uint32_t> u(m, 0), v(m, 1);
        const std::vector<uint8_t> y(m, 1);
        std::vector<double> grad(dim + 1, -1.0);
        double loss = -1.0;
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, u.data(), v.data(), y.data(), m, pw::LG_HADAMARD, zero.data(), 0.0, &loss, grad.data(),
                                nullptr, &where) == pw::LG_HOST_OK && grad[0] == -0.25 && grad[1] == 1.0 && grad[2] == -0.5,
               "two chunks");
    }
    {   // saturated: z = +-1000 (theta = (0, 0, +-1000)).  t = +0.0: the right label costs 0 and has r = 0, the wrong one costs 1000, r = +-1
        double r = -1.0, ell = -1.0;
        pw::lg_sample(1000.0, 1, &r, &ell);
        expect(r == 0.0 && ell == 0.0, "saturated, right label");
        pw::lg_sample(1000.0, 0, &r, &ell);
        expect(r == 1.0 && ell == 1000.0, "saturated, wrong label 0");
        pw::lg_sample(-1000.0, 1, &r, &ell);
        expect(r == -1.0 && ell == 1000.0, "saturated, wrong label 1");
        expect(pw::lg_exp(0.0) == 1.0 && pw::lg_exp(-708.0) > 0.0 && pw::lg_exp(-708.0000001) == 0.0 && pw::lg_log1p(0.0) == 0.0, "ends of the two functions");
        expect(fabs(pw::lg_exp(-1.0) - 0.36787944117144233) < 1e-16, "lg_exp(-1)");
    }
    {   // refusals: nothing is written
        const std::vector<uint32_t> u = {0, 3, 1}, v = {1, 0, 3}, ok = {0, 1, 2};
        const std::vector<uint8_t> y = {1, 0, 1}, y_bad = {1, 0, 2};
        const std::vector<double> huge = {1e308, 1e308, 0.0};
        std::vector<double> grad(dim + 1, -1.0), z(3, -1.0);
        double loss = -1.0;
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, u.data(), v.data(), y.data(), 3, pw::LG_L1, theta.data(), 0.0, &loss, grad.data(), z.data(),
                                &where) == pw::LG_HOST_U_RANGE && where == 1,
               "u out of range");
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, ok.data(), v.data(), y.data(), 3, pw::LG_L1, theta.data(), 0.0, &loss, grad.data(), z.data(),
                                &where) == pw::LG_HOST_V_RANGE && where == 2,
               "v out of range");
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, ok.data(), v.data(), y.data(), 3, pw::LG_ROW, theta.data(), 0.0, &loss, grad.data(), nullptr,
                                &where) == pw::LG_HOST_OK,
               "op row does not look at v");
        loss = -1.0;
        grad.assign(dim + 1, -1.0);
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, ok.data(), ok.data(), y_bad.data(), 3, pw::LG_L1, theta.data(), 0.0, &loss, grad.data(),
                                z.data(), &where) == pw::LG_HOST_LABEL && where == 2,
               "label 2");
        expect(pw::lg_host_eval(A.data(), 3, A.data(), 3, dim, ok.data(), ok.data(), y.data(), 3, pw::LG_ROW, huge.data(), 0.0, &loss, grad.data(), z.data(),
                                &where) == pw::LG_HOST_Z && where == 0,
               "z not finite");
        expect(loss == -1.0 && grad == std::vector<double>(dim + 1, -1.0) && z == std::vector<double>(3, -1.0), "a refusal writes nothing");
        expect(pw::lg_host_theta_bad(theta.data(), dim) == dim + 1 && !pw::lg_l2_valid(-1.0) && !pw::lg_l2_valid(NAN) && pw::lg_l2_valid(0.0) &&
                   !pw::lg_op_known(5) && pw::lg_op_known(pw::LG_L2),
               "the checks that need no data");
    }
    printf(failures ? "logit_selfcheck: %d FAILED\n" : "logit_selfcheck: all passed\n", failures);
    return failures ? 1 : 0;
}
