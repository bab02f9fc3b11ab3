// seq_spec_selfcheck.cpp -- the speculation rounds of the seeded alias / first-order modes (csrc/seq_spec.h) on the host,
// as a stand-alone program for the sanitizers: no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/seq_spec_selfcheck.cpp -o /tmp/seq_spec_selfcheck -lpthread && /tmp/seq_spec_selfcheck
//
// Zachary's karate club and two stars (hub degree 64: nothing rejected; 65: about half the words rejected), every start
// three times, speculative against the plain sequential loop under the configurations of tests/test_seq_spec_host.py.
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../pecanpy_amd/csrc/seq_spec_host.hpp"

namespace {

struct Csr {
    std::vector<uint32_t> indptr, indices;
    uint32_t n() const { return (uint32_t)indptr.size() - 1; }
};

Csr from_edges(uint32_t n, const std::vector<std::pair<uint32_t, uint32_t>> &und) {
    std::vector<std::vector<uint32_t>> adj(n);
    for (auto e : und) { adj[e.first].push_back(e.second); adj[e.second].push_back(e.first); }
    Csr c;
    c.indptr.push_back(0);
    for (auto &row : adj) {
        std::sort(row.begin(), row.end());
        c.indices.insert(c.indices.end(), row.begin(), row.end());
        c.indptr.push_back((uint32_t)c.indices.size());
    }
    return c;
}

Csr karate() {
    static const uint8_t e[][2] = {
        {2, 1},   {3, 1},   {3, 2},   {4, 1},   {4, 2},   {4, 3},   {5, 1},   {6, 1},   {7, 1},   {7, 5},   {7, 6},   {8, 1},   {8, 2},
        {8, 3},   {8, 4},   {9, 1},   {9, 3},   {10, 3},  {11, 1},  {11, 5},  {11, 6},  {12, 1},  {13, 1},  {13, 4},  {14, 1},  {14, 2},
        {14, 3},  {14, 4},  {17, 6},  {17, 7},  {18, 1},  {18, 2},  {20, 1},  {20, 2},  {22, 1},  {22, 2},  {26, 24}, {26, 25}, {28, 3},
        {28, 24}, {28, 25}, {29, 3},  {30, 24}, {30, 27}, {31, 2},  {31, 9},  {32, 1},  {32, 25}, {32, 26}, {32, 29}, {33, 3},  {33, 9},
        {33, 15}, {33, 16}, {33, 19}, {33, 21}, {33, 23}, {33, 24}, {33, 30}, {33, 31}, {33, 32}, {34, 9},  {34, 10}, {34, 14}, {34, 15},
        {34, 16}, {34, 19}, {34, 20}, {34, 21}, {34, 23}, {34, 24}, {34, 27}, {34, 28}, {34, 29}, {34, 30}, {34, 31}, {34, 32}, {34, 33}};
    std::vector<std::pair<uint32_t, uint32_t>> und;
    for (auto &p : e) und.push_back({(uint32_t)p[0] - 1, (uint32_t)p[1] - 1});
    return from_edges(34, und);
}

Csr star(uint32_t leaves) {
    std::vector<std::pair<uint32_t, uint32_t>> und;
    for (uint32_t v = 1; v <= leaves; v++) und.push_back({0u, v});
    return from_edges(leaves + 1, und);
}

int check(const char *name, const Csr &c, uint32_t walks, uint32_t L, uint32_t seed) {
    std::vector<uint32_t> starts;
    for (uint32_t w = 0; w < walks; w++)
        for (uint32_t v = 0; v < c.n(); v++) starts.push_back((v * 7 + w) % c.n());
    const uint64_t n_jobs = starts.size();
    std::vector<uint64_t> want(n_jobs + 1), got(n_jobs + 1);
    pw_seq_config seq = {};
    seq.min_jobs = UINT64_MAX;
    pw_seq_info info;
    if (pw::seq_host_offsets(c.indptr.data(), c.indices.data(), c.n(), starts.data(), n_jobs, L, seed, &seq, want.data(), &info)) return 1;
    pw_seq_config cfgs[7] = {};
    cfgs[1].jobs_per_round = 1;
    cfgs[2].jobs_per_round = 7;
    cfgs[3].jobs_per_round = 64;
    cfgs[4].window_sigmas = -1.0f;
    cfgs[5].force_mean = 1.0f;
    cfgs[6].word_buffer_blocks = 1;
    int bad = 0;
    for (int k = 0; k < 7; k++) {
        cfgs[k].min_jobs = 1;
        std::fill(got.begin(), got.end(), ~0ull);
        if (pw::seq_host_offsets(c.indptr.data(), c.indices.data(), c.n(), starts.data(), n_jobs, L, seed, &cfgs[k], got.data(), &info)) return 1;
        const bool ok = got == want && info.path == 1 && info.committed_jobs == n_jobs && info.rounds <= n_jobs && info.words_consumed == want[n_jobs];
        printf("%-10s cfg %d: %s  jobs %llu rounds %llu candidates %llu misses %llu retries %llu words %llu\n", name, k, ok ? "ok" : "MISMATCH",
               (unsigned long long)n_jobs, (unsigned long long)info.rounds, (unsigned long long)info.candidate_walks,
               (unsigned long long)info.window_misses, (unsigned long long)info.unfinished_retries, (unsigned long long)info.words_consumed);
        bad += ok ? 0 : 1;
    }
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    bad += check("karate", karate(), 10, 30, 4);
    bad += check("star64", star(64), 3, 30, 4);
    bad += check("star65", star(65), 3, 30, 4);
    printf(bad ? "FAILED\n" : "all equal\n");
    return bad ? 1 : 0;
}
