// holdout_selfcheck.cpp -- the host form of the edge hold-out (csrc/holdout.hip.h) as a stand-alone program for the
// sanitizers: no GPU, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/holdout_selfcheck.cpp -o /tmp/holdout_selfcheck && /tmp/holdout_selfcheck
//
// The definition on fixed graphs, fed with words chosen by hand, against answers written out here: the row of an entry, the
// mate search, the first non-loop entry, the split of a graph with self loops in every place the rule names, directed units,
// threshold 0, the refusal of a missing mate, a graph without entries.  Output buffers are exactly as long as the definition
// says they must be, so that a write past an end is the sanitizer's to find.
#include <stdio.h>

#include <vector>

#include "../pecanpy_amd/csrc/holdout.hip.h"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

struct Split {
    int rc;
    uint64_t where = 99;
    std::vector<uint32_t> indptr, indices, u, v;
    std::vector<float> data, weight;
    uint64_t counts[4] = {77, 77, 77, 77};
};

Split split(const std::vector<uint32_t> &indptr, const std::vector<uint32_t> &indices, const std::vector<float> *data, int directed, int protect,
            uint32_t threshold, const std::vector<uint32_t> &words) {
    const uint32_t n = (uint32_t)indptr.size() - 1, nnz = indptr[n];
    Split s;
    s.indptr.assign(n + 1, 77); s.indices.assign(nnz, 77); s.u.assign(nnz, 77); s.v.assign(nnz, 77);
    s.data.assign(nnz, 77.f); s.weight.assign(nnz, 77.f);
    s.rc = pw::ho_host_split(indptr.data(), indices.data(), data ? data->data() : nullptr, n, directed, protect, threshold,
                             [&](uint32_t e) { return words[e]; }, s.indptr.data(), s.indices.data(), s.data.data(), s.u.data(), s.v.data(),
                             s.weight.data(), s.counts, &s.where);
    return s;
}

template <typename T> bool starts_with(const std::vector<T> &got, const std::vector<T> &want) {
    if (got.size() < want.size()) return false;
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i]) return false;
    return true;
}

// rows 0 = [0, 1, 2] (starts with its loop), 1 = [0, 2], 2 = [0, 1, 2, 3] (loop mid-row), 3 = [2, 4], 4 = [3], 5 = [5] (only its
// loop), 6 = [] ; weight of the entry r -> c: 10 r + c
const std::vector<uint32_t> L_INDPTR = {0, 3, 5, 9, 11, 12, 13, 13}, L_INDICES = {0, 1, 2, 0, 2, 0, 1, 2, 3, 2, 4, 3, 5};
const std::vector<float> L_DATA = {0, 1, 2, 10, 12, 20, 21, 22, 23, 32, 34, 43, 55};

void check_parts() {
    const uint32_t rows[13] = {0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 4, 5};
    for (uint32_t e = 0; e < 13; e++) expect(pw::ho_row_of(L_INDPTR.data(), 7, e) == rows[e], "row of an entry (an empty last row behind it)");
    const std::vector<uint32_t> gaps = {0, 0, 0, 2, 2, 3};   // rows 0, 1, 3 empty
    expect(pw::ho_row_of(gaps.data(), 5, 0) == 2 && pw::ho_row_of(gaps.data(), 5, 1) == 2 && pw::ho_row_of(gaps.data(), 5, 2) == 4, "row of an entry between empty rows");
    expect(pw::ho_find(L_INDPTR.data(), L_INDICES.data(), 2, 0) == 5 && pw::ho_find(L_INDPTR.data(), L_INDICES.data(), 2, 3) == 8 &&
               pw::ho_find(L_INDPTR.data(), L_INDICES.data(), 2, 4) == pw::HO_NONE && pw::ho_find(L_INDPTR.data(), L_INDICES.data(), 6, 0) == pw::HO_NONE, "mate search");
    const uint32_t first[7] = {1, 3, 5, 9, 11, pw::HO_NONE, pw::HO_NONE};
    for (uint32_t r = 0; r < 7; r++) expect(pw::ho_first(L_INDPTR.data(), L_INDICES.data(), r) == first[r], "first non-loop entry");
}

void check_loops_graph() {
    // units at 1 (0,1), 2 (0,2), 4 (1,2), 8 (2,3), 10 (3,4).  Words below the threshold 100 at EVERY position but 8: the words of
    // loops, of lower entries and of protected units must not matter.
    std::vector<uint32_t> words(13, 5);
    words[8] = 100;
    Split s = split(L_INDPTR, L_INDICES, &L_DATA, 0, 1, 100, words);   // protected: 1 (f(0)), 2 (mate 5 = f(2)), 8 (mate 9 = f(3)), 10 (mate 11 = f(4))
    expect(s.rc == 0 && s.counts[0] == 11 && s.counts[1] == 1 && s.counts[2] == 5 && s.counts[3] == 4, "protected split: counts");
    expect(starts_with(s.u, {1u}) && starts_with(s.v, {2u}) && starts_with(s.weight, {12.f}) && s.u[1] == 77, "protected split: the one free unit, its own weight");
    expect(s.indptr == std::vector<uint32_t>({0, 3, 4, 7, 9, 10, 11, 11}) && starts_with(s.indices, {0, 1, 2, 0, 0, 2, 3, 2, 4, 3, 5}) &&
               starts_with(s.data, {0, 1, 2, 10, 20, 22, 23, 32, 34, 43, 55}) && s.indices[11] == 77, "protected split: the train CSR");
    s = split(L_INDPTR, L_INDICES, &L_DATA, 0, 0, 100, words);   // no protection: every unit but the one at 8 goes
    expect(s.rc == 0 && s.counts[0] == 5 && s.counts[1] == 4 && s.counts[2] == 5 && s.counts[3] == 0, "bare split: counts");
    expect(starts_with(s.u, {0, 0, 1, 3}) && starts_with(s.v, {1, 2, 2, 4}) && starts_with(s.weight, {1.f, 2.f, 12.f, 34.f}), "bare split: u < v, ascending position");
    expect(s.indptr == std::vector<uint32_t>({0, 1, 1, 3, 4, 4, 5, 5}) && starts_with(s.indices, {0, 2, 3, 2, 5}) && starts_with(s.data, {0, 22, 23, 32, 55}),
           "bare split: loops and the kept pair");
    s = split(L_INDPTR, L_INDICES, nullptr, 0, 1, 0, words);   // threshold 0, no data: the graph, weights 1.0
    expect(s.rc == 0 && s.counts[0] == 13 && s.counts[1] == 0 && s.indptr == L_INDPTR && s.indices == L_INDICES && s.data == std::vector<float>(13, 1.f) &&
               s.u[0] == 77, "threshold 0 returns the graph");
    words.assign(13, 0xfffffffeu);
    s = split(L_INDPTR, L_INDICES, &L_DATA, 0, 0, 0xffffffffu, words);
    expect(s.rc == 0 && s.counts[1] == 5, "a word just below the largest threshold is held out");
    words.assign(13, 0xffffffffu);
    s = split(L_INDPTR, L_INDICES, &L_DATA, 0, 0, 0xffffffffu, words);
    expect(s.rc == 0 && s.counts[1] == 0, "the comparison is strict");
}

void check_directed_and_refusals() {
    // directed: 0 -> [0, 2], 1 -> [0], 2 -> [], 3 -> [1, 2, 3]; units at 1, 2, 3, 4; f = 1, 2, none, 3
    const std::vector<uint32_t> indptr = {0, 2, 3, 3, 6}, indices = {0, 2, 0, 1, 2, 3};
    const std::vector<uint32_t> words(6, 1);
    Split s = split(indptr, indices, nullptr, 1, 1, 2, words);
    expect(s.rc == 0 && s.counts[0] == 5 && s.counts[1] == 1 && s.counts[2] == 4 && s.counts[3] == 3 && s.u[0] == 3 && s.v[0] == 2 && s.weight[0] == 1.f,
           "directed: only the second entry of row 3 is free");
    s = split(indptr, indices, nullptr, 1, 0, 2, words);
    expect(s.rc == 0 && s.counts[0] == 2 && s.counts[1] == 4 && starts_with(s.u, {0, 1, 3, 3}) && starts_with(s.v, {2, 0, 1, 2}) &&
               s.indptr == std::vector<uint32_t>({0, 1, 1, 1, 2}), "directed, bare: the loops stay");
    s = split(indptr, indices, nullptr, 0, 1, 2, words);   // as an undirected graph: 0 -> 2 at position 1 has no mate
    expect(s.rc == pw::HO_HOST_MISSING && s.where == 1 && s.indptr[0] == 77 && s.indices[0] == 77 && s.u[0] == 77 && s.weight[0] == 77.f && s.counts[0] == 77,
           "a missing mate is named and nothing is written");
    const std::vector<uint32_t> none = {0, 0}, no_entries;
    s = split(none, no_entries, nullptr, 0, 1, 5, no_entries);
    expect(s.rc == 0 && s.counts[0] == 0 && s.counts[1] == 0 && s.counts[2] == 0 && s.indptr == none, "one vertex, no entry");
}

}  // namespace

int main() {
    check_parts();
    check_loops_graph();
    check_directed_and_refusals();
    printf(failures ? "holdout_selfcheck: %d failures\n" : "holdout_selfcheck: ok\n", failures);
    return failures ? 1 : 0;
}
