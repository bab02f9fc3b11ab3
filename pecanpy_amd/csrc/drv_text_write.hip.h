#pragma once
// Host driver, text files written from device memory: the word2vec vectors file (emb_text.hip.h) and the walk corpus file
// (walk_text.hip.h), the state they share (TextFile), and the self tests of the %.6f text and of the scan (scan.hip.h).
// Exports pw_vectors_write_text*, pw_walks_write_text*, pw_selftest_format_f6, pw_selftest_exclusive_scan.
#include "drv_core.hip.h"
#include "scan.hip.h"
#include "emb_text.hip.h"
#include "walk_text.hip.h"

// ---- the word2vec text file written from device memory (csrc/emb_text.hip.h) -------------------------------------------------
namespace {

constexpr uint64_t EMB_CHUNK_DEFAULT = 32ull << 20;   // bytes of text per chunk: PECANPY_AMD_EMB_CHUNK_BYTES overrides

// What a call that writes a text file from device memory owns -- released on every way out -- and the part the embedding
// writer and the walk writer share: the scan of the row byte counts, then consecutive rows in chunks that fit a byte budget,
// through one device buffer and two pinned host buffers.  A writer opens the file (with its header line, if it has one),
// allocates and uploads what its kernels read, launches its count kernel between count_begin and count_end, and hands
// write_chunks a callable that launches its fill kernel for rows [lo, hi).
struct TextFile {
    const std::string who;   // the entry's name in the error texts
    const std::string path;
    FILE *file = nullptr;
    PinnedBuf<void> pinned[2];
    bool queued = false;   // work may be in flight on the default stream
    pw::Event ev[8];       // count begin / end; per chunk slot: fill begin, fill end, copy end
    int n_cu = 1;
    DevBuf<uint64_t> d_row_off, d_tmp;       // uint64[n_rows + 1]: byte counts, then offsets; the scan's tile sums
    DevBuf<uint32_t> d_flags;                // one word the fill kernel raises
    DevBuf<char> d_ids, d_buf;               // the names' characters; the text of one chunk
    DevBuf<uint64_t> d_id_off;               // the names' offsets
    std::vector<uint64_t> row_off;                     // host copy: row_off[i] = offset of row i behind the header, [n_rows] = total
    double format_ms = 0, copy_ms = 0, write_ms = 0;
    uint64_t header_bytes = 0, n_chunks = 0;

    TextFile(const char *who_, const char *path_) : who(who_), path(path_) {}
    TextFile(const TextFile &) = delete;
    ~TextFile() {   // (the buffers go behind this body: nothing of the call is in flight by then)
        if (queued) (void)hipStreamSynchronize(nullptr);
        if (file) (void)fclose(file);
    }
    int write_failed() const { return fail(PW_ERR_INVALID, who + ": cannot write " + path + ": " + strerror(errno)); }
    int open(const std::string &header) {
        file = fopen(path.c_str(), "wb");
        if (!file) return fail(PW_ERR_INVALID, who + ": cannot open " + path + ": " + strerror(errno));
        if (fwrite(header.data(), 1, header.size(), file) != header.size()) return write_failed();
        header_bytes = header.size();
        return 0;
    }
    int begin(int device) {
        HIP_TRY(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        n_cu = prop.multiProcessorCount;
        queued = true;
        for (auto &e : ev) HIP_TRY(e.create(hipEventDefault));
        return 0;
    }
    template <typename T> int alloc(DevBuf<T> &buf, uint64_t n) {
        const hipError_t e = buf.alloc(n);
        if (e == hipSuccess) return 0;
        return fail(PW_ERR_NOMEM, who + ": " + std::to_string(n * sizeof(T)) + " bytes do not fit in device memory: " + hipGetErrorString(e));
    }
    // the names of the call on the device, and the per-row buffers of the count pass
    int alloc_rows(uint64_t n_rows, const char *id_chars, const uint64_t *id_offsets, uint64_t n_names) {
        int rc;
        if ((rc = alloc(d_ids, id_offsets[n_names])) || (rc = alloc(d_id_off, n_names + 1)) || (rc = alloc(d_row_off, n_rows + 1)) ||
            (rc = alloc(d_tmp, pw::scan_scratch_elems(n_rows + 1))) || (rc = alloc(d_flags, 1)))
            return rc;
        if (id_offsets[n_names]) HIP_TRY(hipMemcpyAsync(d_ids.p, id_chars, id_offsets[n_names], hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(d_id_off.p, id_offsets, sizeof(uint64_t) * (n_names + 1), hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemsetAsync(d_flags.p, 0, sizeof(uint32_t), nullptr));
        HIP_TRY(hipMemsetAsync(d_row_off.p + n_rows, 0, sizeof(uint64_t), nullptr));   // (the scan's last input: its output is the total)
        return 0;
    }
    // blocks of four wavefronts for one wavefront per row, rows strided over the grid
    unsigned grid(uint64_t rows) const { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((rows + 3) / 4, (uint64_t)n_cu * 16)); }

    // count pass and scan: the writer's count kernel, launched between the two, leaves row i's byte count in d_row_off[i]
    int count_begin() {
        HIP_TRY(hipEventRecord(ev[0], nullptr));
        return 0;
    }
    int count_end(uint64_t n_rows) {
        pw::exclusive_scan_inplace(nullptr, d_row_off.p, n_rows + 1, d_tmp.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[1], nullptr));
        row_off.resize(n_rows + 1);
        HIP_TRY(hipMemcpyAsync(row_off.data(), d_row_off.p, sizeof(uint64_t) * (n_rows + 1), hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        format_ms = ms;
        return 0;
    }
    uint64_t bytes() const { return header_bytes + row_off.back(); }

    // fill(lo, hi, blocks, d_buf) launches the fill kernel for rows [lo, hi) on the default stream: their text at
    // d_buf[row_off[row] - row_off[lo]].  budget >= row_max >= the bytes of any one row.  Closes the file.
    template <typename Fill> int write_chunks(uint64_t budget, uint64_t row_max, Fill fill) {
        const uint64_t n_rows = row_off.size() - 1, total = row_off[n_rows];
        for (uint64_t i = 0; i < n_rows; i++)   // (what the fill pass is bounded by: checked before anything is written through it)
            if (row_off[i + 1] < row_off[i] || row_off[i + 1] - row_off[i] > row_max)
                return fail(PW_ERR_HIP, who + ": row byte counts out of range (internal error)");

        // chunks: consecutive rows while their text fits the budget (one row always does)
        const uint64_t buf_bytes = std::min(budget, total);
        int rc;
        if ((rc = alloc(d_buf, buf_bytes))) return rc;
        for (auto &p : pinned) {
            const hipError_t e = p.alloc(buf_bytes);
            if (e != hipSuccess) return fail(PW_ERR_NOMEM, who + ": pinned host buffer: " + hipGetErrorString(e));
        }
        struct Chunk { uint64_t lo, hi; };
        auto next_chunk = [&](uint64_t lo) {
            // the last row whose end lies within the budget from row lo's start
            const uint64_t limit = row_off[lo] + buf_bytes;
            const uint64_t hi = (uint64_t)(std::upper_bound(row_off.begin() + lo + 1, row_off.end(), limit) - row_off.begin()) - 1;
            return Chunk{lo, hi};
        };
        // slot s = chunk index & 1: events 2 + 3 s .. 4 + 3 s = fill begin, fill end, copy end
        auto issue = [&](const Chunk &c, int s) -> int {
            HIP_TRY(hipEventRecord(ev[2 + 3 * s], nullptr));
            fill(c.lo, c.hi, grid(c.hi - c.lo), d_buf.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev[3 + 3 * s], nullptr));
            HIP_TRY(hipMemcpyAsync(pinned[s].p, d_buf.p, row_off[c.hi] - row_off[c.lo], hipMemcpyDeviceToHost, nullptr));
            HIP_TRY(hipEventRecord(ev[4 + 3 * s], nullptr));
            return 0;
        };
        using clk = std::chrono::steady_clock;
        Chunk cur = next_chunk(0);
        if ((rc = issue(cur, 0))) return rc;
        while (true) {
            const int s = (int)(n_chunks & 1);
            Chunk nxt{cur.hi, cur.hi};
            if (cur.hi < n_rows) {   // the copy of the next chunk runs beside this chunk's fwrite
                nxt = next_chunk(cur.hi);
                if ((rc = issue(nxt, s ^ 1))) return rc;
            }
            HIP_TRY(hipEventSynchronize(ev[4 + 3 * s]));
            float ms_fill = 0, ms_copy = 0;
            HIP_TRY(hipEventElapsedTime(&ms_fill, ev[2 + 3 * s], ev[3 + 3 * s]));
            HIP_TRY(hipEventElapsedTime(&ms_copy, ev[3 + 3 * s], ev[4 + 3 * s]));
            format_ms += ms_fill;
            copy_ms += ms_copy;
            const uint64_t bytes = row_off[cur.hi] - row_off[cur.lo];
            const auto t0 = clk::now();
            if (fwrite(pinned[s].p, 1, bytes, file) != bytes) return write_failed();
            write_ms += std::chrono::duration<double, std::milli>(clk::now() - t0).count();
            n_chunks++;
            if (cur.hi >= n_rows) break;
            cur = nxt;
        }
        uint32_t flags = 0;
        HIP_TRY(hipMemcpyAsync(&flags, d_flags.p, sizeof(flags), hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        if (flags) return fail(PW_ERR_HIP, who + ": the fill pass disagreed with the count pass (internal error)");
        const auto t0 = clk::now();
        FILE *f = file;
        file = nullptr;
        if (fclose(f) != 0) return write_failed();
        write_ms += std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        return 0;
    }
};

// the names of a writer call: offsets that ascend, the longest name; `what` is what one name belongs to in the error text
int check_names(const char *who, const char *what, const char *id_chars, const uint64_t *id_offsets, uint64_t n_names,
                uint64_t *longest_name) {
    *longest_name = 0;
    for (uint64_t i = 0; i < n_names; i++) {
        if (id_offsets[i + 1] < id_offsets[i])
            return fail(PW_ERR_INVALID, std::string(who) + ": id_offsets do not ascend at " + what + " " + std::to_string(i));
        *longest_name = std::max(*longest_name, id_offsets[i + 1] - id_offsets[i]);
    }
    if (id_offsets[n_names] && !id_chars) return fail(PW_ERR_INVALID, "null pointer");
    return 0;
}

uint64_t chunk_budget(const char *env_name, uint64_t row_max) {   // bytes of text per chunk: at least what one row can take
    uint64_t budget = EMB_CHUNK_DEFAULT;
    if (const char *v = getenv(env_name))
        if (*v) budget = (uint64_t)strtoull(v, nullptr, 10);
    return std::max(budget, row_max);
}

}  // namespace

PW_EXPORT int pw_vectors_write_text_device(int device, const float *d_vectors, uint64_t n_rows, uint32_t dim, const char *id_chars,
                                           const uint64_t *id_offsets, const char *path, pw_emb_write_stats *stats) {
    const char *who = "pw_vectors_write_text";
    if (!d_vectors || !id_offsets || !path) return fail(PW_ERR_INVALID, "null pointer");
    if (n_rows == 0 || dim == 0) return fail(PW_ERR_INVALID, "pw_vectors_write_text: n_rows and dim must be positive");
    uint64_t longest_name = 0;
    int rc;
    if ((rc = check_names(who, "row", id_chars, id_offsets, n_rows, &longest_name))) return rc;
    if ((rc = check_device(device))) return rc;
    // the byte budget of a chunk: at least what one row can take (name, dim times " " + 47 characters, newline)
    const uint64_t row_max = longest_name + (uint64_t)dim * pw::F6_SLOT + 1;
    const uint64_t budget = chunk_budget("PECANPY_AMD_EMB_CHUNK_BYTES", row_max);

    TextFile out(who, path);
    if ((rc = out.open(std::to_string(n_rows) + " " + std::to_string(dim) + "\n")) || (rc = out.begin(device))) return rc;
    if ((rc = out.alloc_rows(n_rows, id_chars, id_offsets, n_rows))) return rc;

    if ((rc = out.count_begin())) return rc;
    hipLaunchKernelGGL(pw::emb_count_kernel, dim3(out.grid(n_rows)), dim3(256), 0, nullptr, d_vectors, n_rows, dim, (const uint64_t *)out.d_id_off.p,
                       out.d_row_off.p);
    if ((rc = out.count_end(n_rows))) return rc;
    rc = out.write_chunks(budget, row_max, [&](uint64_t lo, uint64_t hi, unsigned blocks, char *d_buf) {
        hipLaunchKernelGGL(pw::emb_fill_kernel, dim3(blocks), dim3(256), 0, nullptr, d_vectors, lo, hi, dim, (const char *)out.d_ids.p,
                           (const uint64_t *)out.d_id_off.p, (const uint64_t *)out.d_row_off.p, d_buf, out.d_flags.p);
    });
    if (rc) return rc;
    if (stats) {
        stats->format_ms = out.format_ms; stats->copy_ms = out.copy_ms; stats->write_ms = out.write_ms;
        stats->bytes = out.bytes();
        stats->chunks = out.n_chunks;
    }
    return PW_OK;
}

// host-matrix entry: upload, then the device entry
PW_EXPORT int pw_vectors_write_text(int device, const float *vectors, uint64_t n_rows, uint32_t dim, const char *id_chars,
                                    const uint64_t *id_offsets, const char *path, pw_emb_write_stats *stats) {
    if (!vectors || !id_offsets || !path) return fail(PW_ERR_INVALID, "null pointer");
    if (n_rows == 0 || dim == 0) return fail(PW_ERR_INVALID, "pw_vectors_write_text: n_rows and dim must be positive");
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t vbytes = sizeof(float) * (size_t)n_rows * dim;
    DevBuf<float> d_vectors;
    hipError_t e = d_vectors.alloc((size_t)n_rows * dim);
    if (e != hipSuccess)
        return fail(PW_ERR_NOMEM, std::string("pw_vectors_write_text: the matrix does not fit in device memory: ") + hipGetErrorString(e));
    e = hipMemcpy(d_vectors.p, vectors, vbytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? pw_vectors_write_text_device(device, d_vectors.p, n_rows, dim, id_chars, id_offsets, path, stats)
                             : fail(PW_ERR_HIP, std::string("pw_vectors_write_text: ") + hipGetErrorString(e));
    return rc;
}

// ---- the walk corpus file written from device memory (csrc/walk_text.hip.h) ---------------------------------------------------
PW_EXPORT int pw_walks_write_text_device(int device, const uint32_t *d_walks, uint64_t n_walks, uint32_t walk_length,
                                         const char *id_chars, const uint64_t *id_offsets, uint64_t n_names, const char *path,
                                         pw_walks_write_stats *stats) {
    const char *who = "pw_walks_write_text";
    if ((n_walks && !d_walks) || !id_offsets || !path) return fail(PW_ERR_INVALID, "null pointer");
    if (walk_length >= (1u << 31)) return fail(PW_ERR_INVALID, "pw_walks_write_text: walk_length must be below 2^31");
    uint64_t longest_name = 0;
    int rc;
    if ((rc = check_names(who, "name", id_chars, id_offsets, n_names, &longest_name))) return rc;
    if (longest_name > pw::WALK_NAME_MAX)
        return fail(PW_ERR_INVALID, "pw_walks_write_text: a name of " + std::to_string(longest_name) + " bytes (at most " +
                                        std::to_string(pw::WALK_NAME_MAX) + ")");
    if ((rc = check_device(device))) return rc;
    // the byte budget of a chunk: at least the longest possible row, walk_length + 1 times the longest name and its separator
    const uint64_t row_max = ((uint64_t)walk_length + 1) * (longest_name + 1);
    const uint64_t budget = chunk_budget("PECANPY_AMD_WALKS_CHUNK_BYTES", row_max);

    DevBuf<unsigned long long> d_found;   // the count kernel's findings: lowest row with a bad length, with a bad token; tokens
                                          // (declared before `out`: it goes after ~TextFile has waited for the stream)
    TextFile out(who, path);
    if ((rc = out.open(""))) return rc;
    if (stats) *stats = pw_walks_write_stats{0, 0, 0, 0, 0, 0, 0};
    if (n_walks == 0) {   // the empty file
        FILE *f = out.file;
        out.file = nullptr;
        return fclose(f) == 0 ? PW_OK : out.write_failed();
    }
    if ((rc = out.begin(device))) return rc;
    if ((rc = out.alloc_rows(n_walks, id_chars, id_offsets, n_names)) || (rc = out.alloc(d_found, 3))) return rc;
    HIP_TRY(hipMemsetAsync(d_found.p, 0xff, sizeof(unsigned long long) * 2, nullptr));
    HIP_TRY(hipMemsetAsync(d_found.p + 2, 0, sizeof(unsigned long long), nullptr));

    if ((rc = out.count_begin())) return rc;
    hipLaunchKernelGGL(pw::walk_text_count_kernel, dim3(out.grid(n_walks)), dim3(256), 0, nullptr, d_walks, n_walks, walk_length,
                       (const uint64_t *)out.d_id_off.p, n_names, out.d_row_off.p, d_found.p);
    if ((rc = out.count_end(n_walks))) return rc;
    unsigned long long found[3];
    HIP_TRY(hipMemcpy(found, d_found.p, sizeof(found), hipMemcpyDeviceToHost));
    const uint64_t width = (uint64_t)walk_length + 2;
    if (found[0] != ~0ull) {   // nothing of the matrix was looked up, and no fill pass runs: the file stays empty
        uint32_t len = 0;
        HIP_TRY(hipMemcpy(&len, d_walks + found[0] * width + walk_length + 1, sizeof(len), hipMemcpyDeviceToHost));
        return fail(PW_ERR_INVALID, "pw_walks_write_text: row length " + std::to_string(len) + " in row " + std::to_string(found[0]) +
                                        " exceeds walk_length + 1 = " + std::to_string((uint64_t)walk_length + 1));
    }
    if (found[1] != ~0ull) {
        std::vector<uint32_t> row(width);
        HIP_TRY(hipMemcpy(row.data(), d_walks + found[1] * width, sizeof(uint32_t) * width, hipMemcpyDeviceToHost));
        uint64_t c = 0;
        while (c < row[walk_length + 1] && row[c] < n_names) c++;
        return fail(PW_ERR_INVALID, "pw_walks_write_text: node index " + std::to_string(row[c]) + " at position " + std::to_string(c) +
                                        " of row " + std::to_string(found[1]) + " outside the " + std::to_string(n_names) + " names");
    }
    rc = out.write_chunks(budget, row_max, [&](uint64_t lo, uint64_t hi, unsigned blocks, char *d_buf) {
        hipLaunchKernelGGL(pw::walk_text_fill_kernel, dim3(blocks), dim3(256), 0, nullptr, d_walks, lo, hi, walk_length, (const char *)out.d_ids.p,
                           (const uint64_t *)out.d_id_off.p, n_names, (const uint64_t *)out.d_row_off.p, d_buf, out.d_flags.p);
    });
    if (rc) return rc;
    if (stats) {
        stats->format_ms = out.format_ms; stats->copy_ms = out.copy_ms; stats->write_ms = out.write_ms;
        stats->bytes = out.bytes();
        stats->chunks = out.n_chunks;
        stats->rows = n_walks;
        stats->tokens = found[2];
    }
    return PW_OK;
}

// host-matrix entry: upload, then the device entry
PW_EXPORT int pw_walks_write_text(int device, const uint32_t *walks, uint64_t n_walks, uint32_t walk_length, const char *id_chars,
                                  const uint64_t *id_offsets, uint64_t n_names, const char *path, pw_walks_write_stats *stats) {
    if (n_walks == 0 || !walks || walk_length >= (1u << 31))   // (nothing to upload, or refused there)
        return pw_walks_write_text_device(device, nullptr, n_walks, walk_length, id_chars, id_offsets, n_names, path, stats);
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t wbytes = sizeof(uint32_t) * (size_t)n_walks * ((size_t)walk_length + 2);
    DevBuf<uint32_t> d_walks;
    hipError_t e = d_walks.alloc((size_t)n_walks * ((size_t)walk_length + 2));
    if (e != hipSuccess)
        return fail(PW_ERR_NOMEM, std::string("pw_walks_write_text: the matrix does not fit in device memory: ") + hipGetErrorString(e));
    e = hipMemcpy(d_walks.p, walks, wbytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? pw_walks_write_text_device(device, d_walks.p, n_walks, walk_length, id_chars, id_offsets, n_names, path, stats)
                             : fail(PW_ERR_HIP, std::string("pw_walks_write_text: ") + hipGetErrorString(e));
    return rc;
}

// x[i] formatted into chars[48 i ..) (the rest of the slot zero), lens[i] = the count.  on_device = 0: the host build of
// format_f6; on_device = 1: one GPU thread per value.
PW_EXPORT int pw_selftest_format_f6(int on_device, int device, const float *x, uint64_t n, char *chars, uint32_t *lens) {
    if (n && (!x || !chars || !lens)) return fail(PW_ERR_INVALID, "null pointer");
    if (n == 0) return PW_OK;
    if (!on_device) {
        memset(chars, 0, (size_t)n * pw::F6_SLOT);
        for (uint64_t i = 0; i < n; i++) {
            const pw::F6 f = pw::f6_decompose(x[i]);
            const uint32_t len = pw::f6_emit(f, chars + i * pw::F6_SLOT);
            lens[i] = len == pw::f6_len(f) ? len : 0xffffffffu;
        }
        return PW_OK;
    }
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> d_x;
    DevBuf<char> d_chars;
    DevBuf<uint32_t> d_lens;
    const size_t cbytes = (size_t)n * pw::F6_SLOT;
    hipError_t e = d_x.alloc(n);
    if (e == hipSuccess) e = d_chars.alloc(cbytes);
    if (e == hipSuccess) e = d_lens.alloc(n);
    if (e == hipSuccess) e = hipMemcpy(d_x.p, x, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_chars.p, 0, cbytes);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pw::f6_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const float *)d_x.p, n, d_chars.p, d_lens.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(chars, d_chars.p, cbytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(lens, d_lens.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_selftest_format_f6: ") + hipGetErrorString(e));
    return PW_OK;
}

// x[0, n) of uint32 (width 32) or uint64 (width 64) in host memory -> its exclusive scan in place, *total = the sum, through
// scan.hip.h's entry on the null stream
template <typename T> static int selftest_exclusive_scan(T *x, uint64_t n, uint64_t *total) {
    DevBuf<T> d_x, d_scratch;
    T sum = 0;
    hipError_t e = d_x.alloc(n + 1);
    if (e == hipSuccess) e = d_scratch.alloc(pw::scan_scratch_elems(n));
    if (e == hipSuccess && n) e = hipMemcpy(d_x.p, x, sizeof(T) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        pw::exclusive_scan_inplace(nullptr, d_x.p, n, d_scratch.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n) e = hipMemcpy(x, d_x.p, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&sum, d_scratch.p, sizeof(T), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PW_ERR_HIP, std::string("pw_selftest_exclusive_scan: ") + hipGetErrorString(e));
    *total = sum;
    return PW_OK;
}

PW_EXPORT int pw_selftest_exclusive_scan(int device, int width, void *x, uint64_t n, uint64_t *total) {
    if ((n && !x) || !total || (width != 32 && width != 64)) return fail(PW_ERR_INVALID, "bad argument");
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    return width == 32 ? selftest_exclusive_scan((uint32_t *)x, n, total) : selftest_exclusive_scan((uint64_t *)x, n, total);
}
