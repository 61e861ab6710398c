// host_capi.cpp -- implementation of include/sbwthost.h (GPU-free host helpers).
#include "../../../include/sbwthost.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "index_builder.hh"
#include "index_file.hh"
#include "occurrences_file.hh"
#include "positions_file.hh"
#include "seqio.hh"

namespace {
thread_local char g_err[512] = "";
int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}
}  // namespace

struct sbwthost_bits { sbwt::PlainMatrixBits b; };
struct sbwthost_file { sbwt::IndexFileData f; };

extern "C" {

const char *sbwthost_last_error(void) { return g_err; }

int sbwthost_build(const char *const *seqs, const int64_t *seq_lens, int64_t n_seqs, int64_t k, int add_revcomp,
                   int build_ssup, int n_threads, sbwthost_bits **out) {
    if (!out || n_seqs < 0 || (n_seqs > 0 && (!seqs || !seq_lens))) return fail("invalid argument");
    if (k < 2 || k > 255) return fail("Error: this builder supports 2 <= k <= 255");
    try {
        std::vector<std::string> v;
        v.reserve((size_t)n_seqs);
        for (int64_t i = 0; i < n_seqs; i++) v.emplace_back(seqs[i], (size_t)seq_lens[i]);
        sbwthost_bits *r = new sbwthost_bits();
        r->b = sbwt::build_plain_matrix_bits(v, (int)k, add_revcomp != 0, build_ssup != 0, n_threads);
        *out = r;
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}
void sbwthost_bits_free(sbwthost_bits *b) { delete b; }
int sbwthost_bits_info(const sbwthost_bits *b, int64_t *n_nodes, int64_t *n_kmers, int64_t *k, int *has_ssup) {
    if (!b) return fail("NULL handle");
    if (n_nodes) *n_nodes = b->b.n_nodes;
    if (n_kmers) *n_kmers = b->b.n_kmers;
    if (k) *k = b->b.k;
    if (has_ssup) *has_ssup = !b->b.ssup.empty();
    return 0;
}
const uint64_t *sbwthost_bits_words(const sbwthost_bits *b, int which) {
    if (!b) return nullptr;
    switch (which) {
        case 0: return b->b.A.data();
        case 1: return b->b.C.data();
        case 2: return b->b.G.data();
        case 3: return b->b.T.data();
        case 4: return b->b.ssup.empty() ? nullptr : b->b.ssup.data();
        default: return nullptr;
    }
}

int sbwthost_file_write(const char *path, int64_t n_nodes, const uint64_t *A, const uint64_t *C, const uint64_t *G,
                        const uint64_t *T, const uint64_t *ssup, const int64_t C_array[4], const int64_t *precalc_pairs,
                        int64_t precalc_k, int64_t n_kmers, int64_t k) {
    if (!path || !A || !C || !G || !T || !C_array || n_nodes <= 0 || precalc_k < 0 || precalc_k > 20 ||
        (precalc_k > 0 && !precalc_pairs))
        return fail("invalid argument");
    try {
        sbwt::IndexFileData f;
        f.A_bits = sbwt::bit_vector(A, n_nodes);
        f.C_bits = sbwt::bit_vector(C, n_nodes);
        f.G_bits = sbwt::bit_vector(G, n_nodes);
        f.T_bits = sbwt::bit_vector(T, n_nodes);
        if (ssup) f.suffix_group_starts = sbwt::bit_vector(ssup, n_nodes);
        f.C.assign(C_array, C_array + 4);
        size_t np = precalc_k ? ((size_t)1 << (2 * precalc_k)) : 0;
        f.kmer_prefix_precalc.resize(np);
        if (np) memcpy((void *)f.kmer_prefix_precalc.data(), precalc_pairs, np * 16);
        f.precalc_k = precalc_k; f.n_nodes = n_nodes; f.n_kmers = n_kmers; f.k = k;
        std::ofstream out(path, std::ios::binary);
        if (!out.good()) return fail("Error opening file: %s", path);
        sbwt::serialize_string("plain-matrix", out);
        f.serialize(out);
        out.flush();
        if (!out.good()) return fail("Error writing to file %s", path);
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}

int sbwthost_file_read(const char *path, sbwthost_file **out) {
    if (!path || !out) return fail("invalid argument");
    try {
        std::ifstream in(path, std::ios::binary);
        if (!in.good()) return fail("Error opening file: %s", path);
        std::string variant = sbwt::load_string(in);
        if (variant != "plain-matrix") return fail("Error: not a plain-matrix index (variant '%s')", variant.c_str());
        sbwthost_file *r = new sbwthost_file();
        try {
            r->f.load(in);
        } catch (...) {
            delete r;
            throw;
        }
        *out = r;
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}
void sbwthost_file_free(sbwthost_file *f) { delete f; }
int sbwthost_file_info(const sbwthost_file *f, int64_t *n_nodes, int64_t *n_kmers, int64_t *k, int64_t *precalc_k,
                       int64_t C_array[4], int *has_ssup) {
    if (!f) return fail("NULL handle");
    if (n_nodes) *n_nodes = f->f.n_nodes;
    if (n_kmers) *n_kmers = f->f.n_kmers;
    if (k) *k = f->f.k;
    if (precalc_k) *precalc_k = f->f.precalc_k;
    if (C_array) for (int i = 0; i < 4; i++) C_array[i] = f->f.C[(size_t)i];
    if (has_ssup) *has_ssup = f->f.suffix_group_starts.size() > 0;
    return 0;
}
const uint64_t *sbwthost_file_words(const sbwthost_file *f, int which) {
    if (!f) return nullptr;
    switch (which) {
        case 0: return f->f.A_bits.data();
        case 1: return f->f.C_bits.data();
        case 2: return f->f.G_bits.data();
        case 3: return f->f.T_bits.data();
        case 4: return f->f.suffix_group_starts.size() ? f->f.suffix_group_starts.data() : nullptr;
        default: return nullptr;
    }
}
const int64_t *sbwthost_file_precalc(const sbwthost_file *f) {
    return (f && !f->f.kmer_prefix_precalc.empty()) ? (const int64_t *)f->f.kmer_prefix_precalc.data() : nullptr;
}

int sbwthost_read_sequences(const char *path, char **bases, int64_t **read_off, int64_t *n_reads) {
    if (!path || !bases || !read_off || !n_reads) return fail("invalid argument");
    try {
        sbwt::seq_io::Reader reader(path);
        std::vector<char> b;
        std::vector<int64_t> off{0};
        for (;;) {
            int64_t len = reader.get_next_read_to_buffer();
            if (len == 0) break;
            b.insert(b.end(), reader.read_buf, reader.read_buf + len);
            off.push_back((int64_t)b.size());
        }
        *bases = (char *)malloc(b.size() ? b.size() : 1);
        *read_off = (int64_t *)malloc(off.size() * 8);
        if (!*bases || !*read_off) return fail("out of memory");
        if (!b.empty()) memcpy(*bases, b.data(), b.size());
        memcpy(*read_off, off.data(), off.size() * 8);
        *n_reads = (int64_t)off.size() - 1;
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}
int sbwthost_read_sequences_chunked(const char *path, int64_t chunk_bytes, int n_threads, char **bases, int64_t **read_off,
                                    int64_t *n_reads) {
    if (!path || !bases || !read_off || !n_reads) return fail("invalid argument");
    try {
        int64_t size = 0;
        if (!sbwt::seq_io::chunkable_file(path, &size)) return 1;
        std::vector<char> b;
        std::vector<int64_t> off{0};
        sbwt::seq_io::read_file_chunked(path, size, chunk_bytes, n_threads,
                                        [&](std::vector<char> &&pb, std::vector<int64_t> &&po, bool) {
                                            const int64_t base = (int64_t)b.size();
                                            b.insert(b.end(), pb.begin(), pb.end());
                                            for (size_t r = 1; r < po.size(); r++) off.push_back(base + po[r]);
                                        });
        *bases = (char *)malloc(b.size() ? b.size() : 1);
        *read_off = (int64_t *)malloc(off.size() * 8);
        if (!*bases || !*read_off) return fail("out of memory");
        if (!b.empty()) memcpy(*bases, b.data(), b.size());
        memcpy(*read_off, off.data(), off.size() * 8);
        *n_reads = (int64_t)off.size() - 1;
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}
void sbwthost_free(void *p) { free(p); }

int sbwthost_write_file(const char *path, const char *data, int64_t n, int gzip_output, int n_threads) {
    if (!path || n < 0 || (n > 0 && !data)) return fail("invalid argument");
    try {
        sbwt::seq_io::Buffered_ofstream out(path, gzip_output != 0, n_threads);
        for (int64_t pos = 0; pos < n; pos += 3000000) out.write(data + pos, std::min<int64_t>(3000000, n - pos));
        out.close();
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}

int sbwthost_rank_batch(const uint64_t *bits, int64_t n_bits, const int64_t *pos, int64_t n, int64_t *out) {
    if (n_bits < 0 || n < 0 || (n_bits > 0 && !bits) || (n > 0 && (!pos || !out))) return fail("invalid argument");
    try {
        const sbwt::bit_vector v(bits, n_bits);
        sbwt::rank_support_v5_blob rs;
        rs.build(v);
        for (int64_t i = 0; i < n; i++) {
            if (pos[i] < 0 || pos[i] > n_bits) return fail("position %lld outside [0, %lld]", (long long)pos[i], (long long)n_bits);
            out[i] = rs.rank(v, pos[i]);
        }
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}

// ---- colour files: "SBWTCOL1", int64 n_columns, n_colors, k, then n_columns little-endian uint64 rows ----
static const char COLORS_MAGIC[8] = {'S', 'B', 'W', 'T', 'C', 'O', 'L', '1'};

int sbwthost_colors_write(const char *path, const uint64_t *rows, int64_t n_columns, int64_t n_colors, int64_t k) {
    if (!path || n_columns < 0 || (n_columns > 0 && !rows)) return fail("invalid argument");
    if (n_colors < 1 || n_colors > 64) return fail("Error: n_colors must be in 1 .. 64, not %lld", (long long)n_colors);
    std::ofstream out(path, std::ios::binary);
    if (!out.good()) return fail("Error opening file: %s", path);
    const int64_t head[3] = {n_columns, n_colors, k};
    out.write(COLORS_MAGIC, 8);
    out.write(reinterpret_cast<const char *>(head), 24);
    if (n_columns > 0) out.write(reinterpret_cast<const char *>(rows), (std::streamsize)(n_columns * 8));
    out.flush();
    if (!out.good()) return fail("Error writing to file %s", path);
    return 0;
}

int sbwthost_colors_read(const char *path, int64_t *n_columns, int64_t *n_colors, int64_t *k, uint64_t *rows_or_null,
                         int64_t rows_cap) {
    if (!path) return fail("invalid argument");
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) return fail("Error opening file: %s", path);
    char magic[8];
    int64_t head[3];
    in.read(magic, 8);
    if (in.gcount() != 8) return fail("Error: colour file %s is truncated (no magic)", path);
    if (memcmp(magic, COLORS_MAGIC, 8) != 0) return fail("Error: %s is not a colour file (wrong magic, SBWTCOL1 expected)", path);
    in.read(reinterpret_cast<char *>(head), 24);
    if (in.gcount() != 24) return fail("Error: colour file %s is truncated (header)", path);
    if (head[1] < 1 || head[1] > 64) return fail("Error: colour file %s: n_colors = %lld is outside 1 .. 64", path, (long long)head[1]);
    if (head[0] < 0 || head[0] > ((int64_t)1 << 56)) return fail("Error: colour file %s: n_columns = %lld", path, (long long)head[0]);
    in.seekg(0, std::ios::end);
    const int64_t size = (int64_t)in.tellg(), want = 32 + head[0] * 8;
    if (size < want)
        return fail("Error: colour file %s is truncated (%lld bytes, %lld columns need %lld)", path, (long long)size, (long long)head[0],
                    (long long)want);
    if (size > want) return fail("Error: colour file %s has %lld bytes after its %lld rows", path, (long long)(size - want), (long long)head[0]);
    if (n_columns) *n_columns = head[0];
    if (n_colors) *n_colors = head[1];
    if (k) *k = head[2];
    if (!rows_or_null) return 0;
    if (rows_cap < head[0]) return fail("Error: room for %lld rows, the colour file holds %lld", (long long)rows_cap, (long long)head[0]);
    in.seekg(32, std::ios::beg);
    if (head[0] > 0) in.read(reinterpret_cast<char *>(rows_or_null), (std::streamsize)(head[0] * 8));
    if (!in.good()) return fail("Error reading %s", path);
    return 0;
}

// ---- wide colour files: "SBWTCOL2", int64 n_columns, n_colors, k, words_per_row, then n_columns x words_per_row words ----
static const char COLORS_MAGIC_WIDE[8] = {'S', 'B', 'W', 'T', 'C', 'O', 'L', '2'};

int sbwthost_colors_write_wide(const char *path, const uint64_t *rows, int64_t n_columns, int64_t n_colors, int64_t k) {
    if (!path || n_columns < 0 || (n_columns > 0 && !rows)) return fail("invalid argument");
    if (n_colors < 1 || n_colors > 4096) return fail("Error: n_colors must be in 1 .. 4096, not %lld", (long long)n_colors);
    std::ofstream out(path, std::ios::binary);
    if (!out.good()) return fail("Error opening file: %s", path);
    const int64_t words = (n_colors + 63) / 64;
    const int64_t head[4] = {n_columns, n_colors, k, words};
    out.write(COLORS_MAGIC_WIDE, 8);
    out.write(reinterpret_cast<const char *>(head), 32);
    if (n_columns > 0) out.write(reinterpret_cast<const char *>(rows), (std::streamsize)(n_columns * words * 8));
    out.flush();
    if (!out.good()) return fail("Error writing to file %s", path);
    return 0;
}

int sbwthost_colors_read_wide(const char *path, int64_t *n_columns, int64_t *n_colors, int64_t *k, int64_t *words_per_row,
                              uint64_t *rows_or_null, int64_t words_cap) {
    if (!path) return fail("invalid argument");
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) return fail("Error opening file: %s", path);
    char magic[8];
    int64_t head[4];
    in.read(magic, 8);
    if (in.gcount() != 8) return fail("Error: colour file %s is truncated (no magic)", path);
    const bool wide = memcmp(magic, COLORS_MAGIC_WIDE, 8) == 0;
    if (!wide && memcmp(magic, COLORS_MAGIC, 8) != 0)
        return fail("Error: %s is not a colour file (unknown magic, SBWTCOL1 or SBWTCOL2 expected)", path);
    const int64_t head_bytes = wide ? 32 : 24;
    in.read(reinterpret_cast<char *>(head), head_bytes);
    if (in.gcount() != head_bytes) return fail("Error: colour file %s is truncated (header)", path);
    const int64_t max_colors = wide ? 4096 : 64;
    if (head[1] < 1 || head[1] > max_colors)
        return fail("Error: colour file %s: n_colors = %lld is outside 1 .. %lld", path, (long long)head[1], (long long)max_colors);
    const int64_t words = (head[1] + 63) / 64;
    if (wide && head[3] != words)
        return fail("Error: colour file %s: words_per_row = %lld, %lld colours need %lld", path, (long long)head[3], (long long)head[1],
                    (long long)words);
    if (head[0] < 0 || head[0] > ((int64_t)1 << 50)) return fail("Error: colour file %s: n_columns = %lld", path, (long long)head[0]);
    in.seekg(0, std::ios::end);
    const int64_t size = (int64_t)in.tellg(), start = 8 + head_bytes, want = start + head[0] * words * 8;
    if (size < want)
        return fail("Error: colour file %s is truncated (%lld bytes, %lld columns of %lld words need %lld)", path, (long long)size,
                    (long long)head[0], (long long)words, (long long)want);
    if (size > want) return fail("Error: colour file %s has %lld bytes after its %lld rows", path, (long long)(size - want), (long long)head[0]);
    if (n_columns) *n_columns = head[0];
    if (n_colors) *n_colors = head[1];
    if (k) *k = head[2];
    if (words_per_row) *words_per_row = words;
    if (!rows_or_null) return 0;
    if (words_cap < head[0] * words)
        return fail("Error: room for %lld words, the colour file holds %lld", (long long)words_cap, (long long)(head[0] * words));
    in.seekg(start, std::ios::beg);
    if (head[0] > 0) in.read(reinterpret_cast<char *>(rows_or_null), (std::streamsize)(head[0] * words * 8));
    if (!in.good()) return fail("Error reading %s", path);
    return 0;
}

// ---- colour-set files: "SBWTCOL3", int64 n_columns, n_colors, k, words_per_row, n_sets, then n_columns uint32 ids zero-padded
// to a multiple of 8 bytes, then n_sets x words_per_row words ----
static const char COLORS_MAGIC_SETS[8] = {'S', 'B', 'W', 'T', 'C', 'O', 'L', '3'};

// the invariants a file can be held to (include/sbwtgpu.h, "colour sets"): ids below n_sets; row 0 zero, no other row zero, no
// bit >= n_colors.  NULL when they hold, else the message in `msg`.
static const char *colorsets_violation(const uint32_t *ids, int64_t n_ids, int64_t first_col, const uint64_t *table, int64_t n_rows,
                                       int64_t first_row, int64_t n_sets, int64_t n_colors, int64_t words, char *msg, size_t cap) {
    for (int64_t j = 0; j < n_ids; j++)
        if ((int64_t)ids[j] >= n_sets) {
            snprintf(msg, cap, "the id %lld of column %lld is not below n_sets = %lld", (long long)ids[j], (long long)(first_col + j),
                     (long long)n_sets);
            return msg;
        }
    const uint64_t keep = (n_colors & 63) == 0 ? ~0ull : ((1ull << (n_colors & 63)) - 1ull);
    for (int64_t r = 0; r < n_rows; r++) {
        const uint64_t *row = table + r * words;
        uint64_t any = 0;
        for (int64_t w = 0; w < words; w++) any |= row[w];
        if (first_row + r == 0 && any) { snprintf(msg, cap, "row 0 of the table is not all zero"); return msg; }
        if (first_row + r != 0 && !any) {
            snprintf(msg, cap, "row %lld of the table is all zero (only row 0 may be)", (long long)(first_row + r));
            return msg;
        }
        if (row[words - 1] & ~keep) {
            snprintf(msg, cap, "row %lld of the table has a bit >= n_colors = %lld", (long long)(first_row + r), (long long)n_colors);
            return msg;
        }
    }
    return nullptr;
}

int sbwthost_colorsets_write(const char *path, const uint32_t *ids, const uint64_t *table, int64_t n_columns, int64_t n_colors,
                             int64_t k, int64_t n_sets) {
    if (!path || n_columns < 0 || (n_columns > 0 && !ids) || !table) return fail("invalid argument");
    if (n_colors < 1 || n_colors > 4096) return fail("Error: n_colors must be in 1 .. 4096, not %lld", (long long)n_colors);
    if (n_columns >= ((int64_t)1 << 31)) return fail("Error: colour sets hold fewer than 2^31 columns, not %lld", (long long)n_columns);
    if (n_sets < 1 || n_sets > 0xFFFFFFFFll) return fail("Error: n_sets must be in 1 .. 2^32 - 1, not %lld", (long long)n_sets);
    const int64_t words = (n_colors + 63) / 64;
    char msg[160];
    if (colorsets_violation(ids, n_columns, 0, table, n_sets, 0, n_sets, n_colors, words, msg, sizeof msg))
        return fail("Error: colour sets for %s: %s", path, msg);
    std::ofstream out(path, std::ios::binary);
    if (!out.good()) return fail("Error opening file: %s", path);
    const int64_t head[5] = {n_columns, n_colors, k, words, n_sets};
    const char pad[8] = {0};
    out.write(COLORS_MAGIC_SETS, 8);
    out.write(reinterpret_cast<const char *>(head), 40);
    if (n_columns > 0) out.write(reinterpret_cast<const char *>(ids), (std::streamsize)(n_columns * 4));
    if (n_columns & 1) out.write(pad, 4);
    out.write(reinterpret_cast<const char *>(table), (std::streamsize)(n_sets * words * 8));
    out.flush();
    if (!out.good()) return fail("Error writing to file %s", path);
    return 0;
}

int sbwthost_colorsets_read(const char *path, int64_t *n_columns, int64_t *n_colors, int64_t *k, int64_t *words_per_row, int64_t *n_sets,
                            uint32_t *ids_or_null, int64_t ids_cap, uint64_t *table_or_null, int64_t table_words_cap) {
    if (!path) return fail("invalid argument");
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) return fail("Error opening file: %s", path);
    char magic[8];
    int64_t head[5];
    in.read(magic, 8);
    if (in.gcount() != 8) return fail("Error: colour file %s is truncated (no magic)", path);
    if (memcmp(magic, COLORS_MAGIC_SETS, 8) != 0) return fail("Error: %s is not a colour-set file (wrong magic, SBWTCOL3 expected)", path);
    in.read(reinterpret_cast<char *>(head), 40);
    if (in.gcount() != 40) return fail("Error: colour file %s is truncated (header)", path);
    const int64_t n = head[0], nc = head[1], ns = head[4];
    if (nc < 1 || nc > 4096) return fail("Error: colour file %s: n_colors = %lld is outside 1 .. 4096", path, (long long)nc);
    const int64_t words = (nc + 63) / 64;
    if (head[3] != words)
        return fail("Error: colour file %s: words_per_row = %lld, %lld colours need %lld", path, (long long)head[3], (long long)nc,
                    (long long)words);
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail("Error: colour file %s: n_columns = %lld is outside 0 .. 2^31 - 1", path, (long long)n);
    if (ns < 1 || ns > 0xFFFFFFFFll) return fail("Error: colour file %s: n_sets = %lld is outside 1 .. 2^32 - 1", path, (long long)ns);
    in.seekg(0, std::ios::end);
    const int64_t size = (int64_t)in.tellg(), id_bytes = (n * 4 + 7) & ~(int64_t)7, want = 48 + id_bytes + ns * words * 8;
    if (size < want)
        return fail("Error: colour file %s is truncated (%lld bytes, %lld ids and %lld sets of %lld words need %lld)", path, (long long)size,
                    (long long)n, (long long)ns, (long long)words, (long long)want);
    if (size > want) return fail("Error: colour file %s has %lld bytes after its table", path, (long long)(size - want));
    if (ids_or_null && ids_cap < n) return fail("Error: room for %lld ids, the colour file holds %lld", (long long)ids_cap, (long long)n);
    if (table_or_null && table_words_cap < ns * words)
        return fail("Error: room for %lld words, the colour file's table holds %lld", (long long)table_words_cap, (long long)(ns * words));
    // ids and table go through a buffer piece by piece (or straight into the caller's arrays) and are checked on the way
    in.seekg(48, std::ios::beg);
    char msg[160];
    try {
        const int64_t PIECE = (int64_t)1 << 20;
        std::vector<uint32_t> ibuf(ids_or_null ? 0 : (size_t)std::min(n, PIECE));
        for (int64_t lo = 0; lo < n; lo += PIECE) {
            const int64_t m = std::min(PIECE, n - lo);
            uint32_t *dst = ids_or_null ? ids_or_null + lo : ibuf.data();
            in.read(reinterpret_cast<char *>(dst), (std::streamsize)(m * 4));
            if (!in.good()) return fail("Error reading %s", path);
            if (colorsets_violation(dst, m, lo, nullptr, 0, 0, ns, nc, words, msg, sizeof msg)) return fail("Error: colour file %s: %s", path, msg);
        }
        if (n & 1) {
            uint32_t pad = 0;
            in.read(reinterpret_cast<char *>(&pad), 4);
            if (!in.good()) return fail("Error reading %s", path);
            if (pad != 0) return fail("Error: colour file %s: the padding after the ids is not zero", path);
        }
        const int64_t ROWS = std::max<int64_t>(1, PIECE / words);
        std::vector<uint64_t> tbuf(table_or_null ? 0 : (size_t)(std::min(ns, ROWS) * words));
        for (int64_t lo = 0; lo < ns; lo += ROWS) {
            const int64_t m = std::min(ROWS, ns - lo);
            uint64_t *dst = table_or_null ? table_or_null + lo * words : tbuf.data();
            in.read(reinterpret_cast<char *>(dst), (std::streamsize)(m * words * 8));
            if (!in.good()) return fail("Error reading %s", path);
            if (colorsets_violation(nullptr, 0, 0, dst, m, lo, ns, nc, words, msg, sizeof msg)) return fail("Error: colour file %s: %s", path, msg);
        }
    } catch (const std::bad_alloc &) {
        return fail("out of memory");
    }
    if (n_columns) *n_columns = n;
    if (n_colors) *n_colors = nc;
    if (k) *k = head[2];
    if (words_per_row) *words_per_row = words;
    if (n_sets) *n_sets = ns;
    return 0;
}

// ---- position files: "SBWTPOS1" (positions_file.hh holds the format; SBWT::Positions::save / load go through the same code) ----
int sbwthost_positions_write(const char *path, const uint64_t *first, int64_t n_columns, int64_t k, const int32_t *seq_color,
                             const int64_t *seq_len, int64_t n_seqs) {
    if (!path || n_columns < 0 || n_seqs < 0 || (n_columns > 0 && !first) || (n_seqs > 0 && (!seq_color || !seq_len))) return fail("invalid argument");
    try {
        std::vector<sbwt::positions_file::Seq> seqs((size_t)n_seqs);
        for (int64_t i = 0; i < n_seqs; i++) seqs[(size_t)i] = {seq_color[i], 0, seq_len[i]};
        sbwt::positions_file::write(path, first, n_columns, k, seqs.data(), n_seqs);
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}

int sbwthost_positions_read(const char *path, int64_t *n_columns, int64_t *k, int64_t *n_seqs, int32_t *seq_color_or_null,
                            int64_t *seq_len_or_null, int64_t seqs_cap, uint64_t *first_or_null, int64_t first_cap) {
    if (!path) return fail("invalid argument");
    try {
        int64_t n = 0, kk = 0, ns = 0;
        std::vector<sbwt::positions_file::Seq> seqs;
        const bool want_seqs = seq_color_or_null || seq_len_or_null;
        sbwt::positions_file::read(path, n, kk, ns, want_seqs ? &seqs : nullptr, first_or_null, first_cap);
        if (want_seqs && seqs_cap < ns) return fail("Error: room for %lld sequences, the position file lists %lld", (long long)seqs_cap, (long long)ns);
        for (int64_t i = 0; want_seqs && i < ns; i++) {
            if (seq_color_or_null) seq_color_or_null[i] = seqs[(size_t)i].colour;
            if (seq_len_or_null) seq_len_or_null[i] = seqs[(size_t)i].length;
        }
        if (n_columns) *n_columns = n;
        if (k) *k = kk;
        if (n_seqs) *n_seqs = ns;
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}

// ---- occurrence files: "SBWTOCC1" (occurrences_file.hh holds the format; SBWT::Occurrences::save / load go through the same code) ----
int sbwthost_occurrences_write(const char *path, const uint64_t *off, const uint64_t *occ, int64_t n_columns, int64_t k, int64_t n_occ,
                               const int32_t *seq_color, const int64_t *seq_len, int64_t n_seqs) {
    if (!path || !off || n_columns < 0 || n_seqs < 0 || n_occ < 0 || (n_occ > 0 && !occ) || (n_seqs > 0 && (!seq_color || !seq_len)))
        return fail("invalid argument");
    try {
        std::vector<sbwt::occurrences_file::Seq> seqs((size_t)n_seqs);
        for (int64_t i = 0; i < n_seqs; i++) seqs[(size_t)i] = {seq_color[i], 0, seq_len[i]};
        sbwt::occurrences_file::write(path, off, occ, n_columns, k, n_occ, seqs.data(), n_seqs);
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}

int sbwthost_occurrences_read(const char *path, int64_t *n_columns, int64_t *k, int64_t *n_seqs, int64_t *n_occ, int32_t *seq_color_or_null,
                              int64_t *seq_len_or_null, int64_t seqs_cap, uint64_t *off_or_null, int64_t off_cap, uint64_t *occ_or_null,
                              int64_t occ_cap) {
    if (!path) return fail("invalid argument");
    try {
        int64_t n = 0, kk = 0, ns = 0, no = 0;
        std::vector<sbwt::occurrences_file::Seq> seqs;
        const bool want_seqs = seq_color_or_null || seq_len_or_null;
        sbwt::occurrences_file::read(path, n, kk, ns, no, (want_seqs || off_or_null) ? &seqs : nullptr, off_or_null, off_cap, occ_or_null, occ_cap);
        if (want_seqs && seqs_cap < ns) return fail("Error: room for %lld sequences, the occurrence file lists %lld", (long long)seqs_cap, (long long)ns);
        for (int64_t i = 0; want_seqs && i < ns; i++) {
            if (seq_color_or_null) seq_color_or_null[i] = seqs[(size_t)i].colour;
            if (seq_len_or_null) seq_len_or_null[i] = seqs[(size_t)i].length;
        }
        if (n_columns) *n_columns = n;
        if (k) *k = kk;
        if (n_seqs) *n_seqs = ns;
        if (n_occ) *n_occ = no;
        return 0;
    } catch (const std::exception &e) {
        return fail("%s", e.what());
    }
}

}  // extern "C"
