// positions_file.hh -- the position file beside an index file (include/sbwtgpu.h, "positions"):
//   8 bytes "SBWTPOS1"; int64 n_columns, k, n_seqs; per sequence int32 colour, int32 0, int64 length; then n_columns
//   little-endian uint64 of first (UINT64_MAX: no position, else (seq << 32) | (pos << 1) | t with seq < n_seqs).
// Plain C++: what SBWT::Positions::save / load and the host library's sbwthost_positions_* share.  Errors are exceptions.
#pragma once

#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace sbwt {
namespace positions_file {

static const char MAGIC[8] = {'S', 'B', 'W', 'T', 'P', 'O', 'S', '1'};

struct Seq {
    int32_t colour;     // the line of the reference list its file stood on
    int32_t zero;
    int64_t length;     // bases
};
static_assert(sizeof(Seq) == 16, "a sequence entry of the position file is 16 bytes");

inline void write(const std::string &path, const uint64_t *first, int64_t n_columns, int64_t k, const Seq *seqs, int64_t n_seqs) {
    if (n_columns < 0 || n_seqs < 0 || (n_columns > 0 && !first) || (n_seqs > 0 && !seqs)) throw std::runtime_error("invalid argument");
    if (n_seqs > ((int64_t)1 << 30)) throw std::runtime_error("Error: a position file numbers at most 2^30 sequences, not " + std::to_string(n_seqs));
    for (int64_t j = 0; j < n_columns; j++)
        if (first[j] != ~0ull && (int64_t)(first[j] >> 32) >= n_seqs)
            throw std::runtime_error("Error: positions for " + path + ": column " + std::to_string(j) + " lies on sequence " +
                                     std::to_string(first[j] >> 32) + ", " + std::to_string(n_seqs) + " sequences are listed");
    std::ofstream out(path, std::ios::binary);
    if (!out.good()) throw std::runtime_error("Error opening file: " + path);
    const int64_t head[3] = {n_columns, k, n_seqs};
    out.write(MAGIC, 8);
    out.write(reinterpret_cast<const char *>(head), 24);
    for (int64_t i = 0; i < n_seqs; i++) {
        const Seq s = {seqs[i].colour, 0, seqs[i].length};
        out.write(reinterpret_cast<const char *>(&s), 16);
    }
    if (n_columns > 0) out.write(reinterpret_cast<const char *>(first), (std::streamsize)(n_columns * 8));
    out.flush();
    if (!out.good()) throw std::runtime_error("Error writing to file " + path);
}

// The header, and with seqs / first given the body: seqs gets n_seqs entries, first (room for first_cap entries) n_columns.
inline void read(const std::string &path, int64_t &n_columns, int64_t &k, int64_t &n_seqs, std::vector<Seq> *seqs, uint64_t *first,
                 int64_t first_cap) {
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) throw std::runtime_error("Error opening file: " + path);
    char magic[8];
    int64_t head[3];
    in.read(magic, 8);
    if (in.gcount() != 8) throw std::runtime_error("Error: position file " + path + " is truncated (no magic)");
    if (memcmp(magic, MAGIC, 8) != 0) throw std::runtime_error("Error: " + path + " is not a position file (wrong magic, SBWTPOS1 expected)");
    in.read(reinterpret_cast<char *>(head), 24);
    if (in.gcount() != 24) throw std::runtime_error("Error: position file " + path + " is truncated (header)");
    if (head[0] < 0 || head[0] >= ((int64_t)1 << 31))
        throw std::runtime_error("Error: position file " + path + ": n_columns = " + std::to_string(head[0]) + " is outside 0 .. 2^31 - 1");
    if (head[2] < 0 || head[2] > ((int64_t)1 << 30))
        throw std::runtime_error("Error: position file " + path + ": n_seqs = " + std::to_string(head[2]) + " is outside 0 .. 2^30");
    in.seekg(0, std::ios::end);
    const int64_t size = (int64_t)in.tellg(), want = 32 + head[2] * 16 + head[0] * 8;
    if (size < want)
        throw std::runtime_error("Error: position file " + path + " is truncated (" + std::to_string(size) + " bytes, " +
                                 std::to_string(head[2]) + " sequences and " + std::to_string(head[0]) + " columns need " + std::to_string(want) + ")");
    if (size > want) throw std::runtime_error("Error: position file " + path + " has " + std::to_string(size - want) + " bytes after its table");
    n_columns = head[0];
    k = head[1];
    n_seqs = head[2];
    in.seekg(32, std::ios::beg);
    if (seqs) {
        seqs->resize((size_t)n_seqs);
        if (n_seqs > 0) in.read(reinterpret_cast<char *>(seqs->data()), (std::streamsize)(n_seqs * 16));
        if (!in.good()) throw std::runtime_error("Error reading " + path);
        for (const Seq &s : *seqs)
            if (s.zero != 0 || s.length < 0 || s.colour < 0) throw std::runtime_error("Error: position file " + path + ": a sequence entry is damaged");
    }
    if (first) {
        if (first_cap < n_columns)
            throw std::runtime_error("Error: room for " + std::to_string(first_cap) + " entries, the position file holds " + std::to_string(n_columns));
        in.seekg(32 + n_seqs * 16, std::ios::beg);
        if (n_columns > 0) in.read(reinterpret_cast<char *>(first), (std::streamsize)(n_columns * 8));
        if (!in.good()) throw std::runtime_error("Error reading " + path);
        for (int64_t j = 0; j < n_columns; j++)
            if (first[j] != ~0ull && (int64_t)(first[j] >> 32) >= n_seqs)
                throw std::runtime_error("Error: position file " + path + ": column " + std::to_string(j) + " lies on sequence " +
                                         std::to_string(first[j] >> 32) + ", the file lists " + std::to_string(n_seqs));
    }
}

}  // namespace positions_file
}  // namespace sbwt
