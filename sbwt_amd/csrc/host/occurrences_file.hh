// occurrences_file.hh -- the occurrence file beside an index file (include/sbwtgpu.h, "occurrences"):
//   8 bytes "SBWTOCC1"; int64 n_columns, k, n_seqs, n_occ; per sequence int32 colour, int32 0, int64 length (as in "SBWTPOS1");
//   then n_columns + 1 little-endian uint64 of off (off[0] = 0, non-decreasing, off[n_columns] = n_occ); then n_occ uint64 of
//   occ, (seq << 32) | (pos << 1) | t with seq < n_seqs and pos + k within the sequence, strictly ascending within a column.
// Plain C++: what SBWT::Occurrences::save / load and the host library's sbwthost_occurrences_* share.  Errors are exceptions.
#pragma once

#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "positions_file.hh"

namespace sbwt {
namespace occurrences_file {

static const char MAGIC[8] = {'S', 'B', 'W', 'T', 'O', 'C', 'C', '1'};
using Seq = positions_file::Seq;

// what both directions ask of the arrays; `what` begins the message
inline void check(const std::string &what, const uint64_t *off, const uint64_t *occ, int64_t n_columns, int64_t k, int64_t n_occ,
                  const Seq *seqs, int64_t n_seqs) {
    if (off[0] != 0) throw std::runtime_error(what + ": off[0] is not 0");
    for (int64_t j = 0; j < n_columns; j++)
        if (off[j] > off[j + 1]) throw std::runtime_error(what + ": the offsets are not monotone at column " + std::to_string(j));
    if (off[n_columns] != (uint64_t)n_occ)
        throw std::runtime_error(what + ": off[n_columns] = " + std::to_string(off[n_columns]) + " is not n_occ = " + std::to_string(n_occ));
    for (int64_t j = 0; j < n_columns; j++)
        for (uint64_t e = off[j]; e < off[j + 1]; e++) {
            const uint64_t f = occ[e];
            if (e > off[j] && occ[e - 1] >= f) throw std::runtime_error(what + ": the keys of column " + std::to_string(j) + " are not sorted (strictly ascending)");
            const int64_t seq = (int64_t)(f >> 32), pos = (int64_t)((f & 0xFFFFFFFFull) >> 1);
            if (seq >= n_seqs)
                throw std::runtime_error(what + ": column " + std::to_string(j) + " lies on sequence " + std::to_string(seq) + ", " +
                                         std::to_string(n_seqs) + " sequences are listed");
            if (pos + k > seqs[seq].length)
                throw std::runtime_error(what + ": column " + std::to_string(j) + " lies at offset " + std::to_string(pos) + " of sequence " +
                                         std::to_string(seq) + ", beyond its length " + std::to_string(seqs[seq].length));
        }
}

inline void write(const std::string &path, const uint64_t *off, const uint64_t *occ, int64_t n_columns, int64_t k, int64_t n_occ,
                  const Seq *seqs, int64_t n_seqs) {
    if (n_columns < 0 || n_seqs < 0 || n_occ < 0 || !off || (n_occ > 0 && !occ) || (n_seqs > 0 && !seqs)) throw std::runtime_error("invalid argument");
    if (n_seqs > ((int64_t)1 << 30)) throw std::runtime_error("Error: an occurrence file numbers at most 2^30 sequences, not " + std::to_string(n_seqs));
    check("Error: occurrences for " + path, off, occ, n_columns, k, n_occ, seqs, n_seqs);
    std::ofstream out(path, std::ios::binary);
    if (!out.good()) throw std::runtime_error("Error opening file: " + path);
    const int64_t head[4] = {n_columns, k, n_seqs, n_occ};
    out.write(MAGIC, 8);
    out.write(reinterpret_cast<const char *>(head), 32);
    for (int64_t i = 0; i < n_seqs; i++) {
        const Seq s = {seqs[i].colour, 0, seqs[i].length};
        out.write(reinterpret_cast<const char *>(&s), 16);
    }
    out.write(reinterpret_cast<const char *>(off), (std::streamsize)((n_columns + 1) * 8));
    if (n_occ > 0) out.write(reinterpret_cast<const char *>(occ), (std::streamsize)(n_occ * 8));
    out.flush();
    if (!out.good()) throw std::runtime_error("Error writing to file " + path);
}

// The header, and with off / occ given the body: seqs gets n_seqs entries, off (room for off_cap entries) n_columns + 1, occ
// (room for occ_cap) n_occ.  The body is read and checked only when off is given.
inline void read(const std::string &path, int64_t &n_columns, int64_t &k, int64_t &n_seqs, int64_t &n_occ, std::vector<Seq> *seqs,
                 uint64_t *off, int64_t off_cap, uint64_t *occ, int64_t occ_cap) {
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) throw std::runtime_error("Error opening file: " + path);
    char magic[8];
    int64_t head[4];
    in.read(magic, 8);
    if (in.gcount() != 8) throw std::runtime_error("Error: occurrence file " + path + " is truncated (no magic)");
    if (memcmp(magic, MAGIC, 8) != 0) throw std::runtime_error("Error: " + path + " is not an occurrence file (wrong magic, SBWTOCC1 expected)");
    in.read(reinterpret_cast<char *>(head), 32);
    if (in.gcount() != 32) throw std::runtime_error("Error: occurrence file " + path + " is truncated (header)");
    if (head[0] < 0 || head[0] >= ((int64_t)1 << 31))
        throw std::runtime_error("Error: occurrence file " + path + ": n_columns = " + std::to_string(head[0]) + " is outside 0 .. 2^31 - 1");
    if (head[2] < 0 || head[2] > ((int64_t)1 << 30))
        throw std::runtime_error("Error: occurrence file " + path + ": n_seqs = " + std::to_string(head[2]) + " is outside 0 .. 2^30");
    if (head[3] < 0 || head[3] > ((int64_t)1 << 56))
        throw std::runtime_error("Error: occurrence file " + path + ": n_occ = " + std::to_string(head[3]) + " is out of range");
    in.seekg(0, std::ios::end);
    const int64_t size = (int64_t)in.tellg(), want = 40 + head[2] * 16 + (head[0] + 1) * 8 + head[3] * 8;
    if (size < want)
        throw std::runtime_error("Error: occurrence file " + path + " is truncated (" + std::to_string(size) + " bytes, " + std::to_string(head[2]) +
                                 " sequences, " + std::to_string(head[0]) + " columns and " + std::to_string(head[3]) + " occurrences need " +
                                 std::to_string(want) + ")");
    if (size > want) throw std::runtime_error("Error: occurrence file " + path + " has " + std::to_string(size - want) + " bytes after its table");
    n_columns = head[0];
    k = head[1];
    n_seqs = head[2];
    n_occ = head[3];
    std::vector<Seq> own;
    if (!seqs && off) seqs = &own;
    in.seekg(40, std::ios::beg);
    if (seqs) {
        seqs->resize((size_t)n_seqs);
        if (n_seqs > 0) in.read(reinterpret_cast<char *>(seqs->data()), (std::streamsize)(n_seqs * 16));
        if (!in.good()) throw std::runtime_error("Error reading " + path);
        for (const Seq &s : *seqs)
            if (s.zero != 0 || s.length < 0 || s.colour < 0) throw std::runtime_error("Error: occurrence file " + path + ": a sequence entry is damaged");
    }
    if (off) {
        if (off_cap < n_columns + 1 || occ_cap < n_occ || (n_occ > 0 && !occ))
            throw std::runtime_error("Error: room for " + std::to_string(off_cap) + " offsets and " + std::to_string(occ_cap) +
                                     " keys, the occurrence file holds " + std::to_string(n_columns + 1) + " and " + std::to_string(n_occ));
        in.seekg(40 + n_seqs * 16, std::ios::beg);
        in.read(reinterpret_cast<char *>(off), (std::streamsize)((n_columns + 1) * 8));
        if (n_occ > 0) in.read(reinterpret_cast<char *>(occ), (std::streamsize)(n_occ * 8));
        if (!in.good()) throw std::runtime_error("Error reading " + path);
        check("Error: occurrence file " + path, off, occ, n_columns, k, n_occ, seqs->data(), n_seqs);
    }
}

}  // namespace occurrences_file
}  // namespace sbwt
