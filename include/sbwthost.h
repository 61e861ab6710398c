/*
 * sbwthost.h -- C ABI of the GPU-free host helpers (libsbwthost.so): in-memory construction of the
 * plain-matrix SBWT columns and the reference's index file format.  These sit either side of the
 * hot path; tests and bench.py use them to make and move indexes.
 */
#ifndef SBWTHOST_H
#define SBWTHOST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbwthost_bits sbwthost_bits;     /* A/C/G/T(+ssup) bit vectors of one index */
typedef struct sbwthost_file sbwthost_file;     /* a parsed index file */

const char *sbwthost_last_error(void);

/* Sort-based in-memory builder (same columns as NodeBOSSInMemoryConstructor.hh:98-213 / the KMC
 * constructor of the reference).  seqs[i] has seq_lens[i] bytes; k-mers containing anything but
 * upper-case ACGT are skipped.  2 <= k <= 255. */
int  sbwthost_build(const char *const *seqs, const int64_t *seq_lens, int64_t n_seqs, int64_t k,
                    int add_revcomp, int build_streaming_support, int n_threads, sbwthost_bits **out);
void sbwthost_bits_free(sbwthost_bits *b);
int  sbwthost_bits_info(const sbwthost_bits *b, int64_t *n_nodes, int64_t *n_kmers, int64_t *k, int *has_ssup);
/* which: 0..3 = A,C,G,T, 4 = suffix_group_starts (NULL if absent); ceil(n_nodes/64) words */
const uint64_t *sbwthost_bits_words(const sbwthost_bits *b, int which);

/* Index files in the reference format: serialize_string("plain-matrix") (sbwt_build.cpp:142)
 * followed by SBWT::serialize (SBWT.hh:462-491). */
int  sbwthost_file_write(const char *path, int64_t n_nodes, const uint64_t *A, const uint64_t *C,
                         const uint64_t *G, const uint64_t *T, const uint64_t *ssup /* nullable */,
                         const int64_t C_array[4], const int64_t *precalc_pairs, int64_t precalc_k,
                         int64_t n_kmers, int64_t k);
int  sbwthost_file_read(const char *path, sbwthost_file **out);
void sbwthost_file_free(sbwthost_file *f);
int  sbwthost_file_info(const sbwthost_file *f, int64_t *n_nodes, int64_t *n_kmers, int64_t *k,
                        int64_t *precalc_k, int64_t C_array[4], int *has_ssup);
const uint64_t *sbwthost_file_words(const sbwthost_file *f, int which);
const int64_t  *sbwthost_file_precalc(const sbwthost_file *f);

/* FASTA/FASTQ(.gz) reader (SeqIO stand-in): concatenates all reads of `path`.
 * *bases / *read_off are malloc'ed; free with sbwthost_free. */
int  sbwthost_read_sequences(const char *path, char **bases, int64_t **read_off, int64_t *n_reads);
void sbwthost_free(void *p);
/* The same reads by the CLI's reader for plain regular files: the file cut at record starts about chunk_bytes apart,
 * the pieces parsed by n_threads threads and put together in file order (seqio.hh read_file_chunked).  Returns 1 (and
 * reads nothing) when the file is not one that can be cut: gzip data, a pipe, an unknown extension. */
int  sbwthost_read_sequences_chunked(const char *path, int64_t chunk_bytes, int n_threads, char **bases, int64_t **read_off,
                                     int64_t *n_reads);
/* Writes n bytes through the CLI's buffered writer; gzip_output != 0 compresses 1 MiB blocks on n_threads
 * threads (0 = automatic) into a multi-member gzip file (-z of `sbwt search`, sbwt_search.cpp:120). */
int  sbwthost_write_file(const char *path, const char *data, int64_t n, int gzip_output, int n_threads);

/* The host rank directory of the scalar API (host/bitvector.hh: rank_support_v5_blob, the directory an index file carries
 * beside every bit vector): out[i] = number of set bits in bits[0, pos[i]) for n positions, pos[i] in [0, n_bits].
 * (SubsetMatrixRank::rank of ONE position through the C++ mirror answers from this structure; batches of the search
 * path go to the GPU -- this entry point exists so that the directory's arithmetic is tested where there is no GPU.) */
int  sbwthost_rank_batch(const uint64_t *bits, int64_t n_bits, const int64_t *pos, int64_t n, int64_t *out);

/* Colour files (the colour matrix of include/sbwtgpu.h beside its index file): 8 bytes "SBWTCOL1"; int64 n_columns, n_colors,
 * k; then n_columns little-endian uint64 rows.  The read is a two-call pattern: rows_or_null = NULL gives the three sizes,
 * a second call with room for rows_cap >= n_columns rows fills them.  A truncated file, a wrong magic and n_colors outside
 * 1 .. 64 are errors with a message. */
int  sbwthost_colors_write(const char *path, const uint64_t *rows, int64_t n_columns, int64_t n_colors, int64_t k);
int  sbwthost_colors_read(const char *path, int64_t *n_columns, int64_t *n_colors, int64_t *k, uint64_t *rows_or_null,
                          int64_t rows_cap);
/* Wide colour files (more than 64 colours): 8 bytes "SBWTCOL2"; int64 n_columns, n_colors, k, words_per_row; then
 * n_columns x words_per_row little-endian uint64 words, row-major (word w of column j at j * words_per_row + w).
 * 1 <= n_colors <= 4096 and words_per_row = ceil(n_colors / 64).  The read is the same two-call pattern (words_cap counts
 * words: room for n_columns x words_per_row) and also reads an "SBWTCOL1" file, as words_per_row = 1.  A truncated file, an
 * unknown magic, n_colors outside 1 .. 4096 and another words_per_row are errors with a message.  sbwthost_colors_read
 * refuses "SBWTCOL2" files. */
int  sbwthost_colors_write_wide(const char *path, const uint64_t *rows, int64_t n_columns, int64_t n_colors, int64_t k);
int  sbwthost_colors_read_wide(const char *path, int64_t *n_columns, int64_t *n_colors, int64_t *k, int64_t *words_per_row,
                               uint64_t *rows_or_null, int64_t words_cap);
/* Colour-set files (the colour-set object of include/sbwtgpu.h: one id per column and a table of the distinct rows): 8 bytes
 * "SBWTCOL3"; int64 n_columns, n_colors, k, words_per_row, n_sets; then n_columns little-endian uint32 ids, zero-padded to a
 * multiple of 8 bytes; then n_sets x words_per_row little-endian uint64 words, row-major.  The read is the two-call pattern:
 * with ids_or_null = table_or_null = NULL it gives the five sizes, a second call with room for ids_cap >= n_columns ids and
 * table_words_cap >= n_sets x words_per_row words fills them.  Both calls check the header's ranges (1 <= n_colors <= 4096,
 * words_per_row = ceil(n_colors / 64), n_columns < 2^31, 1 <= n_sets < 2^32), the exact file size and every invariant of the
 * object but the ids of dummy columns, which only the index knows: ids below n_sets, row 0 of the table zero, no other row
 * zero, no bit >= n_colors.  Truncation, a wrong magic and any violation are errors with a message; the writer refuses the
 * same violations.  sbwthost_colors_read and sbwthost_colors_read_wide refuse "SBWTCOL3" files as they refuse any unknown
 * magic. */
int  sbwthost_colorsets_write(const char *path, const uint32_t *ids, const uint64_t *table, int64_t n_columns, int64_t n_colors,
                              int64_t k, int64_t n_sets);
int  sbwthost_colorsets_read(const char *path, int64_t *n_columns, int64_t *n_colors, int64_t *k, int64_t *words_per_row,
                             int64_t *n_sets, uint32_t *ids_or_null, int64_t ids_cap, uint64_t *table_or_null, int64_t table_words_cap);
/* Position files (the position table of include/sbwtgpu.h, "positions", beside its index file): 8 bytes "SBWTPOS1"; int64
 * n_columns, k, n_seqs; per sequence int32 colour (the line of the reference list its file stood on), int32 0, int64 length;
 * then n_columns little-endian uint64 of first (UINT64_MAX: no position, else (seq << 32) | (pos << 1) | t).  The read is
 * the two-call pattern: with the three pointers NULL it gives the sizes, a second call with room for seqs_cap >= n_seqs
 * entries and first_cap >= n_columns entries fills them.  Both calls check the header's ranges (n_columns < 2^31, n_seqs
 * <= 2^30) and the exact file size, the filling call also that every position lies on a listed sequence.  Truncation, a
 * wrong magic and any violation are errors with a message; the writer refuses the same violations. */
int  sbwthost_positions_write(const char *path, const uint64_t *first, int64_t n_columns, int64_t k, const int32_t *seq_color,
                              const int64_t *seq_len, int64_t n_seqs);
int  sbwthost_positions_read(const char *path, int64_t *n_columns, int64_t *k, int64_t *n_seqs, int32_t *seq_color_or_null,
                             int64_t *seq_len_or_null, int64_t seqs_cap, uint64_t *first_or_null, int64_t first_cap);
/* Occurrence files (the occurrence table of include/sbwtgpu.h, "occurrences", beside its index file): 8 bytes "SBWTOCC1"; int64
 * n_columns, k, n_seqs, n_occ; per sequence int32 colour, int32 0, int64 length, as in "SBWTPOS1"; then n_columns + 1
 * little-endian uint64 of off; then n_occ uint64 of occ.  The read is the two-call pattern: with the pointers NULL it gives the
 * sizes, a second call with room for seqs_cap >= n_seqs, off_cap >= n_columns + 1 and occ_cap >= n_occ entries fills them.
 * Both calls check the header's ranges and the exact file size (truncation, trailing bytes, another magic); the filling call
 * also refuses non-monotone offsets, unsorted keys within a column, a key on an unlisted sequence and a key whose pos + k lies
 * beyond its sequence's length, each with a message that names the cause.  The writer refuses the same violations. */
int  sbwthost_occurrences_write(const char *path, const uint64_t *off, const uint64_t *occ, int64_t n_columns, int64_t k, int64_t n_occ,
                                const int32_t *seq_color, const int64_t *seq_len, int64_t n_seqs);
int  sbwthost_occurrences_read(const char *path, int64_t *n_columns, int64_t *k, int64_t *n_seqs, int64_t *n_occ,
                               int32_t *seq_color_or_null, int64_t *seq_len_or_null, int64_t seqs_cap, uint64_t *off_or_null,
                               int64_t off_cap, uint64_t *occ_or_null, int64_t occ_cap);

#ifdef __cplusplus
}
#endif
#endif
