/*
 * sbwtgpu.h -- C ABI of the MI355X (gfx950) k-mer search path for plain-matrix SBWT indexes.
 *
 * This is the drop-in boundary: the functions below are what a binding in the reference
 * (algbio/SBWT, C++17) would call instead of running its CPU loop.  Each entry point cites
 * the reference interface it replaces (paths relative to the reference repository root).
 * INTEGRATION.md shows the reference-side glue.
 *
 * Conventions
 *   - plain C, no C++/torch types; all sizes/ranks are int64_t like the reference's API.
 *   - return value: 0 = ok, negative = error (codes below); sbwtgpu_last_error() gives the
 *     message (thread-local).  Nothing throws or aborts across this boundary.
 *   - ownership: handles are owned by the library (destroy them); every buffer is owned by
 *     the caller and only borrowed for the duration of the call (index_create copies).
 *   - threading: a handle is immutable after creation; concurrent query calls on one handle
 *     are allowed (host-buffer calls use a private stream each).
 *   - "host" entry points take host pointers and do H2D/D2H themselves; "_dev" entry points
 *     take device pointers on the index's device plus a hipStream_t (as void*), enqueue
 *     asynchronously and never synchronise.
 *   - bit vectors are arrays of little-endian uint64_t words, bit i of the vector is bit
 *     (i % 64) of word i / 64 -- the sdsl::bit_vector convention used by the reference.
 */
#ifndef SBWTGPU_H
#define SBWTGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBWTGPU_OK                      0
#define SBWTGPU_ERR_INVALID_ARG        -1
#define SBWTGPU_ERR_NO_DEVICE          -2   /* no usable HIP device / wrong device index */
#define SBWTGPU_ERR_HIP                -3   /* a HIP runtime call failed */
#define SBWTGPU_ERR_NO_STREAMING       -4   /* "Error: streaming search support not built" (SBWT.hh:546-547) */
#define SBWTGPU_ERR_PRECALC_TOO_LONG   -5   /* precalc > 20 (SBWT.hh:619-621) */
#define SBWTGPU_ERR_PRECALC_GT_K       -6   /* precalc > k  (SBWT.hh:623-624) */
#define SBWTGPU_ERR_NOT_SINGLETON      -7   /* "Bug: k-mer search did not give a singleton interval" (SBWT.hh:410-413) */
#define SBWTGPU_ERR_OOM                -8
#define SBWTGPU_ERR_READ_TOO_LONG      -9   /* a single read of >= 2^31 bases */
#define SBWTGPU_ERR_STALLED           -10   /* the sorted fused search kernel stopped making progress (a bug: the call
                                               failed instead of hanging the device) */

typedef struct sbwtgpu_index sbwtgpu_index;

/* What sbwt::SBWT<SubsetMatrixRank<sdsl::bit_vector, sdsl::rank_support_v5<>>> holds
 * (include/sbwt/SBWT.hh:36-45, include/sbwt/SubsetMatrixRank.hh:19-23).  Rank supports
 * are not passed: the library builds its own device-side directory from the bits. */
typedef struct {
    int64_t         n_nodes;      /* number of columns (SBWT.hh:43); > 0 (the root always exists) */
    const uint64_t *A_bits;       /* ceil(n_nodes/64) words each */
    const uint64_t *C_bits;
    const uint64_t *G_bits;
    const uint64_t *T_bits;
    const uint64_t *suffix_group_starts; /* NULL => no streaming support (SBWT.hh:253) */
    int64_t         k;            /* SBWT.hh:45 */
    int64_t         n_kmers;      /* SBWT.hh:44 (informational) */
    int64_t         precalc_k;    /* SBWT.hh:41; 0 => no precalc table */
    const int64_t  *precalc;      /* 4^precalc_k (first,second) pairs as loaded from an index
                                     file (SBWT.hh:40,510), or NULL => computed on the device
                                     (do_kmer_prefix_precalc, SBWT.hh:616-645) */
} sbwtgpu_index_desc;

typedef struct {
    int64_t n_nodes, n_kmers, k, precalc_k;
    int64_t C[4];                 /* SBWT.hh:344-349 */
    int32_t has_streaming_support;
    int32_t device;
    int64_t device_precalc_k;     /* depth of the library's own device-side prefix table (>= precalc_k) */
    int64_t blob_bytes;           /* size of the device image (what index_bcast moves) */
    int64_t image_level;          /* what the image holds: 0 = all derived structures, 1 = no path order / transition
                                     table, 2 = blocks + dense prefix table only (see "image_level" below) */
    int64_t n_paths;              /* path order: number of paths (0 without one) */
    int64_t n_branch;             /* columns with two or more successors */
    int64_t default_search_variant; /* the kernel "search_variant" = -1 picks for this index (see below) */
} sbwtgpu_index_info;

/* ---- library ---- */
const char *sbwtgpu_version(void);
const char *sbwtgpu_last_error(void);
int         sbwtgpu_device_count(int *count);
/* Process-wide tuning knobs for experiments (results never depend on them):
 *   "search_variant"  -1 (default) = by the index: 5 on an index with a path order, else the blocks kernel.  5 = the fused route
 *                     (k_search_fused re-encodes the bases itself and takes batches of reads of up to 160 bases; the
 *                     general kernel runs behind it for what it hands on or declines); 4 = always two passes (encode +
 *                     k_search_cert along the path order, per-read segment lists written by the whole wave); 1 =
 *                     k_search_cert on the blocks only; 0 = k_search (the reference's order of searches; cross-checks)
 *   "fused_ragged"    1 (default): the fused route also takes batches of reads of different lengths (it fetches their
 *                     offsets); 0: only batches of reads of one length (SBWTGPU_FUSED_RAGGED)
 *   "fused_pieces"    1 .. 3: the fused route takes a read of more than 160 bases as up to this many pieces of 160 bases
 *                     that overlap by k-1 (tickets are (read, piece)); 1: such reads go to the general kernel.  -1 / 0
 *                     (default) = 3 (k = 63, 250-base reads: 115 -> 243 G k-mers/s; k = 30: 228 -> 235 G since round 5).
 *                     SBWTGPU_FUSED_PIECES.
 *   "split_long"      1 (default): the device entry points cut reads of more than two pieces' worth of k-mers (a piece:
 *                     128 .. 1024 k-mers by batch size) into pieces that lanes take separately, at k-mers whose result
 *                     does not depend on history; 0: one lane per read whatever its length (SBWTGPU_SPLIT_LONG)
 *   "kernel_events"   1: HIP events around the dominant kernel of every search call (sbwtgpu_kernel_times)
 *   "sort_reads"      1: the path-order kernels take the reads sorted by where they start in the path order (a lookup of one
 *                     k-mer per read + a radix sort of (position, read) pairs before the search; lanes of a wave then
 *                     share lines of the index); default 0: the pre-pass costs more than it saves while the path order
 *                     numbers its paths in column order.  Reads that ARRIVE sorted by genome
 *                     position need no switch and run 18 % faster.  Set it before sizing workspaces.  SBWTGPU_SORT_READS.
 *   "probe_len"       length of the certificate probes (-1 = automatic, 0 = off)
 *   "derive_ssup"     1 (default): indexes created without suffix_group_starts get the marks derived on
 *                     the device so that the per-k-mer search loop can use streaming steps internally
 *   "debug"           kernel experiment bits (0 = product behaviour); fused kernel: 32 = no anchors / seeds / resumed compares,
 *                     64 = the k > 31 walk (F_CMP) for every k
 *   "poison_results"  1: every search first fills its result range with 0xA5, every matching-statistics call its len range
 *                        with 0xFF and its interval range with 0xA5, every read-hits call its records with 0xA5 (parity tests)
 *   "read_hits_wave_min"    per-read hit profiles: reads of this many windows or more are reduced by a whole wave, shorter
 *                        ones by one lane each (default 1024; < 1 restores the default)
 *   "read_hits_chunk_bases" sbwtgpu_read_hits_batch cuts its batch into chunks of whole reads of at most this many bases (a
 *                        chunk always takes one read); 0 (default) = 64 Mi
 *   "read_hits_wide"     1: the read-hits calls take the int64 search route also on indexes of fewer than 2^31 columns (tests)
 *   "walks_chunk_bases"  sbwtgpu_unitigs_walks_batch cuts its batch into chunks of whole reads of at most this many bases (a chunk
 *                        always takes one read); 0 (default) = 64 Mi
 *   "pseudoalign_chunk_bases" sbwtgpu_pseudoalign_batch (_wide_batch, _sets_batch) and sbwtgpu_colors_add_batch cut their batch
 *                        into chunks of whole reads of at most this many bases (a chunk always takes one read); 0 (default) = 64 Mi
 *   "screen_chunk_bases" sbwtgpu_screen_add_batch cuts its batch into chunks of whole reads of at most this many bases (a chunk
 *                        always takes one read); 0 (default) = 64 Mi
 *   "genotype_chunk_bases" sbwtgpu_genotype_add_batch cuts its batch into chunks of whole reads of at most this many bases (a
 *                        chunk always takes one read); 0 (default) = 64 Mi
 *   "positions_chunk_bases" sbwtgpu_positions_add_batch and sbwtgpu_positions_map_batch cut their batch into chunks of whole
 *                        sequences of at most this many bases (a chunk always takes one sequence); 0 (default) = 64 Mi
 *   "positions_map_table" the distinct placements per read that the map kernel keeps in LDS before the read goes to the exact
 *                        second kernel: 1 .. SBWTGPU_POSITIONS_MAP_TABLE, 0 (default) = that compiled capacity; another value
 *                        is refused.  No result depends on it (tests reach the second kernel with it)
 *   "occurrences_chunk_bases" sbwtgpu_occurrences_builder_add_batch and sbwtgpu_occurrences_map_batch cut their batch into chunks
 *                        of whole sequences of at most this many bases (a chunk always takes one sequence); 0 (default) = 64 Mi
 *   "occurrences_map_table" the distinct placements per read that the occurrence map kernel keeps in LDS before the read goes to
 *                        the exact second kernel: 1 .. SBWTGPU_OCCURRENCES_MAP_TABLE, 0 (default) = that compiled capacity;
 *                        another value is refused.  No result depends on it (tests reach the second kernel with it)
 *   "verify_fast_bases"  the longest read, in bases, that the first verify kernel takes (its rows in registers) before the read
 *                        goes to the second kernel (rows in LDS): 1 .. 256, 0 (default) = 256; another value is refused.  No
 *                        result depends on it (tests reach the second kernel with short reads)
 *   "align_fast_edit"    the largest edit that the first align kernel takes (a band of 2 edit + 1 diagonals, one mask word per
 *                        row) before the read goes to the second kernel (the whole window, one wave per read): 1 .. 31, 0
 *                        (default) = 31; another value is refused.  No result depends on it
 *   "trans_ext", "trans_wide"   accepted and ignored (round-2 table formats)
 * Read when an index is CREATED (derived acceleration structures inside the device image; environment
 * variables of the same meaning: SBWTGPU_SPARSE_PRECALC, SBWTGPU_PROBE_FILTER, SBWTGPU_PATH_ORDER):
 *   "sparse_depth"    depth of the sparse (hashed) prefix table, 0 = none, default 31 (capped at k)
 *   "probe_filter"    1 (default): Bloom filter over the probe_len-mers of the index for the certificate probes
 *   "path_order"      1 (default): path order + transition table (indexes with suffix-group marks, given or derived)
 *   "big_path"        1 (default): an index of 2^31 .. 2^32 - 2^24 columns with k <= 31 gets the full image too -- columns and
 *                     path positions as 32-bit unsigned values, read by the fused kernel's BIG instantiation (2.25 x 10^9
 *                     columns: 120 GB, 207 G k-mers/s); 0: such an index gets blocks + dense table only, as before round 5
 *                     (23 G k-mers/s).  k > 31 beyond 2^31 columns always steps down.  SBWTGPU_BIG_PATH.
 *   "image_level"     0 (default): the image carries every derived structure (path order + transition table, sparse
 *                     prefix table, probe filter: 43-53 bytes per column for k <= 31, 92 for k = 63); 1: no path order; 2:
 *                     blocks + dense prefix table only (1 byte per column + the table).  Results are the same at every
 *                     level; throughput is not.  SBWTGPU_IMAGE_LEVEL.  A step-down that index_create makes by
 *                     itself (memory) is announced with one line on stderr.
 *   (environment only) SBWTGPU_SPARSE_BUCKETS_PCT: two-entry buckets of the sparse tables per 100 columns (default: 100 for
 *                     k <= 31, 125 for 31 < k <= 63); SBWTGPU_FILTER_LOG2_ADJ: +1 doubles, -1 halves the probe filter (default: 128-bit
 *                     blocks of 8-16 windows, up to 20 where that keeps a filter of more than 128 MB small); SBWTGPU_DEVICE_PRECALC: depth of the dense device prefix table (default:
 *                     log4 n, at most 8 on an image with sparse table and filter, at most 14 otherwise); SBWTGPU_VERBOSE=1 / 2:
 *                     index_create names the parts of the image it builds, with their times, on stderr.
 *   "max_image_bytes" > 0: index_create moves to the next level while the image would be larger than this (and fails
 *                     with SBWTGPU_ERR_OOM if level 2 is still larger); it also steps down by itself when device
 *                     memory runs out.  SBWTGPU_MAX_IMAGE_BYTES.
 *   "force_mega"      1: rank-only images (arbitrary bit vectors) store their block counts relative to a 64-bit base as
 *                     images whose counts pass 2^32 do (tests of that layout at small sizes); default 0.  It changes RANK-ONLY
 *                     images only: the image of an SBWT (n_nodes - 1 set bits: everything but rank() is served) is the same
 *                     with and without it, and its counts are relative only from 2^31 columns on.  That layout is tested on
 *                     small SBWTs by a build with small mega blocks instead (-DSBWT_MEGA_SHIFT=12, sbwt_device.h).
 *   "sort_reads"      1: the path-order kernels take the reads in the order of their first k-mer's path position (a lookup
 *                     and a radix sort per batch inside the caller's workspace; pays only when nothing upstream orders the
 *                     reads and the index is large); default off (SBWTGPU_SORT_READS)
 *   "path_lookahead"  8 (default): how many steps ahead / behind the path order looks for branch points when it chooses
 *                     which successor a column's path takes (paths follow the core of a pan-genome); 0: blind choice
 *                     (SBWTGPU_PATH_LOOKAHEAD)
 *   "path_safe"       substitution-safe bits along the paths (k <= 31; SBWTGPU_PATH_SAFE): 2 (default) wherever the next k
 *                     steps lie on the path, 1 only where the k steps before do too (the first rule), 0 none
 *   "path_stitch"     1 (default): the vertex-disjoint paths are joined into chains through copies of the stretches that
 *                     strains share (at most n/5 copied positions; a graph whose copies would repeat more than n/32
 *                     branching columns keeps its disjoint paths); 0: disjoint paths (SBWTGPU_PATH_STITCH)
 *   "path_stitch_min" shortest stretch worth a copy, default 1 (SBWTGPU_PATH_STITCH_MIN) */
int         sbwtgpu_set_tuning(const char *key, int64_t value);

/* ---- index life cycle ---- */
/* Replaces SBWT(A,C,G,T,ssup,k,n_kmers,precalc_k) ctor (SBWT.hh:335-353) and the tail of
 * SBWT::load (SBWT.hh:500-516): builds the device image (interleaved 64-column blocks with
 * rank counts), the C array, and the prefix table(s), on HIP device `device`. */
int  sbwtgpu_index_create(const sbwtgpu_index_desc *desc, int device, sbwtgpu_index **out);
void sbwtgpu_index_destroy(sbwtgpu_index *idx);
int  sbwtgpu_index_get_info(const sbwtgpu_index *idx, sbwtgpu_index_info *info);
/* get_precalc() (SBWT.hh:131): copies the 4^precalc_k (first,second) pairs to host memory. */
int  sbwtgpu_index_get_precalc(const sbwtgpu_index *idx, int64_t *out_pairs);

/* ---- construction on the device ---- */
/* The plain-matrix SBWT of a set of sequences, built on the GPU: what the reference's constructors produce
 * (build_nodeboss_in_memory, include/sbwt/NodeBOSSInMemoryConstructor.hh:98-213; the KMC-based SBWT(config) ctor,
 * SBWT.hh:300-332, gives the same bits): the four rows A, C, G, T and suffix_group_starts as sdsl-ordered words.
 * k-mers with anything but upper-case ACGT are skipped (:156-159); add_revcomp adds every reverse complement
 * (src/CLI/sbwt_build.cpp:108-123).  2 <= k <= 64 (a k-mer is packed into 64 or 128 bits); for longer k the C++ host
 * mirror (sbwt::build_plain_matrix_bits) builds on the CPU.  Release with sbwtgpu_free_plain_matrix(). */
typedef struct {
    int64_t   n_nodes, n_kmers, k;
    uint64_t *A_bits, *C_bits, *G_bits, *T_bits;   /* ceil(n_nodes/64) words each */
    uint64_t *suffix_group_starts;                 /* NULL when not requested */
} sbwtgpu_plain_matrix_bits;
int  sbwtgpu_build_plain_matrix(const char *const *seqs, const int64_t *seq_len, int64_t n_seqs, int64_t k,
                                int add_revcomp, int build_streaming_support, int device,
                                sbwtgpu_plain_matrix_bits *out);
void sbwtgpu_free_plain_matrix(sbwtgpu_plain_matrix_bits *bits);

/* ---- multi-GPU replication (no reference equivalent) ---- */
/* One process per GPU (torch.distributed / any launcher): rank 0 exports the device image,
 * the launcher broadcasts header (host bytes) and blob (device bytes, e.g. RCCL broadcast over
 * xGMI), every other rank adopts the received bytes.  The blob is position independent. */
int  sbwtgpu_index_export_header(const sbwtgpu_index *idx, void *header_out, int64_t header_cap,
                                 int64_t *header_bytes);
int  sbwtgpu_index_blob(const sbwtgpu_index *idx, void **dev_ptr, int64_t *bytes);
/* Copies the device image into caller-owned device memory (`bytes` must equal blob_bytes),
 * asynchronously on `stream` -- e.g. into the tensor a launcher hands to its broadcast. */
int  sbwtgpu_index_copy_blob(const sbwtgpu_index *idx, void *dst_dev, int64_t bytes, void *stream);
/* Adopts a caller-owned device blob (must stay alive and unchanged while the handle lives). */
int  sbwtgpu_index_adopt(const void *header, int64_t header_bytes, void *dev_blob, int64_t blob_bytes,
                         int device, sbwtgpu_index **out);
/* Single-process form used by the C++ CLI (--gpus N): replicates `root` onto the listed
 * devices with one RCCL ncclBroadcast; out[i] receives the handle for devs[i] (out[i] == root
 * where devs[i] is the root's device).  devs[] may name a device more than once: the image is sent once
 * per distinct device and the duplicates receive the SAME handle (destroy every distinct handle once). */
int  sbwtgpu_index_bcast(sbwtgpu_index *root, int n_dev, const int *devs, sbwtgpu_index **out);

/* ---- queries, host buffers ---- */
/* SubsetMatrixRank::rank(pos, c) (SubsetMatrixRank.hh:31-37) for n (pos, sym) pairs;
 * pos in [0, n_nodes]; sym is the ASCII char; non-ACGT (upper case) => 0. */
int  sbwtgpu_rank_batch(const sbwtgpu_index *idx, const int64_t *pos, const char *sym, int64_t n,
                        int64_t *out);
/* SBWT::streaming_search(const char*, int64_t) (SBWT.hh:544-581) for n_reads reads:
 * read r = bases[read_off[r] .. read_off[r+1]); its max(0, len-k+1) results are written to
 * out[out_off[r] ..] (out_off[r+1]-out_off[r] must equal that count).  -1 = not found.
 * Returns SBWTGPU_ERR_NO_STREAMING where the reference throws. */
int  sbwtgpu_streaming_search_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                                    int64_t n_reads, int64_t *out, const int64_t *out_off);
/* The non-streaming loop of run_queries_not_streaming (src/CLI/sbwt_search.cpp:78-84):
 * out[out_off[r] + i] = SBWT::search(read_r + i) (SBWT.hh:389-415).  Works with or without
 * streaming support. */
int  sbwtgpu_search_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                          int64_t n_reads, int64_t *out, const int64_t *out_off);
/* The same two calls with int32 results (result compaction; consumer: print_vector,
 * src/CLI/sbwt_search.cpp:21-43, which only prints the values): the kernels write int32 themselves, so a result costs
 * 4 bytes of HBM writes and of PCIe instead of 8.  Only for indexes of fewer than 2^31 columns (SBWTGPU_ERR_INVALID_ARG otherwise); -1
 * stays -1.  out[] is indexed like the int64 calls' (out_off in results, not bytes). */
int  sbwtgpu_streaming_search_batch_i32(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                                        int64_t n_reads, int32_t *out, const int64_t *out_off);
int  sbwtgpu_search_batch_i32(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                              int64_t n_reads, int32_t *out, const int64_t *out_off);
/* SBWT::update_sbwt_interval(S, len, I) (SBWT.hh:422-437) for n independent queries:
 * query q extends interval (first[q], second[q]) by bases[off[q] .. off[q+1]) in place. */
int  sbwtgpu_update_interval_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *off,
                                   int64_t n, int64_t *first, int64_t *second);
/* SBWT::forward(node, c) (SBWT.hh:368-381) for n (node, sym) pairs. */
int  sbwtgpu_forward_batch(const sbwtgpu_index *idx, const int64_t *node, const char *sym, int64_t n,
                           int64_t *out);
/* SBWT::partial_search(input, len) (SBWT.hh:525-537) for n queries: query q = bases[off[q] .. off[q+1]); first/second
 * receive the interval of the longest matched prefix (every char upper-cased first, :529), matched its length. */
int  sbwtgpu_partial_search_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *off, int64_t n,
                                  int64_t *first, int64_t *second, int64_t *matched);
/* SBWT::get_kmer / get_kmer_fast (SBWT.hh:700-746) for n columns: out[q*k .. q*k+k) = the k-mer of column
 * colex_rank[q] ('$'-padded on the left for dummy columns), not NUL-terminated. */
int  sbwtgpu_get_kmer_batch(const sbwtgpu_index *idx, const int64_t *colex_rank, int64_t n, char *out);
/* SubsetMatrixSelectSupport::select(j, c) (SubsetMatrixSelectSupport.hh:27-33) for n (j, sym) pairs: the column
 * holding the j-th set bit (1-based) of row sym; non-ACGT => 0.  j must be in [1, ones of the row]. */
int  sbwtgpu_select_batch(const sbwtgpu_index *idx, const int64_t *j, const char *sym, int64_t n, int64_t *out);

/* ---- queries, device buffers (asynchronous on `stream`) ----
 * The device entry points cannot look at the offsets: the caller guarantees that read_off/out_off are
 * non-decreasing, that out_off matches max(0, len-k+1) per read, that no read has 2^31 or more bases
 * and that one call carries fewer than 2^36 bases. */
/* Scratch the search kernels need: a work-queue header, the 2-bit re-encoding of the bases (total_bases/2 + 64
 * bytes), the list of reads the fused kernel hands on (total_bases/8), the pieces of long reads (total_bases/32, at
 * least 8 MB for batches of more than 32 Mbases) and, while "sort_reads" is on, room to sort the reads (about one more
 * byte per base).  Non-decreasing in total_bases: the caller allocates it once for its largest batch and may reuse it
 * across calls on the same stream.  Calls on DIFFERENT streams may run concurrently on one handle when each has its own
 * workspace (and result range): two batches in flight keep the chip full while the waves of the earlier launch leave one
 * by one -- +6 % on 10 M-read batches, +20 % on 1 M-read batches. */
int64_t sbwtgpu_search_workspace_bytes(int64_t total_bases);
int  sbwtgpu_streaming_search_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                                  const int64_t *d_read_off, int64_t n_reads, int64_t *d_out,
                                  const int64_t *d_out_off, void *d_workspace, int64_t workspace_bytes,
                                  void *stream);
int  sbwtgpu_search_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                        const int64_t *d_read_off, int64_t n_reads, int64_t *d_out,
                        const int64_t *d_out_off, void *d_workspace, int64_t workspace_bytes,
                        void *stream);
/* The same two calls with int32 results on the device (d_out is an int32 array indexed by d_out_off, in results): every kernel
 * of the route writes 4 bytes per k-mer, half the write requests of a launch (a third of its time: +10-13 % k-mers/s on
 * BASELINE config 2, 226 -> 256 G).  Indexes of fewer than 2^31 columns only (SBWTGPU_ERR_INVALID_ARG otherwise); -1 stays -1. */
int  sbwtgpu_streaming_search_dev_i32(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                                      const int64_t *d_read_off, int64_t n_reads, int32_t *d_out,
                                      const int64_t *d_out_off, void *d_workspace, int64_t workspace_bytes,
                                      void *stream);
int  sbwtgpu_search_dev_i32(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                            const int64_t *d_read_off, int64_t n_reads, int32_t *d_out,
                            const int64_t *d_out_off, void *d_workspace, int64_t workspace_bytes,
                            void *stream);
int  sbwtgpu_rank_dev(const sbwtgpu_index *idx, const int64_t *d_pos, const char *d_sym, int64_t n,
                      int64_t *d_out, void *stream);
/* The two halves of the calls above, for callers that re-run a search on bases that are already
 * encoded or that want to time the kernels separately: (1) 2-bit re-encoding of the bases into
 * the workspace, (2) the search over an encoded workspace.  streaming != 0 selects
 * streaming_search, 0 the per-k-mer search loop. */
int  sbwtgpu_encode_bases_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                              void *d_workspace, int64_t workspace_bytes, void *stream);
int  sbwtgpu_search_encoded_dev(const sbwtgpu_index *idx, int64_t total_bases, const int64_t *d_read_off,
                                int64_t n_reads, int64_t *d_out, const int64_t *d_out_off,
                                void *d_workspace, int64_t workspace_bytes, int streaming, void *stream);
/* Synchronises `stream`, then reports the status word of the last search on this workspace
 * (0; SBWTGPU_ERR_NOT_SINGLETON: a k-mer search did not end on one column; SBWTGPU_ERR_STALLED: a workgroup of the
 * sorted fused kernel made no progress for 2^20 waits and gave up). */
int  sbwtgpu_workspace_status(const void *d_workspace, void *stream, int *status);
/* Synchronises `stream`, then reports the work the last search on this workspace performed:
 * stats[0] streaming one-step extensions, [1] full searches, [2] interval updates executed past the
 * device prefix table, [3] device prefix-table lookups that returned a non-empty interval, [4] k-mers
 * answered along path runs (streaming steps that needed no block access), [5] substitutions bridged by the
 * path's safe bits, [6..7] reserved (0). */
int  sbwtgpu_workspace_stats(const void *d_workspace, void *stream, int64_t stats[8]);
/* Measurement aid (bench.py's roofline leg): after sbwtgpu_set_tuning("kernel_events", 1), sbwtgpu_streaming_search_dev /
 * sbwtgpu_search_dev record a pair of HIP events on their stream around the dominant kernel (k_search_fused) of every
 * call, without synchronising; this waits for them and reports the durations in ms, oldest first (the last 256 calls
 * since the switch was set; *n = how many). */
int  sbwtgpu_kernel_times(double *ms, int64_t cap, int64_t *n);

/* ---- output formatting on the device ---- */
/* print_vector of src/CLI/sbwt_search.cpp:21-43 for a whole batch: one line per read, every value
 * followed by one space, '\n' per read, -1 as "-1", 0 as an empty token (the reference's behaviour).
 * d_line_off (n_reads+1 entries) receives the byte offset of every read's line; d_line_off[n_reads] is
 * the length of the text.  text_cap must be >= sbwtgpu_format_text_bound(). */
int64_t sbwtgpu_format_text_bound(const sbwtgpu_index *idx, int64_t n_values, int64_t n_reads);
int64_t sbwtgpu_format_scratch_bytes(int64_t n_reads);
int  sbwtgpu_format_results_dev(const sbwtgpu_index *idx, const int64_t *d_values, const int64_t *d_out_off,
                                int64_t n_reads, int64_t n_values, char *d_text, int64_t text_cap,
                                int64_t *d_line_off, void *d_scratch, int64_t scratch_bytes, void *stream);
/* The whole `sbwt search` inner loop for one batch of reads in host memory (run_queries_streaming /
 * run_queries_not_streaming, src/CLI/sbwt_search.cpp:46-91): searches every read (streaming != 0:
 * streaming_search, else the per-k-mer search loop) and returns the formatted output text.  Large
 * batches are cut into chunks that are pipelined over two HIP streams with pinned staging buffers
 * (H2D of chunk i+1 and D2H of chunk i-1 overlap the kernels of chunk i).  *text is malloc'ed by the
 * library: release it with sbwtgpu_free_host().  *n_queries receives the number of k-mers searched. */
int  sbwtgpu_search_text_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                               int64_t n_reads, int streaming, char **text, int64_t *text_bytes,
                               int64_t *n_queries);
/* The same, streamed: `sink` is called from the calling thread with consecutive pieces of the output text, in order, each
 * straight out of a pinned staging buffer that is only valid during the call (what `sbwt search` writes to its output
 * file: no copy of the whole text is ever made).  A non-zero return of the sink aborts the call.
 * Concurrency: several host threads may call this (and every other search entry point) on ONE index at the same time --
 * the handle is immutable and a call owns its stream, its staging slots (three per call here: pinned text, pinned input and
 * device buffers sized by the batch; at most eight are parked between calls) and its workspace; `sbwt search` drives two
 * such calls in turn (SBWT_CLI_SEARCH_THREADS=1: one).  NOT thread-safe: sbwtgpu_set_tuning() and the measurement aids
 * behind it ("kernel_events" / sbwtgpu_kernel_times: one unsynchronised event ring per process) -- set them before the
 * threads start and keep "kernel_events" off while calls overlap. */
typedef int (*sbwtgpu_text_sink)(void *ctx, const char *text, int64_t bytes);
int  sbwtgpu_search_text_stream(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                                int64_t n_reads, int streaming, sbwtgpu_text_sink sink, void *sink_ctx,
                                int64_t *n_queries);
void sbwtgpu_free_host(void *p);
/* sbwtgpu_search_text_batch keeps its pinned staging and device buffers for the next call, and every host thread
 * keeps one small (1 MiB) pinned + device buffer pair and a stream per device for small host-buffer calls (the
 * reference's scalar API arrives as batches of one); this frees the parked buffers and the calling thread's. */
void sbwtgpu_release_cached_buffers(void);

/* ---- k-bounded matching statistics (MS) ----
 * Column j has the label L_j: its k characters, '$'-padded on the left for dummies (L_0 = $^k), in colex order.  The LCS
 * array: lcs[0] = 0, lcs[j] = the length of the longest common suffix of L_{j-1} and L_j ('$' never counts), in [0, k-1].
 * For a read s and each position i, MS gives len[i]: the largest d in [0, k] such that s[i-d+1 .. i] is upper-case ACGT and
 * a suffix of some label -- for a string over ACGT of length <= k the same as a substring of an indexed k-mer -- and
 * [first[i], second[i]]: the colex range of the columns whose labels end with that suffix ([0, n_nodes-1] when len[i] == 0).
 * Any byte other than upper-case A/C/G/T ends a match (len 0 there).  len[i] == k exactly when the k-mer ending at i is in
 * the index, and then first[i] == second[i] is its column.
 *
 * sbwtgpu_index_build_lcs builds the LCS array on the device (idempotent, thread-safe; 1 byte per column in an allocation
 * of its own, not part of the image nor of its byte cap, plus 4 bytes per column of scratch while it runs; a replica made by
 * adopt / bcast builds its own).  SBWTGPU_ERR_OOM leaves the index usable for everything else.  Every call below builds it
 * first when needed.  Rank-only indexes: SBWTGPU_ERR_INVALID_ARG. */
int  sbwtgpu_index_build_lcs(sbwtgpu_index *idx);
/* out[0 .. n_nodes): the LCS array */
int  sbwtgpu_index_get_lcs(const sbwtgpu_index *idx, uint8_t *out);
/* read r = bases[read_off[r] .. read_off[r+1]); the result of base b goes to slot b (len[b], first[b], second[b]), so the
 * arrays hold read_off[n_reads] entries.  first and second: both NULL (lengths only) or both non-NULL.  A read of 2^31 bases
 * or more: SBWTGPU_ERR_READ_TOO_LONG. */
int  sbwtgpu_matching_statistics_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                                       int64_t n_reads, uint8_t *len, int64_t *first, int64_t *second);
/* The same on device buffers, asynchronous on `stream` (after the LCS array exists: the first call builds it and waits):
 * slot b of d_len / d_first / d_second answers d_bases[b], for the reads d_read_off[0 .. n_reads] (device offsets into
 * d_bases, total_bases = d_read_off[n_reads] - d_read_off[0]).  The workspace (sbwtgpu_ms_workspace_bytes, 16-byte aligned)
 * receives the launch's counters, read back by sbwtgpu_ms_workspace_stats: { positions answered, bases walked (warm-up
 * included), positions with len == k, contractions, contractions that recomputed their interval }. */
int64_t sbwtgpu_ms_workspace_bytes(int64_t total_bases);
int  sbwtgpu_matching_statistics_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                                     const int64_t *d_read_off, int64_t n_reads, uint8_t *d_len, int64_t *d_first,
                                     int64_t *d_second, void *d_workspace, int64_t workspace_bytes, void *stream);
int  sbwtgpu_ms_workspace_stats(const void *d_workspace, void *stream, int64_t stats[5]);

/* ---- unitigs: an index turned back into sequence ----
 * The unitigs of the node-centric de Bruijn graph of the indexed k-mers, spelled on the device: every indexed k-mer exactly
 * once, in about 1 + (k-1) / mean unitig length bytes per k-mer.  It is the inverse of sbwtgpu_build_plain_matrix:
 * building from the unitigs with add_revcomp = 0 gives the rows, marks, n_nodes and n_kmers of the index back, bit for bit.
 *
 *   real column     its label has no '$': k backward steps from it do not pass column 0.  There are n_kmers of them.
 *   out-neighbours  of a real column v: C[c] + rank_c(g) for each c in the set of g, the first column of v's suffix group.
 *                   They are real.
 *   in-neighbours   of w: the real members of the suffix group whose first column is pred(w); none if pred(w) is a dummy.
 *                   (A group that holds a real column holds only real columns.)
 *   internal edge   v -> w with outdeg(v) = 1 and indeg(w) = 1.
 *   unitig          a maximal sequence of distinct real columns v1 .. vm joined by internal edges.
 *   start           v is a start unless it has exactly one in-neighbour and that in-neighbour's out-degree is 1.
 *   pure cycle      a component of internal edges with no start (a self-loop such as A^k is one of length 1).  It starts
 *                   at its smallest column and is not closed again.
 *   spelling        label(v1) followed by the last character of v2 .. vm: m + k - 1 bases, upper-case ACGT.
 *   order           ascending column of v1.  The output is fully determined by the index: byte-identical between runs,
 *                   image levels and devices.
 *   strands         the graph is directed, not bidirected: on an index that holds reverse complements the unitigs come in
 *                   reverse-complement pairs.  Merging them is out of scope.
 *
 * sbwtgpu_unitigs_create reads the blocks, the C array and the suffix-group marks only, so it serves every image level and
 * layout; an index without marks gets them derived into scratch, the image is not changed.  Columns are 32-bit unsigned as
 * in the image (indexes of 2^32 - 2^24 columns or more: SBWTGPU_ERR_INVALID_ARG), offsets into the bases 64-bit.  The work
 * does not depend on the length of the longest unitig: list ranking by pointer jumping, at most ceil(log2 n_nodes) rounds.
 * Scratch: 38 bytes per column, released before the call returns; the result: total_bases + 16 bytes per unitig.
 * SBWTGPU_ERR_OOM leaves the index usable.  Rank-only indexes: SBWTGPU_ERR_INVALID_ARG.  An index with no real column
 * gives 0 unitigs.  Thread-safe on an immutable handle like the query calls (a call owns its stream and its scratch). */
typedef struct sbwtgpu_unitigs sbwtgpu_unitigs;
typedef struct sbwtgpu_colorsets sbwtgpu_colorsets;     /* (described with the colour sets, below) */
int  sbwtgpu_unitigs_create(const sbwtgpu_index *idx, sbwtgpu_unitigs **out);      /* device-resident result */
/* n_kmers = the sum of (length of unitig i) - k + 1 = the index's n_kmers */
int  sbwtgpu_unitigs_info(const sbwtgpu_unitigs *u, int64_t *n_unitigs, int64_t *total_bases, int64_t *n_kmers);
/* unitig i is d_bases[d_off[i] .. d_off[i+1]) and starts with the label of column d_first_col[i]; the pointers live as long
 * as the handle (d_off: n_unitigs + 1 entries, d_first_col: n_unitigs) */
int  sbwtgpu_unitigs_dev(const sbwtgpu_unitigs *u, const char **d_bases, const int64_t **d_off /* n+1 */,
                         const int64_t **d_first_col /* n */);
/* the same into host memory: bases[total_bases], off[n_unitigs + 1], first_col[n_unitigs] */
int  sbwtgpu_unitigs_copy(const sbwtgpu_unitigs *u, char *bases, int64_t *off, int64_t *first_col /* may be NULL */);
/* measurement aid (tools/unitig_bench.py): device-event times of the passes of the create call in ms -- [0] predecessors
 * and marks, [1] real flags, [2] internal edges, [3] pointer jumping, [4] ids and offsets, [5] bases -- and the number of
 * pointer-jumping rounds */
int  sbwtgpu_unitigs_stats(const sbwtgpu_unitigs *u, double pass_ms[6], int64_t *jump_rounds);
void sbwtgpu_unitigs_destroy(sbwtgpu_unitigs *u);

/* ---- coloured unitigs: unitigs cut where the colour set changes ----
 * The maximal paths on which every k-mer carries the same colour set, each with the id of that set: what a coloured index
 * exports (a FASTA file and a table of sets).  The input is a colour-set object s of an index (declared further down); the
 * terms real column, out-neighbours, in-neighbours, spelling, order and strands are those of sbwtgpu_unitigs_create.
 *
 *   S(v)            for a real column v the set s means for it: the row table[ids[v]].  Two columns have the same set when
 *                   their rows are equal word for word; equal ids are sufficient but not necessary (an uploaded object may
 *                   hold duplicate rows).
 *   internal edge   v -> w with outdeg(v) = 1, indeg(w) = 1 and S(v) = S(w).
 *   colour break    v -> w with outdeg(v) = 1, indeg(w) = 1 and S(v) != S(w).  n_color_breaks counts them.
 *   coloured unitig a maximal sequence of distinct real columns joined by (coloured) internal edges.
 *   start           v is a start unless it has exactly one in-neighbour u, outdeg(u) = 1 and S(u) = S(v).
 *   pure cycle      a component of coloured internal edges with no start, so all of its columns carry one set.  It starts at
 *                   its smallest column and is not closed again.
 *   cycle with a break  a cycle of plain internal edges with at least one colour break is not a pure cycle: its pieces start
 *                   at the targets of the breaks, and a piece may run across the place where the plain unitig was cut.
 *   empty set       real columns with the empty set (id 0) form coloured unitigs like any other set.  Nothing is dropped:
 *                   the sum of (length - k + 1) over the result is n_kmers.
 *   set id          of unitig i: ids[first_col[i]].  For an object in canonical form it is the id of the set; for one with
 *                   duplicate rows, the id its first column happens to carry.
 *   order           ascending column of the first k-mer.
 *   determinism     the output is a function of the index, the matrix the object means and, for set_id only, its ids:
 *                   byte-identical between runs, image levels, layouts and devices.
 *   no breaks       if every real column carries the same set, bases, offsets and first columns equal those of
 *                   sbwtgpu_unitigs_create byte for byte.
 *
 * The object knows its index (as in sbwtgpu_pseudoalign_sets_*); the index must outlive the call, the result does not
 * reference the colour-set object afterwards.  sbwtgpu_unitigs_info, _dev, _copy, _stats and _destroy serve the handle as they
 * serve a plain one (the set-id gather is booked under pass [4]); the three calls below on a handle of sbwtgpu_unitigs_create:
 * SBWTGPU_ERR_INVALID_ARG.  Refused with SBWTGPU_ERR_INVALID_ARG: NULL arguments and what sbwtgpu_unitigs_create refuses for
 * the object's index.  Scratch stays 38 bytes per column (ids and table are read in place), the result grows by 4 bytes per
 * unitig.  SBWTGPU_ERR_OOM leaves index and object usable.  Thread-safe on immutable handles. */
int  sbwtgpu_unitigs_create_colored(const sbwtgpu_colorsets *s, sbwtgpu_unitigs **out);
int  sbwtgpu_unitigs_set_ids_dev (const sbwtgpu_unitigs *u, const uint32_t **d_set_id /* n_unitigs */);
int  sbwtgpu_unitigs_set_ids_copy(const sbwtgpu_unitigs *u, uint32_t *set_id);
int  sbwtgpu_unitigs_color_info  (const sbwtgpu_unitigs *u, int64_t *n_color_breaks, int64_t *n_sets, int32_t *n_colors);

/* ---- the unitig graph: links between unitigs, the coordinate of every k-mer ----
 * The unitigs above are the segments of the compacted de Bruijn graph; this adds its edges and, for every indexed k-mer, where
 * on the segments it lies.  The terms real column, out-neighbours, unitig, start, pure cycle and order (and for a coloured
 * run internal edge and colour break) are those of the two sections above.
 *
 *   link            let t_i be the last column of unitig i.  For every out-neighbour w of t_i there is one link i -> j, where j
 *                   is the unitig whose first column is w.  Such a j always exists: the edge t_i -> w is not internal, so w is
 *                   a start, and for a cut cycle w is the head, a first column as well.  So a cut pure cycle (A^k included)
 *                   has the self-link i -> i, a colour break is a link, and the columns of one suffix group, each the tail of
 *                   a unitig of its own, have the same targets.
 *   layout          CSR: link_off[n_unitigs + 1] (int64), link_to[n_links] (uint32); the links of unitig i are
 *                   link_to[link_off[i] .. link_off[i+1]).
 *   order           by source unitig, within a source by edge character A < C < G < T, which is also ascending target column
 *                   and ascending target unitig.  The targets of one source are distinct.
 *   invariant       n_links = n_edges - (n_kmers - n_unitigs), n_edges the number of pairs (x, x[1:] + c) of indexed k-mers.
 *   column map      for a real column v: col_unitig[v] is the number of its unitig and col_offset[v] the position r of its
 *                   k-mer in the spelling, so bases[off[u] + r .. + k) is the label of v.  Both uint32[n_nodes]; a dummy
 *                   column has 0xFFFFFFFF in both.
 *   locate          cols[i] is an int64 search result; the answer is (col_unitig, col_offset) of that column, and 0xFFFFFFFF
 *                   in both for a negative value, a value >= n_nodes and a dummy column.
 *   determinism     a function of the index and, for a coloured run, of the matrix the object means: byte-identical between
 *                   runs, image levels, layouts, and marks given or derived.
 *
 * sbwtgpu_unitigs_create_graph takes exactly one of idx (the plain run) and s (the coloured run) and the flags below; flags = 0
 * gives what sbwtgpu_unitigs_create / _create_colored give, which take that path themselves and run no kernel of this
 * section.  The links and the map are made from the ranking state of the same call before its scratch is freed (two flat
 * launches and a scan for the links, one launch for the map); scratch stays 38 bytes per column, the result grows by
 * 8 (n_unitigs + 1) + 4 n_links bytes for the links and 8 n_nodes for the map.  _info, _dev, _copy, _stats, _set_ids_*,
 * _color_info and _destroy serve a graph handle unchanged.  The _dev pointers live as long as the handle;
 * sbwtgpu_unitigs_locate_dev runs on the caller's stream and never synchronises, _locate_batch takes host memory.
 * Refused with SBWTGPU_ERR_INVALID_ARG: both or neither of idx and s, unknown flag bits, a links call on a handle made without
 * SBWTGPU_UNITIGS_LINKS, a map or locate call on one made without SBWTGPU_UNITIGS_COLUMN_MAP, NULL outputs, n < 0, and what
 * the two create calls refuse.  SBWTGPU_ERR_OOM leaves index and object usable and nothing allocated.  The queries are
 * thread-safe on an immutable handle. */
#define SBWTGPU_UNITIGS_LINKS       1u
#define SBWTGPU_UNITIGS_COLUMN_MAP  2u
int  sbwtgpu_unitigs_create_graph(const sbwtgpu_index *idx, const sbwtgpu_colorsets *s, unsigned flags, sbwtgpu_unitigs **out);
int  sbwtgpu_unitigs_links_info (const sbwtgpu_unitigs *u, int64_t *n_links);
int  sbwtgpu_unitigs_links_dev  (const sbwtgpu_unitigs *u, const int64_t **d_link_off /* n_unitigs + 1 */,
                                 const uint32_t **d_link_to /* n_links */);
int  sbwtgpu_unitigs_links_copy (const sbwtgpu_unitigs *u, int64_t *link_off, uint32_t *link_to /* may be NULL if n_links = 0 */);
int  sbwtgpu_unitigs_column_map_dev (const sbwtgpu_unitigs *u, const uint32_t **d_col_unitig, const uint32_t **d_col_offset);
int  sbwtgpu_unitigs_column_map_copy(const sbwtgpu_unitigs *u, uint32_t *col_unitig, uint32_t *col_offset);   /* n_nodes each */
int  sbwtgpu_unitigs_locate_dev  (const sbwtgpu_unitigs *u, const int64_t *d_cols, int64_t n, uint32_t *d_unitig,
                                  uint32_t *d_offset, void *stream);
int  sbwtgpu_unitigs_locate_batch(const sbwtgpu_unitigs *u, const int64_t *cols, int64_t n, uint32_t *unitig, uint32_t *offset);
/* measurement aid (tools/unitig_links_bench.py): device-event times of the link passes and of the map pass in ms, like _stats */
int  sbwtgpu_unitigs_graph_stats (const sbwtgpu_unitigs *u, double *links_ms, double *map_ms);

/* ---- set operations on two indexes: union, intersection, difference, symmetric difference ----
 * The columns of an index are its k-mers in sorted order, so two indexes combine without their input sequences and without
 * a sort: the keys of the real columns of each (label extraction on the device), one merge under the operation's rule, and
 * the part of the device builder that starts from sorted distinct k-mers.
 *
 * CONTRACT: the result is bit for bit what sbwtgpu_build_plain_matrix returns for the result set's k-mers given as n
 * sequences of length k with add_revcomp = 0: rows, marks, n_nodes and n_kmers.  (So an empty result is what that call
 * returns for no sequence at all: the root column alone.)  Release it with sbwtgpu_free_plain_matrix.
 *
 * Both handles must be on the same device and have the same k, 2 <= k <= 64 (the device builder's key: 64 or 128 bits);
 * anything else is SBWTGPU_ERR_INVALID_ARG with a message naming the mismatch, as are rank-only indexes and indexes of
 * 2^32 - 2^24 columns or more (columns are 32-bit unsigned as in the image).  a == b is allowed.  Neither index needs
 * suffix-group marks: only the blocks and the C array are read, so every image level and layout is served.  Scratch: 37
 * bytes per column of an index for k <= 32, 69 above, then about 34 (50) bytes per key of the two lists together; all of
 * it is released before the call returns.  SBWTGPU_ERR_OOM leaves both indexes untouched and usable.
 * The builder's host-side dummy limit applies unchanged: a result with n_nopred x k > 2^26 (n_nopred: its k-mers without a
 * predecessor in it) is SBWTGPU_ERR_OOM -- intersections and differences of fragmented sets reach it sooner than genomes
 * do -- and `info`, when given, still carries the counts and n_nopred then.
 * Thread-safe on immutable handles like the query calls (a call owns its stream and its scratch). */
#define SBWTGPU_SETOP_UNION 0
#define SBWTGPU_SETOP_INTERSECTION 1
#define SBWTGPU_SETOP_DIFFERENCE 2      /* a minus b */
#define SBWTGPU_SETOP_SYMMETRIC_DIFFERENCE 3
typedef struct {
    int64_t n_a, n_b, n_both, n_either;   /* |A|, |B|, |A and B|, |A or B| */
    int64_t n_result, n_nopred;           /* k-mers of the result; those without a predecessor in it */
    double  pass_ms[4];                   /* keys of a, keys of b, merge+select, builder tail + columns */
} sbwtgpu_setop_info;
int  sbwtgpu_index_setop(const sbwtgpu_index *a, const sbwtgpu_index *b, int op, int build_streaming_support,
                         sbwtgpu_plain_matrix_bits *out, sbwtgpu_setop_info *info /* may be NULL */);
/* the four counts alone (Jaccard = n_both / n_either, containment = n_both / n_a): nothing is built; n_result and n_nopred
 * are 0, pass_ms[3] is 0 */
int  sbwtgpu_index_setop_counts(const sbwtgpu_index *a, const sbwtgpu_index *b, sbwtgpu_setop_info *info);
/* The sorted keys themselves, for callers and tests: 8 (k <= 32) or 16 (32 < k <= 64) bytes per k-mer, little-endian,
 * n_kmers of them, ascending = column order.  Character i of the k-mer (A, C, G, T = 0 .. 3) is at bits 2i of its key.
 * *n_keys and *key_bytes are set whenever the extraction ran; cap_bytes < n_keys x key_bytes: SBWTGPU_ERR_INVALID_ARG and
 * nothing is written to out_keys (out_keys = NULL with cap_bytes = 0 asks for the two numbers). */
int  sbwtgpu_index_kmer_keys(const sbwtgpu_index *idx, void *out_keys, int64_t cap_bytes, int64_t *n_keys, int *key_bytes);

/* ---- per-read hit profiles: counts, covered bases, longest run ----
 * What a screen of reads against an index needs: a handful of numbers per read instead of one value per k-mer (16 bytes per
 * read instead of 4 or 8 per window over PCIe and into the output file).
 *
 * Read r has L bases and m = max(0, L - k + 1) windows.
 *   hits      strands = 1 (forward): hit[i] = 1 exactly where SBWT::search of window i is >= 0 -- the rule of
 *             sbwtgpu_search_batch: any byte other than upper-case A/C/G/T in the window means no hit.
 *             strands = 2 (either strand): hit[i] = forward hit, OR the reverse complement of window i is indexed.  The
 *             complement is A<->T, C<->G on upper-case bytes only; a window holding any other byte is no hit on either strand.
 *   record    four int32_t per read, in read order:
 *             n_kmers       = m
 *             n_found       = the sum of hit[i]
 *             covered_bases = the size of the union over hits i of [i, i + k); equivalently the sum over hits i of
 *                             min(k, next_hit(i) - i), with next_hit = +infinity for the last hit
 *             longest_run   = the largest number of consecutive hits; the longest exact match of at least k bases is
 *                             longest_run + k - 1 when longest_run > 0
 *             A read with m = 0 gives {0, 0, 0, 0}.
 * The search kernels are used as they are (int32 results below 2^31 columns, int64 above; the per-k-mer search semantics, with
 * or without suffix-group marks); new kernels turn their results into one bit per window and the bits into records.  For
 * strands = 2 the whole base buffer is reverse-complemented once and searched as a mirrored batch into the same result buffer.
 * Rank-only indexes: SBWTGPU_ERR_INVALID_ARG.  The result does not depend on tuning, image level or chunking. */
typedef struct { int32_t n_kmers, n_found, covered_bases, longest_run; } sbwtgpu_read_hits;
/* Host buffers: read r = bases[read_off[r] .. read_off[r+1]), out[r] its record.  The batch is cut into chunks of whole reads
 * (tuning "read_hits_chunk_bases"), so device memory is bounded whatever the batch size (a single read longer than the budget
 * is a chunk of its own); only bases and offsets go to the device and only records come back.  Thread-safe on one handle like
 * the search entry points.  A read of 2^31 bases or more: SBWTGPU_ERR_READ_TOO_LONG. */
int     sbwtgpu_read_hits_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads,
                                int strands, sbwtgpu_read_hits *out);
/* Device buffers, one pass over the batch, asynchronous on `stream`, never synchronises.  d_bases holds total_bases bases and
 * d_read_off (n_reads + 1 entries, non-decreasing, d_read_off[n_reads] <= total_bases; d_read_off[0] need not be 0) are
 * offsets into it, as for sbwtgpu_search_dev; the other preconditions are those of the "_dev" search calls, and n_reads < 2^31.
 * d_out: n_reads records.  The workspace (16-byte aligned) holds the search workspace, the result buffer (8 bytes per base),
 * the bit vector, the result offsets -- computed on the device from d_read_off and k -- and, for two strands, the mirrored
 * bases and offsets: about 10.2 (11.2) bytes per base + 24 (40) per read.  Its size is non-decreasing in total_bases and in
 * n_reads; a workspace that is too small is SBWTGPU_ERR_INVALID_ARG.  sbwtgpu_workspace_status on the workspace reports the
 * status word of the call's last search.  Calls on different streams may run concurrently on one handle when each has its
 * own workspace and records. */
int64_t sbwtgpu_read_hits_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands);
int     sbwtgpu_read_hits_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                              int64_t n_reads, int strands, sbwtgpu_read_hits *d_out, void *d_workspace,
                              int64_t workspace_bytes, void *stream);

/* ---- reads threaded through the unitig graph: walks and unitig coverage ----
 * Which unitigs a read runs along, and how far: a few 16-byte records per read instead of 8 bytes per window from search +
 * locate.  The inputs are an index, a graph handle u made from it with SBWTGPU_UNITIGS_COLUMN_MAP (plain or coloured) and a
 * batch of reads given as sbwtgpu_read_hits_* takes them.  One strand only.
 *
 * Read r has L bases and m = max(0, L - k + 1) windows.  Window i hits when SBWT::search of it is >= 0 -- the rule of
 * sbwtgpu_search_batch: any byte other than upper-case A/C/G/T in the window means no hit.  A hit has a coordinate (U_i, O_i):
 * the column map's pair for its column (a search result is never a dummy column).
 *   step        a maximal range of windows [i, i + n) of one read in which every window hits and U_{j+1} = U_j,
 *               O_{j+1} = O_j + 1 for every consecutive pair.
 *   record      { unitig = U_i, offset = O_i, read_pos = i, n_kmers = n }
 *   layout      CSR: step_off[n_reads + 1] (int64, step_off[0] = 0); steps[step_off[r] .. step_off[r+1]) are read r's steps by
 *               ascending read_pos.  A read with no hit, or with m = 0, has none.
 *   what follows  the steps of a read do not overlap.  Step s+1 CONTINUES step s when read_pos[s+1] = read_pos[s] + n_kmers[s];
 *               then offset[s] + n_kmers[s] is unitig s's k-mer count, offset[s+1] = 0, and (unitig[s], unitig[s+1]) is a link
 *               of the handle (for a coloured handle a colour break is a link; a read going round a cut cycle repeats the
 *               unitig through its self-link).  Otherwise at least one window between the two misses.  The sum of n_kmers over
 *               a read is n_found of its sbwtgpu_read_hits record (strands = 1).
 *   coverage    optional int64[n_unitigs]: entry j is the sum of n_kmers over all steps of the batch with unitig = j -- the
 *               GFA KC value of segment j for the read set.
 *   determinism a function of the index, the handle and the reads: byte-identical between runs, image levels, tuning, chunking,
 *               and marks given or derived.
 *
 * sbwtgpu_unitigs_walks_prepare builds the handle's start bitmap (one bit per column: its offset in its unitig is 0; n_nodes / 8
 * bytes, owned by the handle and freed by sbwtgpu_unitigs_destroy) with one streaming pass over the column map; idempotent and
 * thread-safe.  The create calls are unchanged and launch and allocate nothing for it.
 *
 * _dev: asynchronous on `stream`, never synchronises, never allocates; needs a prepared handle.  The preconditions are those of
 * sbwtgpu_read_hits_dev (d_read_off[0] need not be 0, n_reads < 2^31).  d_step_off[n_reads] always receives the true number of
 * steps, also when it exceeds steps_cap: the caller compares (the number of windows is always enough).  Only the steps of
 * number < steps_cap are stored, nothing at or beyond d_steps[steps_cap].  d_unitig_kmers, when given, is ADDED to (all steps
 * count, stored or not), so a caller sums batches; steps_cap below the number of steps TOGETHER with coverage is a slow path
 * (every step that is not stored is walked back to its start, 64 windows per load).  The workspace (16-byte aligned) holds the search workspace first -- so
 * sbwtgpu_workspace_status reports the search's status word -- then the int32 results (4 bytes per base), three bit vectors over
 * the windows and two rank directories (about 0.88 bytes per base) and 32 bytes per read; its size is non-decreasing in both
 * arguments.
 *
 * _batch: host buffers; prepares the handle if needed; cuts the batch into chunks of whole reads (tuning "walks_chunk_bases"),
 * so device memory is bounded.  step_off (n_reads + 1 entries, the caller's) is global over the batch; *steps_out is host
 * memory of the library (release it with sbwtgpu_free_host), NULL with *n_steps = 0 when there are no steps.  unitig_kmers,
 * when given, receives the totals of this call.  Thread-safe on one index and handle like the other queries.
 *
 * SBWTGPU_ERR_INVALID_ARG, with a message naming the cause: a handle made without SBWTGPU_UNITIGS_COLUMN_MAP; _dev on a handle
 * that was not prepared; a handle whose n_nodes or k differ from the index's; an index of 2^31 columns or more; a rank-only
 * index; NULL outputs; n_reads < 0; steps_cap < 0; a workspace that is too small.  A read of 2^31 bases or more:
 * SBWTGPU_ERR_READ_TOO_LONG. */
typedef struct { uint32_t unitig, offset; int32_t read_pos, n_kmers; } sbwtgpu_walk_step;
int     sbwtgpu_unitigs_walks_prepare(sbwtgpu_unitigs *u);
int64_t sbwtgpu_unitigs_walks_workspace_bytes(int64_t total_bases, int64_t n_reads);
int     sbwtgpu_unitigs_walks_dev(const sbwtgpu_index *idx, const sbwtgpu_unitigs *u, const char *d_bases, int64_t total_bases,
                                  const int64_t *d_read_off, int64_t n_reads, int64_t *d_step_off /* n_reads + 1 */,
                                  sbwtgpu_walk_step *d_steps, int64_t steps_cap, int64_t *d_unitig_kmers_or_null /* n_unitigs, added to */,
                                  void *d_workspace, int64_t workspace_bytes, void *stream);
int     sbwtgpu_unitigs_walks_batch(const sbwtgpu_index *idx, const sbwtgpu_unitigs *u, const char *bases, const int64_t *read_off,
                                    int64_t n_reads, int64_t *step_off /* n_reads + 1 */, sbwtgpu_walk_step **steps_out,
                                    int64_t *n_steps, int64_t *unitig_kmers_or_null /* n_unitigs, the totals of this call */);

/* ---- colours and pseudoalignment: which of the indexed references hold a k-mer or a read ----
 * One index over N references (strains of a pan-genome) and one search answer "which references hold this read", instead of
 * N indexes, N searches of the same reads and a join.
 *
 * Colour matrix.  An index of n columns carries n little-endian uint64_t rows and n_colors colours, 1 <= n_colors <= 64.
 *   - Bit c of row j is set exactly when column j is a real column whose k-mer was given for colour c.
 *   - Dummy columns and bits >= n_colors are always 0.
 *   - More than 64 colours: the wide calls below (rows of W words, up to SBWTGPU_MAX_COLORS colours).
 * Colouring.  add(color c, sequences, strands):
 *   - Every window of every sequence is searched with the rule of sbwtgpu_search_batch: upper-case ACGT only; any other byte
 *     in the window means no hit.
 *   - A hit on column j sets bit c of row j.
 *   - strands = 2 also searches the reverse complement of every window and sets bit c on that column too.  This is needed
 *     for indexes built with reverse complements.  The complement rule is read-hits' rule.
 *   - Windows that the index lacks are skipped and counted.
 *   - The call returns n_windows and n_hit_windows.  For two strands, a window counts once if either strand hit.
 *   - Adding is idempotent and order-independent.
 * Colour set of a window.
 *   - S_i is the row of the window's column, or 0 if the window is not found.
 *   - With strands = 2, S_i is the row of the forward hit OR the row of the reverse-complement hit; a missing hit
 *     contributes 0.
 *   - A found window with S_i = 0 counts as not found.
 * Record per read: { uint64_t colors; int32_t n_kmers; int32_t n_found; }, 16 bytes.
 *   - n_kmers = m = max(0, L - k + 1).
 *   - n_found = the number of windows i with S_i != 0.
 *   - count_c = the number of windows i with bit c set in S_i.
 *   - Let D = n_found when denominator = 0 and D = m when denominator = 1.
 *   - Bit c of colors is set exactly when D > 0 and count_c x 1 000 000 >= threshold_ppm x D, in 64-bit integer arithmetic,
 *     1 <= threshold_ppm <= 1 000 000.  No floating point anywhere.
 *   - threshold_ppm = 1 000 000 with denominator = 0 is the classical intersection over the found k-mers.
 *   - m = 0 gives {0, 0, 0}.
 * Optional counts output: n_reads x n_colors int32_t, counts[r x n_colors + c] = count_c.
 * Refusals, each SBWTGPU_ERR_INVALID_ARG with a message naming the cause: rank-only indexes; indexes of 2^31 columns or more
 * (the int32 search results are the only route); n_colors outside 1..64 (1..4096 for the wide create); color >= n_colors; a threshold or denominator out of
 * range; a colours object used with an index of another n_nodes or k (an object is bound to its index when it is created;
 * callers that load rows from a file compare the file's n_columns and k with the index first, as the CLI and the Python
 * binding do).
 *
 * Memory and ownership: sbwtgpu_colors_create allocates 8 bytes per column on the index's device and zeroes them, or uploads
 * rows_or_null (n_nodes rows) after clearing bits >= n_colors and the rows of dummy columns.  The index must outlive the
 * colours object.  SBWTGPU_ERR_OOM leaves the index untouched and usable.
 * Concurrency: the queries (pseudoalign_batch / _dev, info, copy) are thread-safe on one index and one colours object.
 * sbwtgpu_colors_add_batch changes the object and must not run concurrently with anything else on the same object. */
typedef struct sbwtgpu_colors sbwtgpu_colors;
typedef struct { int64_t n_columns, k; int32_t n_colors; int64_t n_colored_columns; int64_t per_color[64]; } sbwtgpu_colors_info_t;
typedef struct { uint64_t colors; int32_t n_kmers, n_found; } sbwtgpu_pseudoalignment;

int  sbwtgpu_colors_create(const sbwtgpu_index *idx, int n_colors, const uint64_t *rows_or_null, sbwtgpu_colors **out);
void sbwtgpu_colors_destroy(sbwtgpu_colors *c);
/* Host buffers, as sbwtgpu_read_hits_batch takes them: sequence r = bases[read_off[r] .. read_off[r+1]).  Chunked by whole
 * reads (tuning "pseudoalign_chunk_bases", default 64 Mi) on the parked pipeline slots; only bases and offsets go down.
 * n_windows / n_hit_windows may be NULL.  A sequence of 2^31 bases or more: SBWTGPU_ERR_READ_TOO_LONG. */
int  sbwtgpu_colors_add_batch(sbwtgpu_colors *c, int color, const char *bases, const int64_t *read_off, int64_t n_reads,
                              int strands, int64_t *n_windows, int64_t *n_hit_windows);
/* coloured columns (rows that are not 0) in total and per colour, counted on the device */
int  sbwtgpu_colors_info(const sbwtgpu_colors *c, sbwtgpu_colors_info_t *info);
/* the n_columns rows into host memory / the device array itself (valid as long as the object) */
int  sbwtgpu_colors_copy(const sbwtgpu_colors *c, uint64_t *rows_out);
int  sbwtgpu_colors_dev(const sbwtgpu_colors *c, const uint64_t **d_rows);
/* Host buffers: out[r] the record of read r, counts_or_null the counts.  Chunked like sbwtgpu_colors_add_batch; only records,
 * and counts if asked for, come back.  The result does not depend on tuning, image level or chunking. */
int  sbwtgpu_pseudoalign_batch(const sbwtgpu_colors *c, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                               int threshold_ppm, int denominator, sbwtgpu_pseudoalignment *out, int32_t *counts_or_null);
/* Device buffers, asynchronous on `stream`, never synchronises; the preconditions of sbwtgpu_read_hits_dev (d_read_off[0] need
 * not be 0; n_reads < 2^31).  d_out: n_reads records, 8-byte aligned; d_counts_or_null: n_reads x n_colors int32.  The
 * workspace (16-byte aligned) holds the search workspace first -- sbwtgpu_workspace_status reports the status word of the
 * call's last search -- then the int32 results, the result offsets and, for two strands, the mirrored bases, offsets and
 * results: about 5.1 (10.2) bytes per base + 24 (40) per read.  Its size is non-decreasing in total_bases and in n_reads; a
 * workspace that is too small is SBWTGPU_ERR_INVALID_ARG. */
int64_t sbwtgpu_pseudoalign_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands);
int  sbwtgpu_pseudoalign_dev(const sbwtgpu_colors *c, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                             int64_t n_reads, int strands, int threshold_ppm, int denominator,
                             sbwtgpu_pseudoalignment *d_out, int32_t *d_counts_or_null,
                             void *d_workspace, int64_t workspace_bytes, void *stream);

/* ---- wide colour matrices: more than 64 references ----
 * A wide matrix of an index of n columns is n x W little-endian uint64_t words, row-major, W = ceil(n_colors / 64),
 * 1 <= n_colors <= SBWTGPU_MAX_COLORS.  Word w of column j is at rows[j * W + w].
 *   - Colour c is bit c & 63 of word c >> 6.
 *   - Bit c of row j is set exactly when column j is a real column whose k-mer was given for colour c.
 *   - Dummy columns are all zero.
 *   - Bits >= n_colors in the last word are zero.
 *   - With W = 1 this is the matrix above.
 * Colouring is add(c, sequences, strands) above, unchanged.
 * The colour set S_i of a window is the W-word row of its column.  With two strands it is the word-wise OR of the two rows.
 * It is all zero when nothing is found.  A found window whose row is zero in every word counts as not found.
 * A read's result is three things:
 *   - n_kmers = m = max(0, L - k + 1).
 *   - n_found = #{i : S_i != 0}.
 *   - W words of colors.
 * Bit c of colors is set exactly when D > 0 and count_c x 1 000 000 >= threshold_ppm x D, in 64-bit integers.  D is n_found
 * when denominator = 0 and m when denominator = 1.  This is the same rule as above, with no floating point.
 * The optional counts output is n_reads x n_colors int32.
 * For n_colors <= 64 the wide calls return exactly what the calls above return.
 *
 * One object type serves both: sbwtgpu_colors_add_batch, _copy (n x W words), _dev and _destroy work on any colours object,
 * and every wide call works on an object of sbwtgpu_colors_create.  sbwtgpu_colors_info, sbwtgpu_pseudoalign_batch and
 * sbwtgpu_pseudoalign_dev refuse an object of more than 64 colours (SBWTGPU_ERR_INVALID_ARG, the message names the wide call):
 * their 16-byte record and per_color[64] cannot hold more.  The refusals, ownership and concurrency rules above carry over;
 * SBWTGPU_ERR_OOM for the n x W x 8 bytes leaves the index usable. */
#define SBWTGPU_MAX_COLORS 4096
typedef struct { int32_t n_kmers, n_found; } sbwtgpu_read_found;

int  sbwtgpu_colors_create_wide(const sbwtgpu_index *idx, int n_colors /* 1..4096 */, const uint64_t *rows_or_null /* n_nodes x W */,
                                sbwtgpu_colors **out);
int  sbwtgpu_colors_words(const sbwtgpu_colors *c);            /* W */
/* every output may be NULL; per_color: n_colors entries */
int  sbwtgpu_colors_info_wide(const sbwtgpu_colors *c, int64_t *n_columns, int64_t *k, int32_t *n_colors, int64_t *n_colored_columns,
                              int64_t *per_color);
/* Host buffers: out[r] = {n_kmers, n_found} of read r, colors_out its W words (n_reads x W), counts_or_null n_reads x n_colors.
 * Chunked like sbwtgpu_pseudoalign_batch: 8 + 8 W bytes per read come back, and 4 n_colors more with counts.  The result does not
 * depend on tuning, image level or chunking. */
int  sbwtgpu_pseudoalign_wide_batch(const sbwtgpu_colors *c, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                                    int threshold_ppm, int denominator, sbwtgpu_read_found *out, uint64_t *colors_out,
                                    int32_t *counts_or_null);
/* Device buffers, as sbwtgpu_pseudoalign_dev: the same preconditions, the same workspace (sbwtgpu_pseudoalign_workspace_bytes does
 * not depend on the colours) with the same layout.  d_out: n_reads records of 8 bytes; d_colors: n_reads x W words. */
int  sbwtgpu_pseudoalign_wide_dev(const sbwtgpu_colors *c, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                  int64_t n_reads, int strands, int threshold_ppm, int denominator,
                                  sbwtgpu_read_found *d_out, uint64_t *d_colors, int32_t *d_counts_or_null,
                                  void *d_workspace, int64_t workspace_bytes, void *stream);

/* ---- colour sets: one id per column and a table of the distinct rows ----
 * A colour-set object of an index of n columns (n < 2^31) with n_colors in 1 .. SBWTGPU_MAX_COLORS and
 * W = ceil(n_colors / 64) holds
 *   - ids: n uint32_t;
 *   - n_sets >= 1;
 *   - table: n_sets x W little-endian uint64_t, row-major.
 * It MEANS the wide matrix rows[j * W + w] = table[ids[j] * W + w].
 * Invariants, checked on every way in:
 *   - Row 0 of the table is all zero.
 *   - No other row is all zero, so a column is coloured exactly when ids[j] != 0.
 *   - No bit >= n_colors is set.
 *   - Every id is < n_sets.
 *   - Dummy columns have id 0.
 * Duplicate rows and unused rows are allowed in an uploaded object: queries stay correct and lose only the fast path.
 * Canonical form (what sbwtgpu_colorsets_compress produces and the files written by the CLI hold):
 *   - The distinct non-zero rows of the matrix are numbered 1, 2, ... in the order of the smallest column that carries them.
 *   - Row 0 is the empty set.
 *   - n_sets = 1 + the number of distinct non-zero rows.
 * Two runs of compress give identical bytes.
 * Query results: records, colour words and counts are exactly those of the wide calls above on the matrix the object means --
 * one and two strands, threshold_ppm, denominator, optional counts, and a found window with an empty set counting as not found.
 *
 * Memory: 4 bytes per column and 8 W bytes per distinct set on the index's device.  compress needs, while it runs and beside
 * its result, 13 bytes per column (the slots of a hash table of 2 n + 1 uint32, one flag byte and one uint32 of their scan) and
 * a few KiB; create and info need one byte per column while they run.  The index must outlive the object; the colours object
 * given to compress is unchanged and may be destroyed afterwards.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): those of the colour calls above (rank-only indexes,
 * 2^31 columns or more, ranges, an object of another index, NULL pointers) and, for create, every broken invariant but the
 * dummy columns' ids, which it sets to 0.  SBWTGPU_ERR_OOM leaves index and inputs usable.
 * Concurrency: the queries (pseudoalign_sets_batch / _dev, expand, info, copy) are thread-safe on one object.
 * (The type is declared with the unitigs above, whose coloured call takes one.) */

/* any colours object, W = 1 included */
int  sbwtgpu_colorsets_compress(const sbwtgpu_colors *c, sbwtgpu_colorsets **out);
/* ids: n_nodes entries; table: n_sets x W words.  The checks run on the device. */
int  sbwtgpu_colorsets_create(const sbwtgpu_index *idx, int n_colors, const uint32_t *ids, int64_t n_sets, const uint64_t *table,
                              sbwtgpu_colorsets **out);
/* the wide colours object it means (of sbwtgpu_colors_create_wide; destroy it with sbwtgpu_colors_destroy) */
int  sbwtgpu_colorsets_expand(const sbwtgpu_colorsets *s, sbwtgpu_colors **out);
void sbwtgpu_colorsets_destroy(sbwtgpu_colorsets *s);
/* every output may be NULL; device_bytes = 4 n_columns + 8 words n_sets */
int  sbwtgpu_colorsets_info(const sbwtgpu_colorsets *s, int64_t *n_columns, int64_t *k, int32_t *n_colors, int32_t *words,
                            int64_t *n_sets, int64_t *n_colored_columns, int64_t *device_bytes);
/* ids_out: n_columns entries, table_out: n_sets x W words; either may be NULL */
int  sbwtgpu_colorsets_copy(const sbwtgpu_colorsets *s, uint32_t *ids_out, uint64_t *table_out);
int  sbwtgpu_colorsets_dev(const sbwtgpu_colorsets *s, const uint32_t **d_ids, const uint64_t **d_table);
/* sbwtgpu_pseudoalign_wide_batch and _dev with a colour-set object in the place of the colours object: the same arguments,
 * outputs, chunking ("pseudoalign_chunk_bases") and workspace (sbwtgpu_pseudoalign_workspace_bytes, the same layout). */
int  sbwtgpu_pseudoalign_sets_batch(const sbwtgpu_colorsets *s, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                                    int threshold_ppm, int denominator, sbwtgpu_read_found *out, uint64_t *colors_out,
                                    int32_t *counts_or_null);
int  sbwtgpu_pseudoalign_sets_dev(const sbwtgpu_colorsets *s, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                  int64_t n_reads, int strands, int threshold_ppm, int denominator,
                                  sbwtgpu_read_found *d_out, uint64_t *d_colors, int32_t *d_counts_or_null,
                                  void *d_workspace, int64_t workspace_bytes, void *stream);

/* ---- colour sets built one colour at a time: the builder ----
 * sbwtgpu_colors_create_wide -> sbwtgpu_colors_add_batch x N -> sbwtgpu_colorsets_compress holds an n x W x 8-byte matrix on the
 * device before the 4-byte ids come out.  A colour-set BUILDER takes the same adds and holds only the object it is making.
 * It is bound to one index of n columns (n < 2^31, not rank-only) and one n_colors in 1 .. SBWTGPU_MAX_COLORS;
 * W = ceil(n_colors / 64) is fixed for its life.  Each colour is NEW, OPEN (at most one at a time) or CLOSED.
 * add_batch:
 *   - It is sbwtgpu_colors_add_batch in every respect but the target: the same search rule, strands, meaning of n_windows and
 *     n_hit_windows, chunking by "pseudoalign_chunk_bases" on the parked pipeline slots, and SBWTGPU_ERR_READ_TOO_LONG.
 *   - A hit on column j MARKS j for `color`.  If `color` is open, the marks accumulate.  If another colour is open, that
 *     colour is closed first and `color` opens.
 *   - A closed colour is refused (SBWTGPU_ERR_INVALID_ARG): the sequences of one colour must come in consecutive calls.
 *   - Closing a colour c merges its marks: every marked column's set becomes its old set + {c}.
 *   - Within an open colour, adding is idempotent and order-independent.  Colours may be opened in any order, and colours
 *     may be left out.
 * finish:
 *   - It closes the open colour and returns a colour-set object in canonical form: byte for byte what
 *     sbwtgpu_colorsets_compress returns for a wide object coloured by the same adds.
 *   - The builder is consumed: every later call but destroy is refused.
 * info:
 *   - Before finish, it reports the state as of the last closed colour.  per_color[c] is the number of columns marked when c
 *     was closed, and 0 for new or open colours.  n_colored_columns counts columns with a non-empty set.  device_bytes is
 *     what the builder holds now.
 * Memory: 4 n bytes of ids, n / 8 of marks (in 64-bit words) and cap x (8 W + 4) bytes for a table of cap rows with their
 * column counts; cap starts at 64 rows and doubles when the sets outgrow it (a new allocation, a device copy, a free).
 * While a colour is closed: 4 bytes per set.  While finish runs: 1 + 4 bytes per column, 4 per set and the result's table.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): those of the colour calls (a rank-only index, an
 * index of 2^31 columns or more, n_colors, color or strands out of range, NULL pointers).  SBWTGPU_ERR_OOM or SBWTGPU_ERR_HIP --
 * when the table grows, for one -- leaves the index usable and the builder broken: every later call but destroy then returns
 * SBWTGPU_ERR_INVALID_ARG with "builder is broken".
 * Concurrency: a builder is not thread-safe.  The index must outlive it. */
typedef struct sbwtgpu_colorsets_builder sbwtgpu_colorsets_builder;

int  sbwtgpu_colorsets_builder_create(const sbwtgpu_index *idx, int n_colors, sbwtgpu_colorsets_builder **out);
int  sbwtgpu_colorsets_builder_add_batch(sbwtgpu_colorsets_builder *b, int color, const char *bases, const int64_t *read_off,
                                         int64_t n_reads, int strands, int64_t *n_windows, int64_t *n_hit_windows);
/* every output may be NULL; per_color: n_colors entries */
int  sbwtgpu_colorsets_builder_info(const sbwtgpu_colorsets_builder *b, int64_t *n_columns, int64_t *k, int32_t *n_colors,
                                    int32_t *words, int64_t *n_sets, int64_t *n_colored_columns, int64_t *per_color,
                                    int64_t *device_bytes);
/* the object is independent of the builder (destroy it with sbwtgpu_colorsets_destroy) */
int  sbwtgpu_colorsets_builder_finish(sbwtgpu_colorsets_builder *b, sbwtgpu_colorsets **out);
void sbwtgpu_colorsets_builder_destroy(sbwtgpu_colorsets_builder *b);

/* ---- colour sets carried onto another index: the coloured merge ----
 * sbwtgpu_index_setop combines two indexes when their sequences are gone; this call carries their colours along, without the
 * sequences and without a wide matrix.
 * Inputs: u is a target index; sa is a colour-set object of an index a; sb, which is optional, one of an index b;
 * color_offset_b is an integer.  For a k-mer x, S_a(x) is the colour set sa means for x's column in a, and the empty set when
 * x is not a k-mer of a.  S_b is defined likewise.
 * The result is a colour-set object OF u:
 *   - Every real column j of u, with k-mer x, has the set S_a(x) + { c + color_offset_b : c in S_b(x) }.
 *   - Dummy columns have id 0.
 *   - n_colors_out = max(n_colors_a, color_offset_b + n_colors_b).  It is n_colors_a when sb is NULL.
 *   - W_out = ceil(n_colors_out / 64).
 *   - The object is in the canonical form above: distinct non-zero rows numbered by the smallest column of u that carries
 *     them, row 0 empty, no row unused or duplicated.
 * u may be any index with the same k: the union (the coloured merge), the intersection or a difference (colours restricted
 * to the surviving k-mers), a itself (re-canonicalises an uploaded object), an unrelated index (everything is empty and
 * n_sets = 1).  color_offset_b = n_colors_a concatenates the two colour spaces; color_offset_b = 0 says colour c is the same
 * reference on both sides, and rows are OR-ed.  The inputs may be non-canonical uploaded objects, and with overlapping colour
 * spaces two different pairs (id_a, id_b) can give the same row: the result is canonical in both cases.
 * info (may be NULL): n_real_u = the real columns of u; n_from_a / n_from_b / n_from_both = those whose k-mer is in a / b /
 * both; n_pairs = the distinct pairs (id_a, id_b) other than (0, 0); n_sets of the result; pass_ms on the host clock: keys,
 * locate and gather, pairs and rows, canonical numbering.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL u, sa or out; different k among u, a, b; k
 * outside 2 .. 64 (the set operations' range); a rank-only index among the three; u of 2^31 columns or more; different
 * devices; color_offset_b < 0; color_offset_b != 0 when sb is NULL; n_colors_out > SBWTGPU_MAX_COLORS.
 * sa and sb may be the same object, and u may be a or b.  SBWTGPU_ERR_OOM leaves everything usable.  Scratch, all released
 * before the call returns: the set operations' 37 / 69 bytes per column of one index at a time, 12 / 20 bytes per k-mer of
 * the three indexes for keys and columns, then 25 bytes per k-mer of u and 25 + 8 W_out per distinct pair.
 * Thread-safe on immutable handles: the call owns its stream.  The returned object is bound to u, as every colour-set object
 * is bound to its index; u must outlive it. */
typedef struct { int64_t n_real_u, n_from_a, n_from_b, n_from_both, n_pairs, n_sets; double pass_ms[4]; } sbwtgpu_colorsets_merge_info;
int  sbwtgpu_colorsets_merge(const sbwtgpu_index *u, const sbwtgpu_colorsets *sa, const sbwtgpu_colorsets *sb /* may be NULL */,
                             int color_offset_b, sbwtgpu_colorsets **out, sbwtgpu_colorsets_merge_info *info /* may be NULL */);

/* ---- shared k-mers: how many k-mers each pair of references shares ----
 * A colour-set object s of an index of n columns has C = n_colors, W = ceil(C / 64), n_sets, ids and table.
 *   - Set sizes: size[t] = #{ j : ids[j] = t } for 0 <= t < n_sets.  Dummy columns carry id 0, so size[0] counts them
 *     together with the uncoloured real columns; the sizes sum to n.
 *   - Weights: w[t] = size[t] by default, or a caller-supplied int64 with 0 <= w[t] <= 2^31 - 1.  w[0] is ignored (it is
 *     not even checked): row 0 is the empty set.
 *   - The shared matrix: G[a][b] = the sum of w[t] over the sets t >= 1 whose table row has bits a and b both set, for
 *     0 <= a, b < C.  int64, C x C, row-major, exact: there is no floating point anywhere.
 * With the default weights G[a][b] is the number of index k-mers that references a and b both hold, G[a][a] the number of
 * k-mers of reference a, and G is symmetric (it is with any weights).  Every k-mer distance (Jaccard, containment, ...) is
 * host arithmetic on G.  The result depends on what the object means only: an uploaded object with duplicate rows, unused
 * rows or another numbering gives the G of its canonical form (an unused row has size 0).  Two calls give identical bytes.
 * Objects of fewer than "gram_mfma_min_sets" sets (sbwtgpu_set_tuning; default 512, 0 = always, a huge value = never) take
 * a plain kernel, larger ones the matrix cores (v_mfma_i32_16x16x64_i8 over 7-bit limbs of the weights, 32-bit sums added
 * into the 64-bit matrix every "gram_flush_sets" sets at the latest: default 65536, rounded down to a multiple of 64 and
 * at least 64; a value v with 127 v >= 2^31, or below 1, is refused).  Results never depend on either key.
 * sbwtgpu_shared_info: n_sets_used = the sets t >= 1 with w[t] > 0; used_mfma = 1 for the matrix-core route; n_limbs = the
 * 7-bit limbs of the largest weight (0 .. 5); pass_ms on the host clock: sizes, transpose and compaction (weights, sort,
 * limbs, bit planes), product, mirror with copy.
 * The _dev form takes device pointers (d_weights_or_null: n_sets int64; d_matrix: C x C int64, every entry is written;
 * the workspace of sbwtgpu_colorsets_shared_workspace_bytes(s) bytes, 256-byte aligned), is asynchronous on `stream` and
 * never synchronises.  It cannot report an out-of-range weight through its return value: the first 64-bit word of the
 * workspace is a status word, all ones when every weight was in range, otherwise the smallest offending set -- such a
 * weight was taken as 0, and the matrix is not to be used.  Read it after the stream has finished.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL s or output; a weight that is negative or
 * above 2^31 - 1 (checked on the device; the message names the smallest offending set); a workspace that is too small.
 * Scratch of the host form, released before it returns: the matrix (8 C^2 bytes), the weights when given (8 n_sets), and
 * the workspace: with S = n_sets and P = C, both rounded up to 64, 21 S + S P / 8 + 8 P^2 bytes and the radix sort's
 * storage on the matrix-core route, 4 S on the plain route.  SBWTGPU_ERR_OOM leaves index and object usable.
 * Thread-safe on one object: a call owns its stream and its scratch. */
int     sbwtgpu_colorsets_set_sizes(const sbwtgpu_colorsets *s, int64_t *sizes_out /* n_sets */);
typedef struct { int64_t n_sets_used; int32_t n_colors, words, used_mfma, n_limbs; double pass_ms[4]; } sbwtgpu_shared_info;
int     sbwtgpu_colorsets_shared_kmers(const sbwtgpu_colorsets *s, const int64_t *weights_or_null /* n_sets */,
                                       int64_t *matrix_out /* n_colors x n_colors */, sbwtgpu_shared_info *info_or_null);
int64_t sbwtgpu_colorsets_shared_workspace_bytes(const sbwtgpu_colorsets *s);
int     sbwtgpu_colorsets_shared_kmers_dev(const sbwtgpu_colorsets *s, const int64_t *d_weights_or_null, int64_t *d_matrix,
                                           void *d_workspace, int64_t workspace_bytes, void *stream);

/* ---- colour select: the k-mers whose colour set satisfies a predicate, as an index ----
 * The core k-mers of a clade, the k-mers unique to one strain, the accessory k-mers, the k-mers held by at least p of n
 * references: each is a sub-index of a coloured index.  sbwtgpu_index_setop cannot give them, for it needs one index per
 * reference, and the colours exist so that those indexes need not.
 * Inputs: a colour-set object s of an index, with C = n_colors and W = ceil(C / 64) words per row, and a predicate
 * P = (include, exclude, min_in, max_in).  include and exclude are W-word masks, bit c at bit c & 63 of word c >> 6 as
 * everywhere else; exclude_or_null = NULL means all zero.
 *   - A row MATCHES exactly when (row & exclude) == 0 and min_in <= popcount(row & include) <= max_in.  Integer arithmetic,
 *     no floating point.
 *   - A real column j is SELECTED exactly when table[ids[j]] matches.  Row 0, the empty set, is judged like any other row:
 *     min_in = 0 therefore selects uncoloured real columns.  Dummy columns are never selected: they have no key.
 *   - The verdict depends on what the object MEANS: an uploaded object with duplicate or unused rows selects the same k-mers
 *     as its canonical form.
 *   - The RESULT is bit for bit what sbwtgpu_build_plain_matrix returns for the selected k-mers given as sequences of length
 *     k with add_revcomp = 0 -- rows, marks, n_nodes and n_kmers (the contract of sbwtgpu_index_setop).  An empty selection
 *     gives the root column alone.  Two calls give identical bytes.
 * The common cases:   core of a group g       include g,   exclude none,                   min_in |g|, max_in >= |g|
 *                     unique to g             include g,   exclude the complement within C, min_in 1,   max_in any
 *                     accessory               include all, exclude none,                   min_in 1,   max_in C - 1
 *                     soft core (p of g)      include g,   exclude none,                   min_in p,   max_in any
 * Example, k = 3, colour 0 = AACCG, colour 1 = CCGGTT: AAC and ACC carry {0}, CCG carries {0, 1}, CGG, GGT and GTT carry {1}.
 * include {0, 1}, min 2 gives {CCG}; include {0}, exclude {1}, min 1 gives {AAC, ACC}; include {0, 1}, min 1, max 1 gives
 * {AAC, ACC, CGG, GGT, GTT}; include {0, 1}, min 0, max 0 gives {} as nothing is uncoloured.
 * sbwtgpu_colorsets_match_sets gives the verdict per table row, match_out[t] = 1 or 0 for t < n_sets (a coloured-unitig
 * FASTA is filtered by header with it).  sbwtgpu_colorsets_select_counts gives the counts without building;
 * sbwtgpu_colorsets_select builds.
 * sbwtgpu_color_select_info: n_real = the real columns of the index; n_selected; n_sets_matched = the distinct rows that
 * match and that at least one real column carries (rows by content: the number for the canonical form); n_nopred = the
 * selected k-mers without a predecessor among them (select only; 0 from select_counts); pass_ms on the host clock: keys;
 * verdicts, flags and select; builder tail and columns (0 from select_counts).
 * Colours of the result need no call of their own: make an index v from the bits and call
 * sbwtgpu_colorsets_merge(v, s, NULL, 0, ...).
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL s, p, include or output; a bit at or above
 * n_colors in either mask; min_in < 0 or max_in < min_in (a min_in above popcount(include) is legal and selects nothing);
 * an object used with another index; and, for the two select calls, what the set operations refuse: k outside 2 .. 64, a
 * rank-only index, the column limit.
 * The builder's dummy limit applies unchanged: n_nopred x k > 2^26 is SBWTGPU_ERR_OOM with the counts still in info.
 * Selections are fragmented sets and reach this limit sooner than genomes do: dump the unitigs and use the host builder.
 * Scratch, all released before the call returns: the set operations' 37 / 69 bytes per column (k <= 32 / k <= 64) while
 * the keys are extracted, 12 / 20 bytes per k-mer for keys and columns, 6 bytes per set, 1 byte per k-mer for the flags,
 * 8 / 16 bytes per selected k-mer, then the builder tail's.  When more than one non-empty row matches, also 4 + 8 W bytes
 * per such row and about 17 more while they are compared by content.  SBWTGPU_ERR_OOM leaves index and object usable.
 * Thread-safe on immutable handles: every call owns its stream and its scratch. */
typedef struct { const uint64_t *include; const uint64_t *exclude_or_null; int32_t min_in, max_in; } sbwtgpu_color_predicate;
typedef struct { int64_t n_real, n_selected, n_sets_matched, n_nopred; double pass_ms[3]; } sbwtgpu_color_select_info;
int  sbwtgpu_colorsets_match_sets(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, uint8_t *match_out /* n_sets */);
int  sbwtgpu_colorsets_select_counts(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, sbwtgpu_color_select_info *info);
int  sbwtgpu_colorsets_select(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, int build_streaming_support,
                              sbwtgpu_plain_matrix_bits *out, sbwtgpu_color_select_info *info /* may be NULL */);

/* ---- screen: which references are in a read set, and how much of each ----
 * The sample-level counterpart of the per-read hit profiles and of the shared k-mers: per reference the number of its
 * k-mers, how many distinct ones the sample contains (breadth: the exact containment) and how many of the sample's windows
 * fall on it (depth).  A screen object is an accumulator on the device that lives across batches.
 * Inputs: a colour-set object s of an index of n columns, with n_sets, ids, table, C = n_colors and W words per row, and
 * batches of reads in the form sbwtgpu_read_hits_* takes them.
 * The sample M is the multiset of the windows of all reads added so far.  A window counts under the rule of
 * sbwtgpu_search_batch: a byte other than upper-case A/C/G/T in it means no hit.  With strands = 2, M also holds the
 * reverse complement of every window (the complement rule of the read-hit profiles): a window is then two occurrences, and
 * a palindromic window two occurrences of one k-mer.  A window whose search result is >= 0 is one HIT on that column; with
 * two strands each of its two k-mers is.  The object holds
 *   - n_windows, the size of M, misses counted (strands = 2: twice the windows);
 *   - n_hits, the number of hits;
 *   - seen, one bit per column: bit v is set when column v has a hit.  uint64 words, bit v % 64 of word v / 64; n_seen is
 *     its popcount;
 *   - set_hits[t], int64[n_sets]: the hits on columns with ids[v] = t.  Set 0, the empty set, is counted like any other;
 *     the entries sum to n_hits.
 * Derived on demand -- the object stays usable, and more batches may follow:
 *   - set_kmers[t] = size[t] of sbwtgpu_colorsets_set_sizes (size[0] includes the dummy columns);
 *   - set_seen[t] = #{ v : ids[v] = t and seen[v] }; the entries sum to n_seen;
 *   - per colour c and X one of kmers, seen, hits: ref_X[c] = the sum of set_X[t] over the sets t >= 1 whose row has bit c.
 *     ref_kmers[c] is the number of index k-mers of reference c (the diagonal of the shared matrix), ref_seen[c] /
 *     ref_kmers[c] the containment of c in the sample, ref_hits[c] / ref_kmers[c] its mean k-mer depth.
 * Everything is exact int64; there is no floating point anywhere.  The state is a function of the index, of what the
 * object s MEANS and of the multiset of reads added: it does not depend on batch boundaries, chunking, tuning, image level,
 * stream, or the order of concurrent adds.  For an uploaded s with duplicate rows or another numbering the per-set vectors
 * follow its ids, the per-colour vectors are those of its canonical form.
 * sbwtgpu_screen_create allocates n / 8 + 8 n_sets bytes and a few words, zeroed; s and its index must outlive the object.
 * sbwtgpu_screen_reset zeroes it again (it waits for the device first).
 * sbwtgpu_screen_add_dev takes device pointers with the preconditions of sbwtgpu_read_hits_dev, is asynchronous on `stream`,
 * never synchronises and never allocates.  Its workspace, of sbwtgpu_screen_workspace_bytes (non-decreasing in total_bases
 * and n_reads), is 16-byte aligned and begins with the search workspace: sbwtgpu_workspace_status on it reports the
 * search's status word.  After the searches (the forward batch and, for two strands, the mirrored batch of the read-hit
 * profiles; int32 results: colour sets exist below 2^31 columns only) one kernel launch feeds the accumulator.
 * sbwtgpu_screen_add_batch takes host buffers and cuts the batch into chunks of whole reads of at most
 * "screen_chunk_bases" bases (sbwtgpu_set_tuning; 0 = the default of 64 Mi; a chunk always takes one read), two in flight.
 * Only bases and offsets go to the device; nothing but each chunk's status word comes back.
 * sbwtgpu_screen_info, _sets, _colors and _seen_copy run on a stream of the object's own; they see every add that has
 * returned from sbwtgpu_screen_add_batch, which finishes its streams before it returns.  A caller of sbwtgpu_screen_add_dev
 * on a stream of their own finishes that stream first.  They leave the object unchanged; any output may be NULL.
 * sbwtgpu_screen_seen_dev gives the bitmap in place: ceil(n / 64) words that live as long as x.
 * Adds from several host threads or streams on one object are safe -- the object is built on atomics -- as long as each
 * caller brings a workspace of its own; the queries serialise on the object.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL arguments; strands not 1 or 2; n_reads < 0
 * or >= 2^31; a workspace that is too small; and what the colour-set queries refuse for the object's index.  A read of 2^31
 * bases or more: SBWTGPU_ERR_READ_TOO_LONG.  SBWTGPU_ERR_OOM leaves index and colour sets usable and nothing allocated.
 * Scratch of _sets and _colors, released before they return: 16 n_sets + 24 C bytes. */
typedef struct sbwtgpu_screen sbwtgpu_screen;
int     sbwtgpu_screen_create(const sbwtgpu_colorsets *s, sbwtgpu_screen **out);
int     sbwtgpu_screen_reset(sbwtgpu_screen *x);
void    sbwtgpu_screen_destroy(sbwtgpu_screen *x);
int64_t sbwtgpu_screen_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands);
int     sbwtgpu_screen_add_dev(sbwtgpu_screen *x, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                               int64_t n_reads, int strands, void *d_workspace, int64_t workspace_bytes, void *stream);
int     sbwtgpu_screen_add_batch(sbwtgpu_screen *x, const char *bases, const int64_t *read_off, int64_t n_reads, int strands);
int     sbwtgpu_screen_info(const sbwtgpu_screen *x, int64_t *n_windows, int64_t *n_hits, int64_t *n_seen, int64_t *n_sets,
                            int32_t *n_colors);
int     sbwtgpu_screen_sets(const sbwtgpu_screen *x, int64_t *set_kmers, int64_t *set_seen, int64_t *set_hits /* n_sets each */);
int     sbwtgpu_screen_colors(const sbwtgpu_screen *x, int64_t *ref_kmers, int64_t *ref_seen, int64_t *ref_hits /* n_colors each */);
int     sbwtgpu_screen_seen_dev(const sbwtgpu_screen *x, const uint64_t **d_seen);
int     sbwtgpu_screen_seen_copy(const sbwtgpu_screen *x, uint64_t *seen /* ceil(n / 64) */);

/* ---- bubbles: where the references differ, and which reference carries which allele ----
 * Variant sites of the PLAIN unitig graph: a handle u of sbwtgpu_unitigs_create_graph(idx, NULL, flags, ...) with
 * SBWTGPU_UNITIGS_LINKS.  The terms unitig, link, link_off, link_to, column map, real column and S(v) (the colour row of
 * column v, table[ids[v]]) are those of the sections on unitigs, coloured unitigs and the unitig graph.  In the plain graph a
 * unitig with one in-link and one out-link is never followed by another such unitig (that edge would be internal), so every
 * branch of a bubble is one unitig.  A coloured handle cuts branches at colour breaks and is refused: pass the plain handle
 * plus the colour-set object.
 *   in-degree       of unitig j: the number of entries of link_to equal to j.
 *   out-degree      of unitig i: link_off[i+1] - link_off[i].
 *   bubble          four unitigs (s, a, b, t) with: outdeg(s) = 2 and its links in CSR order are a, b (a is reached by the
 *                   smaller edge character; a != b); indeg(a) = indeg(b) = 1 and outdeg(a) = outdeg(b) = 1; the link of a
 *                   and the link of b go to the same unitig t, and indeg(t) = 2; a, b are neither s nor t.  s = t is
 *                   allowed: a bubble on a cycle, and it is reported.
 *   no bubble       deliberately: sites with three or four branches; a branch that is an edge s -> t with no unitig on it
 *                   (a deletion against the other branch); nested structures (superbubbles); tips.
 *   n_kmers[j]      the k-mers of branch[j]: its length - k + 1.
 *   kind            SBWTGPU_BUBBLE_SNP when n_kmers[0] = n_kmers[1] = k (both paths add k + 1 characters of which the last k
 *                   spell t's first k-mer: one free character, a single-base substitution), else SBWTGPU_BUBBLE_OTHER.
 *   allele          of branch j: the last n_kmers[j] characters of its spelling (what its k-mers add); for an SNP the variant
 *                   base is allele[0].  The caller cuts them from sbwtgpu_unitigs_copy's bases.
 *   order           records ascend by source.  The result is a function of the index alone and, with colours, of the matrix
 *                   the object means: byte-identical between runs, image levels, layouts, and marks given or derived.
 *   branch colours  with a colour-set object s of W-word rows (and SBWTGPU_UNITIGS_COLUMN_MAP on the handle), two rows for
 *                   branch j of bubble i at uint64[(2 i + j) W + w]: inter = AND of S(v) over the columns v of unitig
 *                   branch[j] (the references that hold the whole allele), uni = OR over the same columns (those that hold
 *                   any of its k-mers).  An object with duplicate rows or another numbering gives the same rows; bits at or
 *                   above n_colors are 0.
 *   strands         the graph is directed: on an index that holds reverse complements every bubble appears twice, once per
 *                   strand, with s and t swapped and the alleles reverse-complemented (the convention of
 *                   sbwtgpu_unitigs_create).  Pairing them is left to the caller.
 * sbwtgpu_bubbles_create runs on a stream of its own (in-degrees, detection, a scan, a fill, and with s one pass over the
 * column map), with 24 bytes of scratch per unitig that it frees before it returns; the result takes 32 n_bubbles bytes and
 * with colours 32 W n_bubbles more.  Nothing proportional to the number of columns is allocated.  Zero unitigs or zero links
 * give zero bubbles and success.  _info: n_colors = words = 0 without an object; n_bubbles must not be NULL, the others may.
 * _dev: d_rec must not be NULL; the pointers are NULL where there is nothing (no bubble; rows without an object) and live
 * as long as b.  _copy: rec may be NULL when there is no bubble, inter / uni when there is no bubble or no object.
 * sbwtgpu_bubbles_in_degrees_copy is the first pass alone.  The handle, the object and the index stay unchanged, and b
 * holds no reference to them: they may be destroyed before b.  The calls are thread-safe on immutable handles.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL u or out; a handle made without
 * SBWTGPU_UNITIGS_LINKS; a coloured handle; an object given with a handle made without SBWTGPU_UNITIGS_COLUMN_MAP; an object
 * whose index has another number of columns or another k than the handle's; NULL outputs where a value exists.
 * SBWTGPU_ERR_OOM leaves the handle, the object and the index usable and nothing allocated. */
#define SBWTGPU_BUBBLE_OTHER 0u
#define SBWTGPU_BUBBLE_SNP   1u
typedef struct { uint32_t source, branch[2], sink, n_kmers[2], kind, reserved /* 0 */; } sbwtgpu_bubble;   /* 32 bytes */
typedef struct sbwtgpu_bubbles sbwtgpu_bubbles;
int  sbwtgpu_bubbles_create(const sbwtgpu_unitigs *u, const sbwtgpu_colorsets *s_or_null, sbwtgpu_bubbles **out);
int  sbwtgpu_bubbles_info  (const sbwtgpu_bubbles *b, int64_t *n_bubbles, int64_t *n_snps, int32_t *n_colors, int32_t *words);
int  sbwtgpu_bubbles_dev   (const sbwtgpu_bubbles *b, const sbwtgpu_bubble **d_rec, const uint64_t **d_inter, const uint64_t **d_union);
int  sbwtgpu_bubbles_copy  (const sbwtgpu_bubbles *b, sbwtgpu_bubble *rec, uint64_t *inter, uint64_t *uni);
/* pass 1 alone: indeg[n_unitigs] (may be NULL when there is no unitig) */
int  sbwtgpu_bubbles_in_degrees_copy(const sbwtgpu_unitigs *u, uint32_t *indeg);
/* measurement aid (tools/bubbles_bench.py): device-event times in ms of in-degrees, detect, compact, branch colours */
int  sbwtgpu_bubbles_stats (const sbwtgpu_bubbles *b, double pass_ms[4]);
void sbwtgpu_bubbles_destroy(sbwtgpu_bubbles *b);

/* ---- genotype: which allele of every bubble a read set carries ----
 * The sample-level counterpart of the bubbles: per allele the k-mer depth of a read set, per bubble a call, per reference
 * how often the sample follows it where the references differ.  A genotype object is an accumulator on the device that
 * lives across batches, like a screen object.
 * Inputs
 *   - idx: an index.
 *   - u: a plain graph handle made from idx with SBWTGPU_UNITIGS_LINKS | SBWTGPU_UNITIGS_COLUMN_MAP.
 *   - b: a bubbles object made from u, with or without colours.
 * Slots and branch columns
 *   - Slot s = 2i + j is branch j of bubble i.
 *   - A branch column is a real column v whose col_unitig[v] is branch[j] of some bubble.
 *   - A branch belongs to exactly one bubble, so its slot is unique.
 *   - branch_off[s] is the exclusive prefix sum of n_kmers in slot order.  P = branch_off[2B] is the total.
 *   - Branch column v has position p = branch_off[s] + col_offset[v].
 * State
 *   The state is exact uint64 / int64 and uses no floating point anywhere.
 *   - kmer_hits[p], for p in [0, P).
 *   - Three scalars: n_windows, n_hits and n_site_hits.
 * What one add does
 *   An add takes reads and strands in {1, 2}.
 *   1. Every window is searched by the rule of sbwtgpu_search_batch: upper-case ACGT only.
 *   2. With strands = 2, the mirrored batch of Screen / read-hits is searched too.
 *   3. Every hit on a branch column adds 1 to that column's kmer_hits.  It is counted in n_site_hits.
 *   4. Every hit anywhere is counted in n_hits.
 *   5. Every window is counted in n_windows, once per strand searched, as Screen counts them.
 *   6. Hits on sources, sinks and every other unitig change nothing else.
 * Determinism
 *   The state is a function of the index and of the multiset of reads and strands added.  It does not depend on batch
 *   boundaries, chunking, tuning, image level, streams or the order of concurrent adds.
 * Derived on demand
 *   The object stays usable afterwards.  All values are int64 and each vector has 2B entries.
 *   - seen[s] = #{ p in branch s : kmer_hits[p] > 0 }.
 *   - hits[s] = the sum of kmer_hits over branch s.
 *   - min_hits[s] = the minimum of kmer_hits over branch s.
 * Calls
 *   The parameters are breadth_ppm in [1, 10^6] and min_depth >= 0.
 *   - Allele j of bubble i is present when both conditions hold, in 64-bit integers:
 *       seen[s] * 10^6 >= breadth_ppm * n_kmers[s];
 *       hits[s] >= min_depth * n_kmers[s]   (evaluated as hits[s] / n_kmers[s] >= min_depth, which no min_depth overflows).
 *   - call[i] is a uint8: bit 0 = allele a present, bit 1 = allele b present.  So 0 is no call, 1 is a, 2 is b and 3 is both.
 * Per colour
 *   The colour vectors exist only when b was made with a colour-set object.  The genotype object copies b's inter rows at
 *   create.
 *   - Colour c is informative at bubble i when bit c is set in exactly one of inter[2i], inter[2i+1].  Call that allele j_c.
 *   - ref_sites[c] = the informative bubbles with call != 0.
 *   - ref_match[c] = those whose call has bit j_c set.
 *   - ref_only[c] = those whose call equals 1 << j_c.
 *   - All three vectors are int64[n_colors].
 *   - ref_only[c] / ref_sites[c] answers "which reference does the sample follow where the references differ".
 * Strands
 *   On an index with reverse complements every bubble exists twice (section 24), and each twin keeps its own counters.
 *   Pairing the twins stays out of scope.
 * sbwtgpu_genotype_create allocates 8 P bytes of state and a few words, zeroed, and beside them what the adds read: n / 8
 * bytes of branch bitmap, n / 16 of rank directory, 4 P of positions, 16 B of branch_off and, with colours, 16 W B of inter
 * rows.  It runs three streaming passes and two scans on a stream of the object's own, with scratch (4 bytes per unitig, 16
 * per slot, 16 per 64 columns) that it frees before it returns.  It keeps references to idx and u, which must outlive g,
 * and none to b: it copies what it needs, and b may be destroyed before the first add.  B = 0 gives a valid object with
 * empty outputs.  sbwtgpu_genotype_reset zeroes the state again (it waits for the device first).
 * sbwtgpu_genotype_add_dev takes device pointers with the preconditions of sbwtgpu_read_hits_dev, is asynchronous on
 * `stream`, never synchronises and never allocates.  Its workspace, of sbwtgpu_genotype_workspace_bytes (non-decreasing in
 * total_bases and n_reads), is 16-byte aligned and begins with the search workspace: sbwtgpu_workspace_status on it reports
 * the search's status word.  After the searches (the forward batch and, for two strands, the mirrored batch of the read-hit
 * profiles; int32 results) one kernel launch feeds the accumulator.
 * sbwtgpu_genotype_add_batch takes host buffers and cuts the batch into chunks of whole reads of at most
 * "genotype_chunk_bases" bases (sbwtgpu_set_tuning; 0 = the default of 64 Mi; a chunk always takes one read), two in flight.
 * Only bases and offsets go to the device; nothing but each chunk's status word comes back.
 * sbwtgpu_genotype_info, _branches, _kmer_hits_copy and _calls run on a stream of the object's own; they see every add that
 * has returned from sbwtgpu_genotype_add_batch, which finishes its streams before it returns.  A caller of
 * sbwtgpu_genotype_add_dev on a stream of their own finishes that stream first.  They leave the object unchanged; any output
 * may be NULL.
 * Adds from several host threads or streams on one object are safe -- the object is built on atomics -- as long as each
 * caller brings a workspace of its own; the queries serialise on the object.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL arguments; a coloured handle; a handle without
 * links, or without the column map; a handle whose n_nodes or k differ from the index's; a b that does not fit u (a record
 * names a unitig >= n_unitigs, or its n_kmers is not that unitig's k-mer count, or two slots name one unitig; checked on the
 * device while the slot table is filled); an index of 2^31 columns or more; a rank-only index; strands not 1 or 2; n_reads
 * < 0 or >= 2^31; a workspace that is too small; breadth_ppm or min_depth out of range; colour outputs asked of an object
 * made from a colourless b.  A b made from a handle of ANOTHER index is refused by the same check; where its record indices
 * and k-mer counts happen to fit u's unitigs this is not detectable, and the object then counts at those unitigs.
 * A read of 2^31 bases or more: SBWTGPU_ERR_READ_TOO_LONG.  SBWTGPU_ERR_OOM leaves everything usable and nothing allocated.
 * Scratch of _branches and _calls, released before they return: 48 B + 24 n_colors bytes at the most. */
typedef struct sbwtgpu_genotype sbwtgpu_genotype;
int     sbwtgpu_genotype_create(const sbwtgpu_index *idx, const sbwtgpu_unitigs *u, const sbwtgpu_bubbles *b, sbwtgpu_genotype **out);
int     sbwtgpu_genotype_reset(sbwtgpu_genotype *g);
void    sbwtgpu_genotype_destroy(sbwtgpu_genotype *g);
int64_t sbwtgpu_genotype_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands);
int     sbwtgpu_genotype_add_dev(sbwtgpu_genotype *g, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                 int64_t n_reads, int strands, void *d_workspace, int64_t workspace_bytes, void *stream);
int     sbwtgpu_genotype_add_batch(sbwtgpu_genotype *g, const char *bases, const int64_t *read_off, int64_t n_reads, int strands);
int     sbwtgpu_genotype_info(const sbwtgpu_genotype *g, int64_t *n_bubbles, int64_t *n_branch_kmers /* P */, int64_t *n_windows,
                              int64_t *n_hits, int64_t *n_site_hits, int32_t *n_colors);
int     sbwtgpu_genotype_branches(const sbwtgpu_genotype *g, int64_t *seen, int64_t *hits, int64_t *min_hits /* 2 B each */);
int     sbwtgpu_genotype_kmer_hits_copy(const sbwtgpu_genotype *g, int64_t *branch_off /* 2 B + 1 */, uint64_t *kmer_hits /* P */);
int     sbwtgpu_genotype_calls(const sbwtgpu_genotype *g, int32_t breadth_ppm, int64_t min_depth, uint8_t *call /* B */,
                               int64_t *ref_sites, int64_t *ref_match, int64_t *ref_only /* n_colors each, or NULL */);

/* ---- positions: where on a reference a k-mer lies, and where a read maps ----
 * One table, holding for every column the smallest reference coordinate at which its k-mer occurs, and one read-side call,
 * which for every read finds the reference placement that most of its k-mers agree on: seed-and-vote mapping on the diagonal
 * ref_pos - read_pos.  Everything is exact integers.  There is no floating point anywhere.
 * The position table
 *   A sbwtgpu_positions object is bound to one index of n columns and its k.  The index must have n < 2^31 and must not be
 *   rank-only.
 *   It holds first[v], one uint64 per column.  UINT64_MAX means "no position".
 *   - Sequence numbers.  The caller numbers the reference sequences.  An add of n_reads sequences with first_seq gives
 *     sequence i of the batch the number first_seq + i.  Numbers must be in 0 ... 2^30 - 1.
 *   - Window and strand flag.  A window of sequence q at 0-based offset pos is x = q[pos .. pos+k).  It follows the rule of
 *     sbwtgpu_search_batch: upper-case ACGT only.
 *     - If the search of x gives column v >= 0, the key (seq << 32) | (pos << 1) | 0 is offered to first[v].
 *     - With strands = 2, the search of the reverse complement of x gives v' >= 0, and the key with low bit 1 is offered to
 *       first[v'].  The complement rule is that of the read-hit profiles.
 *     - first[v] is the minimum of the keys offered.  The low bit t says that the column's k-mer is the reverse complement of
 *       the reference window at pos.
 *     - A palindromic window offers both keys to one column.  The minimum keeps t = 0.
 *   - State.  The state is a function of the index and of the set of (sequence number, sequence, strands) triples added.  It
 *     does not depend on batch boundaries, chunking, the order of adds, concurrent adds from several host threads, tuning,
 *     image level or streams.
 *     - Adding one sequence twice under the same number changes nothing.
 *     - Adding it under two numbers leaves the smaller.
 *   - Scalars.  These are exact int64:
 *     - n_windows: windows offered, once per strand searched;
 *     - n_hits;
 *     - n_positioned: the number of columns with a position, derived on demand.
 * Mapping a read
 *   The read has W windows.  Window i, 0-based on the read as given, is searched as x.  With strands = 2 it is also searched
 *   as rc(x), in the mirrored batch.  A result >= 0 is a hit (i, s) on column v, with s = 0 for the first search and s = 1 for
 *   the second.  A hit whose first[v] is a position (seq, pos, t) is anchored.
 *   An anchored hit votes for the placement (seq, o, start):
 *   - o = s XOR t;
 *   - start = pos - i if o = 0;
 *   - start = pos - (W - 1 - i) if o = 1.
 *   start is the reference coordinate of the read's leftmost base when the read lies on the reference in orientation o.  It
 *   is signed and may be negative.
 *   The record per read is 32 bytes (sbwtgpu_read_map):
 *   - (seq, strand = o, start) is the placement with the most votes.  Ties go to the lexicographically smallest
 *     (seq, o, start), with start compared as signed.
 *   - votes is the winner's count.
 *   - votes2 is the largest count among all other placements, and 0 if there is none.
 *   - n_found is the number of hits over the strands searched.  It equals n_found of sbwtgpu_read_hits_* only with one strand.
 *   - n_anchored is the number of anchored hits.
 *   - With n_anchored = 0 the record is {0, -1, 0, 0, 0, n_found, 0}.
 *   first keeps only the smallest occurrence.  A k-mer that several references share therefore votes for the one with the
 *   smallest number.  This is a projection onto the first reference that holds each k-mer, not an enumeration of all
 *   occurrences.
 * sbwtgpu_positions_create allocates 8 n bytes and a few words, every entry "no position"; idx must outlive the object.
 * sbwtgpu_positions_reset empties it again (it waits for the device first).  sbwtgpu_positions_upload makes an object from a
 * copied table; it refuses, on the device, any entry that is neither UINT64_MAX nor a key with seq < 2^30 (n_windows and n_hits
 * of an uploaded object are 0).
 * sbwtgpu_positions_add_batch takes host buffers and cuts the batch into chunks of whole sequences of at most
 * "positions_chunk_bases" bases (sbwtgpu_set_tuning; 0 = the default of 64 Mi; a chunk always takes one whole sequence), two
 * in flight.  After the searches one kernel runs over the results, one lane per result: it finds each result's sequence and
 * offset from the window offsets by bisection and issues one 64-bit atomic minimum per hit, and none when the value already
 * there is smaller.  *n_windows: the windows of the batch; *n_hit_windows: those with a hit on either strand (both may be NULL).
 * sbwtgpu_positions_info: any output may be NULL; device_bytes is what the object holds on the device.
 * sbwtgpu_positions_first_copy copies first (n entries); sbwtgpu_positions_first_dev gives it in place, alive as long as p.
 * sbwtgpu_positions_map_dev takes device pointers with the preconditions of sbwtgpu_read_hits_dev and writes n_reads records
 * to d_out.  It is asynchronous on `stream`, never synchronises and never allocates.  Its workspace, of
 * sbwtgpu_positions_map_workspace_bytes (non-decreasing in total_bases and n_reads), is 16-byte aligned and begins with the
 * search workspace: sbwtgpu_workspace_status on it reports the search's status word.  After the searches two kernels run: one
 * wave per read with a table of SBWTGPU_POSITIONS_MAP_TABLE distinct placements in LDS, and a second one, always launched,
 * that recomputes exactly the reads whose placements outgrew that table.  Every read gets the exact record.  The second
 * kernel gives a listed read one wave and compares every window's key with every other's: its time is quadratic in the read's
 * WINDOWS (times the strands), about W^2 / 64 gather trips, whatever share of them hit.  That is meant for the odd junk read
 * among short reads.  A long read that leaves the diagonal often -- a 100 kb read with indels, a contig -- has more than
 * SBWTGPU_POSITIONS_MAP_TABLE placements, takes this path and holds its stream for a long time (10^5 windows: some 10^8
 * trips of one wave): such reads are outside the intended use; cut them into pieces of a few thousand bases and map those.
 * sbwtgpu_positions_map_batch is the same call on host buffers, chunked like the adds; out holds n_reads records.
 * info, first_copy and reset serialise on the object and see every add that has returned.  Adds from several host threads on
 * one object are safe: the table is built on atomic minima.  The map calls only read the object.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL arguments; a rank-only index; an index of 2^31
 * columns or more; strands not 1 or 2; n_reads < 0 or >= 2^31; first_seq < 0 or first_seq + n_reads > 2^30; a workspace that
 * is too small; an object used after its index changed.  A read of 2^30 bases or more in the map calls gives
 * SBWTGPU_ERR_READ_TOO_LONG, so the int32 counts cannot overflow with two strands, and a sequence of 2^31 bases or more in an
 * add likewise.  sbwtgpu_positions_map_batch checks every read's length from the offsets.  sbwtgpu_positions_map_dev cannot
 * see the lengths: it refuses only a batch of ONE read of 2^30 bases or more.  In a larger batch the lengths are the caller's
 * to keep below 2^30: the record of a longer read is UNDEFINED (its start and its counts wrap); no memory outside the
 * caller's buffers is read or written, and the records of the other reads are what they should be.  SBWTGPU_ERR_OOM leaves the index usable and nothing allocated. */
#define SBWTGPU_POSITIONS_MAP_TABLE 256
typedef struct { int64_t start; int32_t seq; int32_t strand; int32_t votes; int32_t votes2; int32_t n_found; int32_t n_anchored; } sbwtgpu_read_map;
typedef struct sbwtgpu_positions sbwtgpu_positions;
int     sbwtgpu_positions_create(const sbwtgpu_index *idx, sbwtgpu_positions **out);
int     sbwtgpu_positions_upload(const sbwtgpu_index *idx, const uint64_t *first /* n */, sbwtgpu_positions **out);
int     sbwtgpu_positions_reset(sbwtgpu_positions *p);
void    sbwtgpu_positions_destroy(sbwtgpu_positions *p);
int     sbwtgpu_positions_add_batch(sbwtgpu_positions *p, int64_t first_seq, const char *bases, const int64_t *read_off,
                                    int64_t n_reads, int strands, int64_t *n_windows, int64_t *n_hit_windows);
int     sbwtgpu_positions_info(const sbwtgpu_positions *p, int64_t *n_columns, int64_t *k, int64_t *n_windows, int64_t *n_hits,
                               int64_t *n_positioned, int64_t *device_bytes);
int     sbwtgpu_positions_first_copy(const sbwtgpu_positions *p, uint64_t *first /* n */);
int     sbwtgpu_positions_first_dev(const sbwtgpu_positions *p, const uint64_t **d_first);
int64_t sbwtgpu_positions_map_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands);
int     sbwtgpu_positions_map_dev(const sbwtgpu_positions *p, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                  int64_t n_reads, int strands, sbwtgpu_read_map *d_out, void *d_workspace,
                                  int64_t workspace_bytes, void *stream);
int     sbwtgpu_positions_map_batch(const sbwtgpu_positions *p, const char *bases, const int64_t *read_off, int64_t n_reads,
                                    int strands, sbwtgpu_read_map *out);

/* ---- occurrences: EVERY place on the references where a k-mer lies, and reads mapped by all of them ----
 * The positions object above keeps one coordinate per column.  This object keeps all of them, as CSR arrays, and its map call
 * votes with all of them: a read lands on the reference it fits best, and an equally good placement shows as votes2 == votes.
 * Everything is exact integers.
 * The occurrence table
 *   A sbwtgpu_occurrences object is bound to one index of n columns and its k.  The index must have n < 2^31 and must not be
 *   rank-only.
 *   - It holds off[0..n] as uint64, with off[0] = 0, non-decreasing and off[n] = N.
 *   - It holds occ[0..N) as uint64, the keys of "positions": (seq << 32) | (pos << 1) | t.  Within a column they are strictly
 *     ascending, so they are distinct.
 *   - occ[off[v] .. off[v+1]) is exactly the set of keys that the rules of "positions" OFFER to first[v], over all
 *     (number, sequence, strands) triples added.  The rules are the same: the window x = q[pos .. pos+k), upper-case ACGT only,
 *     with strands = 2 the search of the reverse complement of x offers the key with t = 1 to its column v', the t bit says that
 *     the column's k-mer is the reverse complement of the reference window at pos.
 *   - Consequences:
 *     - occ[off[v]] == first[v] wherever the column has an occurrence.
 *     - A palindromic window with two strands leaves both keys, t = 0 and t = 1, in one column.
 *     - One sequence added twice under one number changes nothing.
 *     - One sequence added under two numbers leaves both.
 *     - The state is a function of the index and of the SET of triples.  It does not depend on batch boundaries, chunking,
 *       order, host threads, tuning, image level or streams.
 *   - Scalars, exact int64:
 *     - n_windows and n_hits, as in "positions" (0 for an uploaded object);
 *     - n_occurrences = N;
 *     - n_positioned, the columns with at least one occurrence;
 *     - max_count, the largest occurrence count of a column.
 * Building
 *   The sizes are unknown until every reference is seen, so the object comes from a builder.
 *   sbwtgpu_occurrences_builder_create starts one on idx, which must outlive the builder and the object.
 *   sbwtgpu_occurrences_builder_add_batch takes host buffers with the arguments of sbwtgpu_positions_add_batch.  It cuts the
 *   batch into chunks of whole sequences of at most "occurrences_chunk_bases" bases, two in flight.  After the searches one kernel
 *   runs over the results, one lane per result: it finds each result's sequence and offset by bisection and appends
 *   (column, key) to a log on the device, with one atomic per wave on the log's length.  Before a chunk is launched the log has
 *   room for what it holds plus the chunk's windows x strands; it grows by doubling (which waits for the device).  Adds from
 *   several host threads on one builder are safe: THEY ARE SERIALISED on the builder, one add runs at a time.
 *   sbwtgpu_occurrences_builder_finish sorts the log by (column, key) with two stable radix sorts, flags the first entry of each
 *   run of equal pairs, selects the flagged keys into occ, counts them per column and scans the counts into off.  On success it
 *   consumes the builder (the log is freed) and gives the object; on failure the builder is still the caller's to destroy.
 *   Device memory: a logged hit takes 12 bytes in the log, whose capacity is at most twice its length; finish needs another
 *   12 bytes per logged hit for the sort's second buffer, then (that buffer freed) 1 byte per logged hit of flags and 8 bytes per
 *   distinct occurrence: the peak is at most 36 bytes per logged hit, plus 8 (n + 1) bytes of off and rocPRIM's scratch.
 *   sbwtgpu_occurrences_builder_destroy frees an unfinished builder.
 * sbwtgpu_occurrences_upload makes an object from copied arrays (off: n + 1 entries, occ: n_occ).  It checks them on the
 * device: off[0] = 0, off non-decreasing, off[n] = n_occ, the keys of a column strictly ascending, seq < 2^30.  Its message
 * names the first (smallest) offending column.
 * sbwtgpu_occurrences_info: any output may be NULL; device_bytes is what the object holds on the device.
 * sbwtgpu_occurrences_offsets_copy / _keys_copy copy off (n + 1 entries) and occ (N entries); _offsets_dev / _keys_dev give
 * them in place, alive as long as the object.
 * sbwtgpu_occurrences_to_positions makes a positions object of the same index with first[v] = occ[off[v]], or "no position"
 * for an empty column: what the same adds give sbwtgpu_positions_add_batch.  Its n_windows and n_hits are 0.
 * Mapping a read with every occurrence
 *   It is the mapping of "positions" with one change.  A hit (i, s) on column v has c = off[v+1] - off[v] occurrences.
 *   - With c = 0 the hit is found and not anchored.
 *   - With c > max_occ the k-mer is repetitive.  The hit is found, casts no vote and is not anchored.
 *   - Otherwise the hit is anchored.  It casts ONE VOTE FOR EACH of its c occurrences (seq, pos, t): the placement
 *     (seq, o = s XOR t, start) with start = pos - i if o = 0 and start = pos - (W - 1 - i) if o = 1.
 *   Two occurrences of one k-mer never give the same placement: within one (seq, t) a distinct pos gives a distinct start, and
 *   a distinct t gives a distinct o.  So a hit votes at most once per placement.
 *   The record is sbwtgpu_read_map:
 *   - the winner (seq, strand = o, start) has the most votes, ties to the smallest (seq, o, start), start signed;
 *   - votes is its count; votes2 is the largest count among all other placements, 0 if there is none;
 *   - n_found is the hits over the strands searched;
 *   - n_anchored is the hits that voted, not the number of votes cast;
 *   - with n_anchored = 0 the record is {0, -1, 0, 0, 0, n_found, 0}.
 *   max_occ must be in 1 .. SBWTGPU_OCCURRENCES_MAX_OCC (2^20); anything else is refused.
 * sbwtgpu_occurrences_map_dev takes device pointers with the preconditions of sbwtgpu_positions_map_dev and writes n_reads
 * records to d_out.  It is asynchronous on `stream`, never synchronises and never allocates.  Its workspace, of
 * sbwtgpu_occurrences_map_workspace_bytes (non-decreasing in total_bases and n_reads), is 16-byte aligned and begins with the
 * search workspace: sbwtgpu_workspace_status on it reports the search's status word.  After the searches three kernels run.
 * The first gives a read one wave and keeps SBWTGPU_OCCURRENCES_MAP_TABLE distinct placements in LDS (256: at 12 bytes an entry
 * a block of four waves takes 12 KiB, so eight blocks, the CU's 32 waves, take 96 of its 160 KiB; 512 would cut the resident
 * waves to 24).  The second, always launched, recomputes exactly the reads whose placements outgrew the table: it enumerates
 * the read's votes again in P slices of the key space, a hash of the placement modulo P, only the current slice's placements
 * enter the table, and P doubles from 2 until every slice fits.  A slice that overflows ends its P at once, so the cost is
 * about P enumerations of the read's votes for the final P, which is a few times (distinct placements / table capacity), and
 * a part of an enumeration for every smaller P; the gathers of the re-enumerations stay in L2.  A read that no P up to 1024
 * fits goes to the third kernel, also always launched, which counts placement by placement in ascending order without a
 * table: one enumeration per distinct placement.  Together they terminate on every input, and every read gets the exact record.
 * sbwtgpu_occurrences_map_batch is the same call on host buffers, chunked like the adds; out holds n_reads records.
 * The map calls and the copies only read the object; they may run from several host threads.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL arguments; a rank-only index; an index of 2^31
 * columns or more; strands not 1 or 2; n_reads < 0 or >= 2^31; first_seq < 0 or first_seq + n_reads > 2^30; max_occ outside
 * 1 .. 2^20; a workspace that is too small; an object or builder used after its index changed.  A read of 2^30 bases or more
 * in the map calls gives SBWTGPU_ERR_READ_TOO_LONG, and a sequence of 2^31 bases or more in an add likewise; the lengths in
 * sbwtgpu_occurrences_map_dev are the caller's to keep below 2^30, as in sbwtgpu_positions_map_dev.  SBWTGPU_ERR_OOM leaves the
 * index usable and nothing allocated. */
#define SBWTGPU_OCCURRENCES_MAP_TABLE 256
#define SBWTGPU_OCCURRENCES_MAX_OCC (1 << 20)
typedef struct sbwtgpu_occurrences sbwtgpu_occurrences;
typedef struct sbwtgpu_occurrences_builder sbwtgpu_occurrences_builder;
int     sbwtgpu_occurrences_builder_create(const sbwtgpu_index *idx, sbwtgpu_occurrences_builder **out);
int     sbwtgpu_occurrences_builder_add_batch(sbwtgpu_occurrences_builder *b, int64_t first_seq, const char *bases,
                                              const int64_t *read_off, int64_t n_reads, int strands, int64_t *n_windows,
                                              int64_t *n_hit_windows);
int     sbwtgpu_occurrences_builder_finish(sbwtgpu_occurrences_builder *b, sbwtgpu_occurrences **out);
void    sbwtgpu_occurrences_builder_destroy(sbwtgpu_occurrences_builder *b);
int     sbwtgpu_occurrences_upload(const sbwtgpu_index *idx, const uint64_t *off /* n + 1 */, const uint64_t *occ /* n_occ */,
                                   int64_t n_occ, sbwtgpu_occurrences **out);
void    sbwtgpu_occurrences_destroy(sbwtgpu_occurrences *o);
int     sbwtgpu_occurrences_info(const sbwtgpu_occurrences *o, int64_t *n_columns, int64_t *k, int64_t *n_windows, int64_t *n_hits,
                                 int64_t *n_occurrences, int64_t *n_positioned, int64_t *max_count, int64_t *device_bytes);
int     sbwtgpu_occurrences_offsets_copy(const sbwtgpu_occurrences *o, uint64_t *off /* n + 1 */);
int     sbwtgpu_occurrences_keys_copy(const sbwtgpu_occurrences *o, uint64_t *occ /* n_occurrences */);
int     sbwtgpu_occurrences_offsets_dev(const sbwtgpu_occurrences *o, const uint64_t **d_off);
int     sbwtgpu_occurrences_keys_dev(const sbwtgpu_occurrences *o, const uint64_t **d_occ);
int     sbwtgpu_occurrences_to_positions(const sbwtgpu_occurrences *o, sbwtgpu_positions **out);
int64_t sbwtgpu_occurrences_map_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands);
int     sbwtgpu_occurrences_map_dev(const sbwtgpu_occurrences *o, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                    int64_t n_reads, int strands, int max_occ, sbwtgpu_read_map *d_out, void *d_workspace,
                                    int64_t workspace_bytes, void *stream);
int     sbwtgpu_occurrences_map_batch(const sbwtgpu_occurrences *o, const char *bases, const int64_t *read_off, int64_t n_reads,
                                      int strands, int max_occ, sbwtgpu_read_map *out);

/* ---- reference sequences and verification ----
 * The map calls above place a read by counting k-mer votes; their record is a hypothesis about a diagonal.  These calls look
 * at the bases: a packed copy of the reference sequences on the device, and one call that takes reads and their map records and
 * returns, per read, the mismatches on the voted diagonal and the best edit distance in a window around it.  They need no
 * index: they take reads, records and the reference object.  Everything is exact integers.
 * The reference object
 *   sbwtgpu_refseqs lives on one device and holds sequences numbered 0, 1, ... densely.
 *   sbwtgpu_refseqs_add_batch(r, first_seq, bases, read_off, n) appends n sequences.
 *   - first_seq must equal the number of sequences held so far.  Otherwise the call is refused and the message names both
 *     numbers.
 *   - The numbering rule is the one --positions-out and --occurrences-out use, so a record's seq indexes this object.
 *   - A base is valid if it is one of upper-case A C G T.  Every other byte (lower case, N, NUL) is stored as "invalid" and
 *     matches nothing, not even itself.
 *   Layout:
 *   - 2 bits per base, 32 bases per uint64.
 *   - One validity bit per base, 64 per uint64.
 *   - Every sequence starts at a multiple of 64 bases in both arrays, so no two sequences share a word.
 *   - Padding bits, and the 2-bit fields of invalid bases, are zero.
 *   - That is 0.375 bytes per base.  The arrays grow by doubling, as the occurrence builder's log does.
 *   Concurrency:
 *   - Adds are serialised on the object's mutex.
 *   - The verify calls only read the object and MUST NOT RUN CONCURRENTLY WITH AN ADD (an add may move the arrays; it waits
 *     for the device before it frees the old ones).  Verify calls from several host threads on one object are safe.
 * Oriented read
 *   For a record with strand = o, the oriented read is r = read for o = 0 and r = rc(read) for o = 1.  The complement rule is
 *   that of the read-hit profiles, and an invalid byte stays invalid.  L is the read's length and T is sequence seq of length n.
 *   Reference coordinate p matches r[j] iff 0 <= p < n, T[p] and r[j] are both valid, and they are equal.
 * The result record
 *   sbwtgpu_read_verify is 16 bytes: int64 ref_end; int32 mismatches; int32 edit.
 *   - mismatches is the number of j in [0, L) for which start + j does not match r[j].  An overhang beyond either end of the
 *     sequence counts base by base.
 *   - edit, with band B = band (0 ... SBWTGPU_VERIFY_MAX_BAND = 256), is defined on the window of reference coordinates
 *     [start - B, start + L + B).
 *     - edit is the smallest Levenshtein distance between r and any substring of the window.  The empty substring is included.
 *     - Substitution, insertion and deletion cost 1 each.
 *     - A pair is equal only if it matches as defined above.
 *     - This is the last row of Sellers' table: D[0][t] = 0 for t = 0 ... L + 2B, D[i][0] = i, and edit = min_t D[L][t].
 *   - ref_end is the smallest exclusive end coordinate start - B + t at which that minimum is attained.
 *   - The path is not band-limited.  The band only sizes the window.
 * Special cases
 *   - The unverified record is {0, -1, -1}.  It is returned for a record with seq < 0, seq >= n_seqs, strand outside {0, 1}, or
 *     |start| >= 2^40.
 *   - A read longer than SBWTGPU_VERIFY_MAX_READ = 1024 bases gets its exact mismatches, with edit = -1 and ref_end = 0.  The
 *     window table is quadratic, and such reads are to be cut into pieces, as the map calls' text above already says.
 *   - L = 0 gives {start - B, 0, 0}.
 * Properties that follow from the definitions
 *   - edit <= mismatches for every B.
 *   - edit is non-increasing in B.
 *   - edit = 0 iff r occurs in the window.
 *   - (rc(read), 1 - strand) gives the same record as (read, strand).
 *   - The result does not depend on what the neighbouring sequences in the packed arrays hold.
 * Not built: the runner-up's verification (the map record does not carry its placement), a reference file format (the CLI
 * re-reads the sequence files), SAM/PAF files, clipping of overhangs.  The begin of the best alignment and its CIGAR: "alignment
 * of mapped reads" below.
 * sbwtgpu_refseqs_create makes an empty object on `device` (SBWTGPU_ERR_NO_DEVICE without one).  sbwtgpu_refseqs_add_batch
 * takes host buffers (sequence i is bases[read_off[i] .. read_off[i + 1])), stages the batch on the device in one piece and
 * packs it with one kernel, one lane per 2-bit word; it returns when the sequences are in place.
 * sbwtgpu_refseqs_info: any output may be NULL; n_invalid counts the bases that are not upper-case ACGT; device_bytes is what
 * the object holds on the device.  sbwtgpu_refseqs_lengths_copy copies the n_seqs lengths.  sbwtgpu_refseqs_get unpacks bases
 * pos .. pos + len of sequence seq to ASCII (no NUL), N for every invalid base.
 * sbwtgpu_refseqs_verify_dev takes device pointers (d_bases: total_bases bytes; d_read_off: n_reads + 1 offsets that begin at
 * 0; d_map: n_reads map records, of which it reads only seq, strand and start; d_out: n_reads records).  It is asynchronous on
 * `stream`, never synchronises and never allocates.  Its workspace, of sbwtgpu_refseqs_verify_workspace_bytes (non-decreasing
 * in both arguments, a multiple of 256), is 16-byte aligned: a 256-byte header and 4 bytes per read.  Two kernels run.  The
 * first gives every read ONE LANE: Myers' bit-vector form of the table is sequential over the window's columns and parallel
 * over 64 rows per machine word, so 64 reads per wave keep every lane busy; the rows of a read of up to 256 bases live in
 * registers, and a wave runs the code of its longest read.  Longer reads go onto a list in the workspace.  The second kernel,
 * always launched, runs over that list with the rows in LDS (reads of up to 1024 bases) or counts the mismatches of a still
 * longer read in a linear pass.  "verify_fast_bases" (sbwtgpu_set_tuning: 1 .. 256, 0 = 256) lowers the first kernel's limit; no
 * result depends on it (tests reach the second kernel with short reads).  A record whose offsets are not those of a batch
 * (negative length, a read outside the base buffer) is answered with the unverified record.
 * sbwtgpu_refseqs_verify_batch is the same call on host buffers: one staged range, not pipelined.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL arguments; band outside 0 ... 256; n_reads < 0
 * or >= 2^31; first_seq not equal to the next number; more than 2^30 sequences; a workspace that is too small; get outside its
 * sequence.  A sequence of 2^31 bases or more gives SBWTGPU_ERR_READ_TOO_LONG.  SBWTGPU_ERR_OOM leaves the object as it was. */
typedef struct { int64_t ref_end; int32_t mismatches; int32_t edit; } sbwtgpu_read_verify;
typedef struct sbwtgpu_refseqs sbwtgpu_refseqs;
#define SBWTGPU_VERIFY_MAX_BAND 256
#define SBWTGPU_VERIFY_MAX_READ 1024
int     sbwtgpu_refseqs_create(int device, sbwtgpu_refseqs **out);
void    sbwtgpu_refseqs_destroy(sbwtgpu_refseqs *r);
int     sbwtgpu_refseqs_add_batch(sbwtgpu_refseqs *r, int64_t first_seq, const char *bases, const int64_t *read_off, int64_t n_seqs);
int     sbwtgpu_refseqs_info(const sbwtgpu_refseqs *r, int64_t *n_seqs, int64_t *total_bases, int64_t *n_invalid, int64_t *device_bytes);
int     sbwtgpu_refseqs_lengths_copy(const sbwtgpu_refseqs *r, int64_t *len /* n_seqs */);
int     sbwtgpu_refseqs_get(const sbwtgpu_refseqs *r, int64_t seq, int64_t pos, int64_t len, char *out);
int64_t sbwtgpu_refseqs_verify_workspace_bytes(int64_t total_bases, int64_t n_reads);
int     sbwtgpu_refseqs_verify_dev(const sbwtgpu_refseqs *r, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                   int64_t n_reads, const sbwtgpu_read_map *d_map, int band, sbwtgpu_read_verify *d_out,
                                   void *d_workspace, int64_t workspace_bytes, void *stream);
int     sbwtgpu_refseqs_verify_batch(const sbwtgpu_refseqs *r, const char *bases, const int64_t *read_off, int64_t n_reads,
                                     const sbwtgpu_read_map *map, int band, sbwtgpu_read_verify *out);

/* ---- alignment of mapped reads ----
 * The verify calls above say that a read fits its placement with `edit` edits and where the best alignment ends.  These calls
 * say where it begins and what it is: the runs of = X I D, as a CIGAR.  The terms of "reference sequences and verification"
 * apply unchanged: valid base, oriented read r, "coordinate p matches r[j]", the window [start - B, start + L + B), Sellers'
 * table D with D[0][t] = 0 and D[i][0] = i, edit, ref_end.
 * Column t >= 1 of D stands for reference coordinate start - B + t - 1.  Let tE = ref_end - (start - B).
 * The alignment of a read with edit >= 0 and L > 0 is the path found by walking back from (i, t) = (L, tE) until i = 0.  At
 * each cell take the FIRST step that applies:
 *   1. Diagonal.  Applies if t > 0 and D[i-1][t-1] + c == D[i][t], where c = 0 if column t's coordinate matches r[i-1] and c = 1
 *      otherwise.  Emit = when c = 0 and X when c = 1.  Then i--, t--.
 *   2. Insertion.  Applies if D[i-1][t] + 1 == D[i][t].  Emit I: read base r[i-1] faces nothing.  Then i--.
 *   3. Deletion.  Otherwise t > 0 and D[i][t-1] + 1 == D[i][t].  Emit D: a reference coordinate faces nothing.  Then t--.
 * When i = 0, ref_begin = start - B + t.  The emitted operations are reversed into read order, and equal neighbours are merged
 * into runs.
 * A run is one uint32 as in BAM: length << 4 | code, with I = 1, D = 2, = = 7, X = 8.  A coordinate outside [0, n) or on an
 * invalid base is an ordinary column that matches nothing.  It can only be X or D.  ref_begin may be negative and ref_end may
 * exceed n, exactly as ref_end can today.
 * The record
 *   sbwtgpu_read_align is 16 bytes: int64 ref_begin; int32 n_ops; int32 n_eq.  n_ops is the number of runs.  n_eq is the number
 *   of = columns.
 * Special cases
 *   - An unverified record, or a read of more than 1024 bases (edit = -1), gives {0, 0, 0} and no runs.
 *   - L = 0 gives {start - B, 0, 0}.
 *   - n_ops = 0 holds in no other case.
 * Properties that follow
 *   - #= + #X + #I = L.
 *   - #= + #X + #D = ref_end - ref_begin.
 *   - #X + #I + #D = edit.
 *   - The first and the last run are never D.  The start is free, and tE is the smallest minimiser.
 *   - n_ops <= 2 edit + 1.
 *   - No two neighbouring runs have the same code.
 *   - edit = 0 gives the single run L= and ref_begin = ref_end - L.
 *   - ref_begin >= start - B.
 *   - (rc(read), 1 - strand) gives the same alignment as (read, strand).
 *   - The alignment does not depend on neighbouring sequences.
 * The band lemma
 *   Restrict the table to the diagonals d = t - i with |d - (tE - L)| <= edit, and treat every cell outside as infinite.  The
 *   walk over this banded table takes exactly the same steps as the walk over the full table.
 *   - Every cell the walk visits lies on an optimal path to (L, tE).
 *   - Such a path has at most edit indels, so it cannot leave the band, and its cells' banded values equal the true ones.
 *   - A neighbour that fails its test in the full table has a banded value at least as large, so it fails there too.
 *   So the traceback needs 2 edit + 1 cells per row, not the window.
 * sbwtgpu_align_dev takes the device pointers of sbwtgpu_refseqs_verify_dev and runs that call's kernels first, unchanged:
 * d_verify_out receives exactly what sbwtgpu_refseqs_verify_dev writes for the same input.  Then d_out receives the n_reads
 * records, d_op_off the n_reads + 1 run offsets, and d_ops the runs: read i's are d_ops[d_op_off[i] .. d_op_off[i + 1]), in read
 * order.  ops_cap follows the rule of sbwtgpu_unitigs_walks_dev: d_op_off[n_reads] always receives the true total, only runs
 * numbered below ops_cap are stored, and nothing is written at or beyond d_ops[ops_cap] (d_ops may be NULL for ops_cap = 0).  The
 * call is asynchronous on `stream`, never synchronises and never allocates; the offsets come from a device scan on that stream.
 * Its workspace, of sbwtgpu_align_workspace_bytes (a multiple of 256, non-decreasing in both arguments, 16-byte aligned), holds
 * the verify workspace first, then a 256-byte header, 12 bytes per read and the scratch of a fixed grid of waves (at most 288 MiB,
 * whatever the batch).
 * The kernels: the first gives every read ONE LANE.  A lane with edit = 0 needs no table.  The others run the banded table row
 * by row, the row in registers, and record per row which of tests 1 and 2 hold for each band cell, two bit masks of at most 64
 * bits, in the wave's [row][lane] scratch; then they walk back over those masks.  A wave runs the code of its widest member
 * (bands for edit <= 1, 3, 7, 15, 31).  Reads with edit > 31, or of more than 256 bases, go onto a list; the second kernel
 * gives each of them one wave, which runs the whole window (up to 1536 columns, 24 per lane) and is exact for every edit.
 * THE SECOND KERNEL IS FAR SLOWER: it is a fixed grid of 64 waves, one read each, some 6 % of an MI355X's SIMDs.  A batch of
 * reads of more than 256 bases runs entirely there; the layer's measured throughput is that of reads of
 * up to 256 bases and 31 edits.
 * "align_fast_edit" (sbwtgpu_set_tuning: 1 .. 31, 0 = 31) lowers the first kernel's limit; no result depends on it (tests
 * reach the second kernel with short reads).  Both kernels run twice around the scan: count the runs, then store them.
 * sbwtgpu_align_batch is the same call on host buffers: one staged range, not pipelined.  verify_out, out and op_off
 * (n_reads + 1) are the caller's; *ops_out is memory of the library that holds the *n_ops runs (release it with
 * sbwtgpu_free_host), NULL when there are no runs.
 * Both calls are safe from several host threads on one object and, like the verify calls, must not run during an add.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): those of the verify calls, ops_cap < 0, and NULL
 * outputs (d_verify_out, d_out, d_op_off; d_ops with ops_cap > 0; verify_out, out, op_off, ops_out, n_ops). */
typedef struct { int64_t ref_begin; int32_t n_ops; int32_t n_eq; } sbwtgpu_read_align;
int64_t sbwtgpu_align_workspace_bytes(int64_t total_bases, int64_t n_reads);
int     sbwtgpu_align_dev(const sbwtgpu_refseqs *r, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                          const sbwtgpu_read_map *d_map, int band, sbwtgpu_read_verify *d_verify_out, sbwtgpu_read_align *d_out,
                          int64_t *d_op_off /* n_reads + 1 */, uint32_t *d_ops, int64_t ops_cap,
                          void *d_workspace, int64_t workspace_bytes, void *stream);
int     sbwtgpu_align_batch(const sbwtgpu_refseqs *r, const char *bases, const int64_t *read_off, int64_t n_reads, const sbwtgpu_read_map *map,
                            int band, sbwtgpu_read_verify *verify_out, sbwtgpu_read_align *out, int64_t *op_off, uint32_t **ops_out, int64_t *n_ops);

/* ---- pileup of aligned reads ----
 * The align calls above end in a per-read record.  A pileup sums those records over a read set: what the sample says about
 * reference base p -- depth, the bases seen, deletions and insertions -- in an accumulator that lives on the device across
 * batches.  It is the reference-coordinate counterpart of sbwtgpu_genotype_*, which works on the graph.  The terms of the two
 * headings above hold unchanged: valid base, oriented read r, "coordinate p matches r[j]", edit, ref_begin, ref_end, and the
 * runs.  Everything is exact integers.
 * Filter
 *   sbwtgpu_pileup_filter is 16 bytes: int32 min_votes, require_unique, max_edit, reserved.  A read is PILED iff all of these
 *   hold:
 *   - Its align record has n_ops > 0.
 *   - 0 <= seq < n_seqs of the pileup.
 *   - votes >= min_votes.
 *   - require_unique == 0 or votes > votes2.
 *   - max_edit < 0 or edit <= max_edit.
 *   reserved must be 0.  Every other read is OFFERED only.
 * Columns
 *   Replay the runs of a piled read from p = ref_begin, j = 0.  Let n be the length of sequence seq.
 *   - = at p: covers p.
 *   - X at p: covers p.  Let b = r[j], the base of the ORIENTED read.  For strand 1 that is the complement of read[L - 1 - j].
 *     - If b is valid, it is an observation of base b at p.
 *     - If b is not valid, it is an observation of `other`.
 *   - D at p: covers p and is an observation of `del`.
 *   - I run of length l:
 *     - If it is the first or the last run of the alignment it is a CLIP.  It adds l to the scalar n_clipped and nothing else.
 *     - Otherwise it is one observation of `ins` at its anchor, the coordinate p - 1 of the column before it.  This is VCF's
 *       convention.  The inserted bases themselves are not kept.
 *   A column or anchor with p outside [0, n) adds one to the scalar n_overhang and nothing per base.
 * The per-base record
 *   sbwtgpu_pileup_base is 32 bytes, uint32 depth, n[4], n_del, n_ins, n_other.
 *   - depth is the number of columns covering p.
 *   - n[c] counts observations of base code c (A 0, C 1, G 2, T 3).  The = columns count under the reference's own code.
 *   - n_del, n_ins and n_other are as above.
 *   Properties:
 *   - depth = n[0] + n[1] + n[2] + n[3] + n_del + n_other.
 *   - At an invalid reference base no = exists, so the record holds only what the X and D columns gave.
 *   - n_ins <= depth.
 *   - The sum of depth over all bases, plus the overhang columns, is the sum of ref_end - ref_begin over the piled reads.
 *   - The pileup of a read set does not depend on batch boundaries, order, chunking or the number of host threads.
 *   - (rc(read), 1 - strand) piles as (read, strand).
 * Calls
 *   Thresholds are min_depth >= 1, min_alt >= 1 and min_frac_ppm in 0 ... 10^6.  Calls are made at a VALID reference base p only.
 *   - A candidate allele a runs through 0 ... 3 except the reference's code, then 4 (DEL, count n_del), then 5 (INS, count n_ins).
 *   - A candidate with count c is CALLED iff depth >= min_depth, c >= min_alt and c*10^6 >= min_frac_ppm*depth.  The
 *     products are 64-bit.
 *   - sbwtgpu_pileup_call is 32 bytes: int64 pos; int32 seq, allele, ref, depth, count, ref_count.  ref is the reference's code
 *     and ref_count is n[ref].
 *   - Calls come in ascending (seq, pos, allele).
 * Not built: consecutive deleted bases joined into one event, the inserted sequence, base qualities, a consensus sequence, VCF
 * or SAM files, the runner-up placement.
 * The object
 *   sbwtgpu_pileup_create(r, out) covers the sequences r holds at that moment.  r must outlive the pileup, and, as for the verify
 *   calls, no call on the pileup may run during an add to r.  It allocates 32 bytes per base of r's slots (units of 64 bases, as
 *   the packed layout has them), one entry more, 256 bytes of scalars and 8 bytes per 1024 entries for the read-outs.
 *   SBWTGPU_ERR_OOM leaves nothing allocated.  sbwtgpu_pileup_reset zeroes everything; it waits for the device first.
 *   The counters lie at the coordinates of r's layout: base p of sequence s is entry 64 * slot(s) + p.  One of the eight words
 *   of an entry is a DIFFERENCE ARRAY: every coordinate of [ref_begin, ref_end) is exactly one of = X D, so the = columns need
 *   no counter.  A piled read adds +1 at ref_begin and -1 at ref_end (both clamped to [0, n]) and one to a counter per X and D
 *   column and per interior I run.  At read-out the depth is the prefix sum over ALL entries, and the matches are the depth
 *   minus the rest.  A read's -1 at n of a sequence whose length is a multiple of 64 lands on the entry that the next
 *   sequence's coordinate 0 uses; the prefix sum over all entries still gives every base its true value.
 * Adding
 *   sbwtgpu_pileup_add_aligned_dev takes what sbwtgpu_align_dev took and wrote for the same batch: bases, offsets, map records,
 *   d_verify, d_align, d_op_off and d_ops.  THE RUNS MUST ALL BE THERE: it is the caller's duty to have given sbwtgpu_align_dev
 *   an ops_cap >= the total.  It has no workspace, is asynchronous on `stream`, never synchronises and never allocates.  One
 *   kernel, ONE LANE per read: the filter, the walk over the read's runs, two atomics on the difference array and one 32-bit
 *   atomic per X or D column and per interior I run; the scalars go to the 256-byte block once per wave.
 *   A lane loops once per column of its X and D runs, so a wave takes as long as its read with the most such columns: one
 *   long D run (a read of several hundred bases beside a large deletion, band permitting) holds its 63 neighbours for that many
 *   steps.  The run lengths are trusted as sbwtgpu_align_dev wrote them.
 *   sbwtgpu_pileup_add_dev takes reads and map records and runs sbwtgpu_align_dev first, unchanged, then the same kernel.  Its
 *   workspace, of sbwtgpu_pileup_workspace_bytes (a multiple of 256, non-decreasing in both arguments, 16-byte aligned), holds
 *   the align workspace first, then the verify and align records and the run offsets, then room for 2 L runs per read (the bound
 *   of sbwtgpu_align_batch).  sbwtgpu_pileup_add_batch is the same call on host buffers: one staged range, not pipelined.
 *   Overflow: an add that would take the reads offered since the last reset above 2^31 - 1 is refused, so no 32-bit counter can
 *   wrap.
 * Reading out
 *   sbwtgpu_pileup_info: any output may be NULL.  n_columns is the sum of depth over all bases.  sbwtgpu_pileup_counts_copy
 *   writes the len records of coordinates pos .. pos + len of sequence seq to host memory; sbwtgpu_pileup_counts_dev writes them
 *   to device memory, asynchronously on `stream` (it sees the adds that `stream` is ordered after).  sbwtgpu_pileup_calls
 *   returns the calls in memory of the library (release it with sbwtgpu_free_host), NULL with *n = 0 for no calls: count, device
 *   scan, fill.  Read-out does not disturb the accumulators: an add after a read-out continues the same pileup.
 *   COST OF A READ-OUT: every counts and calls call first sums the difference array over ALL entries (one pass over the
 *   table's 32 bytes per base), however small the range asked for; nothing is cached between calls.  Ask for long ranges.
 *   counts_copy and calls also allocate their result on the device per call.
 * Concurrency: adds from several host threads on one object are safe, since the table is built on atomic adds.  info, counts,
 * calls and reset serialise on the object; info, counts_copy, calls and reset wait for the device and so see every add that has
 * returned.  That wait is hipDeviceSynchronize: it waits for EVERY stream of the device, work that has nothing to do with the
 * pileup included, and holds the object's mutex meanwhile.  counts_dev waits for nothing.
 * Refusals (SBWTGPU_ERR_INVALID_ARG with a message that names the cause): NULL arguments; reserved != 0; band outside 0 ... 256;
 * n_reads < 0 or >= 2^31; the overflow rule; a workspace that is too small; counts outside its sequence; thresholds out of
 * range. */
typedef struct { int32_t min_votes; int32_t require_unique; int32_t max_edit; int32_t reserved; } sbwtgpu_pileup_filter;
typedef struct { uint32_t depth; uint32_t n[4]; uint32_t n_del; uint32_t n_ins; uint32_t n_other; } sbwtgpu_pileup_base;
typedef struct { int64_t pos; int32_t seq; int32_t allele; int32_t ref; int32_t depth; int32_t count; int32_t ref_count; } sbwtgpu_pileup_call;
typedef struct sbwtgpu_pileup sbwtgpu_pileup;
#define SBWTGPU_PILEUP_DEL 4
#define SBWTGPU_PILEUP_INS 5
int     sbwtgpu_pileup_create(const sbwtgpu_refseqs *r, sbwtgpu_pileup **out);
int     sbwtgpu_pileup_reset(sbwtgpu_pileup *p);
void    sbwtgpu_pileup_destroy(sbwtgpu_pileup *p);
int     sbwtgpu_pileup_add_aligned_dev(sbwtgpu_pileup *p, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                                       const sbwtgpu_read_map *d_map, const sbwtgpu_read_verify *d_verify, const sbwtgpu_read_align *d_align,
                                       const int64_t *d_op_off, const uint32_t *d_ops, const sbwtgpu_pileup_filter *f, void *stream);
int64_t sbwtgpu_pileup_workspace_bytes(int64_t total_bases, int64_t n_reads);
int     sbwtgpu_pileup_add_dev(sbwtgpu_pileup *p, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                               const sbwtgpu_read_map *d_map, int band, const sbwtgpu_pileup_filter *f,
                               void *d_workspace, int64_t workspace_bytes, void *stream);
int     sbwtgpu_pileup_add_batch(sbwtgpu_pileup *p, const char *bases, const int64_t *read_off, int64_t n_reads, const sbwtgpu_read_map *map,
                                 int band, const sbwtgpu_pileup_filter *f);
int     sbwtgpu_pileup_info(const sbwtgpu_pileup *p, int64_t *n_seqs, int64_t *total_bases, int64_t *n_offered, int64_t *n_piled,
                            int64_t *n_columns, int64_t *n_clipped, int64_t *n_overhang, int64_t *device_bytes);
int     sbwtgpu_pileup_counts_copy(const sbwtgpu_pileup *p, int64_t seq, int64_t pos, int64_t len, sbwtgpu_pileup_base *out);
int     sbwtgpu_pileup_counts_dev(const sbwtgpu_pileup *p, int64_t seq, int64_t pos, int64_t len, sbwtgpu_pileup_base *d_out, void *stream);
int     sbwtgpu_pileup_calls(const sbwtgpu_pileup *p, int32_t min_depth, int32_t min_alt, int32_t min_frac_ppm, sbwtgpu_pileup_call **out,
                             int64_t *n);

#ifdef __cplusplus
}
#endif
#endif
