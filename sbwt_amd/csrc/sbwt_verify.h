// sbwt_verify.h -- the reference sequences packed on the device and the verification of mapped reads against them
// (sbwt_verify.hip; include/sbwtgpu.h, "reference sequences and verification").  What the C-ABI host
// code launches.
#pragma once
#include <hip/hip_runtime.h>

#define SBWT_VF_FAST_BASES 256      // the longest read the first kernel takes: four words of rows in registers
#define SBWT_VF_MAX_READ 1024       // the longest read that gets an edit distance (sixteen words of rows in LDS)
#define SBWT_VF_MAX_BAND 256

// A sequence of the object: where it starts in the packed arrays, in units of 64 bases, and its length in bases.  Sequence s
// owns the words bits[2 slot .. 2 (slot + ceil(len / 64))) and valid[slot .. slot + ceil(len / 64)).
struct SbwtRefSeq { long long slot, len; };
static_assert(sizeof(SbwtRefSeq) == 16, "a sequence entry is two words");

// the counters of a reference object, on the device
struct SbwtRefCounters { unsigned long long n_invalid; unsigned long long pad[31]; };
static_assert(sizeof(SbwtRefCounters) == 256, "the reference counters are 256 bytes");

// the map record as the kernels read it (sbwtgpu_read_map) and the record they write (sbwtgpu_read_verify)
struct SbwtVerifyMap { long long start; int seq, strand, votes, votes2, n_found, n_anchored; };
struct SbwtReadVerify { long long ref_end; int mismatches, edit; };
static_assert(sizeof(SbwtVerifyMap) == 32 && sizeof(SbwtReadVerify) == 16, "the records of the ABI");

// The head of the verify calls' workspace: the length of the list of reads that the first kernel left to the second, then
// the list (4 bytes per read).
struct SbwtVerifyHeader { unsigned n_slow; unsigned pad[63]; };
static_assert(sizeof(SbwtVerifyHeader) == 256, "the verify header is 256 bytes");

// Packs the n sequences d_src[d_src_off[i] .. d_src_off[i + 1]) into the words that tab[first_seq + i] names: the 2-bit words
// [2 slot_lo, 2 slot_hi) and the validity words [slot_lo, slot_hi), every one of them written (padding as zero).
// ctr->n_invalid grows by the bases that are not upper-case ACGT.
void sbwt_launch_ref_pack(const char *d_src, const long long *d_src_off, const SbwtRefSeq *tab, long long first_seq, long long n,
                          long long slot_lo, long long slot_hi, unsigned long long *d_bits, unsigned long long *d_valid,
                          SbwtRefCounters *ctr, hipStream_t stream);

// d_out[0 .. len) = the bases pos .. pos + len of the sequence at `slot` as ASCII, N for an invalid one
void sbwt_launch_ref_unpack(const unsigned long long *d_bits, const unsigned long long *d_valid, long long slot, long long pos,
                            long long len, char *d_out, hipStream_t stream);

// One record per read from its bases, its map record (seq, strand, start) and the packed references.  Two launches: one lane
// per read for the reads of at most fast_bases (1 .. SBWT_VF_FAST_BASES) bases, which appends the longer ones to d_slow, and a
// grid-stride kernel over that list.  hdr is zeroed here first.
void sbwt_launch_verify(const char *d_bases, long long total_bases, const long long *d_read_off, long long n_reads,
                        const SbwtVerifyMap *d_map, const SbwtRefSeq *tab, long long n_seqs, const unsigned long long *d_bits,
                        const unsigned long long *d_valid, int band, int fast_bases, SbwtReadVerify *d_out, SbwtVerifyHeader *hdr,
                        unsigned *d_slow, hipStream_t stream);
