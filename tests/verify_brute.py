"""The definition of "reference sequences and verification" (include/sbwtgpu.h) in pure Python, from
strings: what the packed object stores and gives back, the oriented read, the mismatches on the voted diagonal, Sellers' table
as a plain double loop and as numpy rows, the record with its special cases, and the three columns the CLI appends.

A record is the tuple (ref_end, mismatches, edit).  A map record is (seq, strand, start)."""
import numpy as np

MAX_BAND = 256
MAX_READ = 1024
UNVERIFIED = (0, -1, -1)
START_LIMIT = 1 << 40
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}        # A<->T, C<->G on upper-case bytes only


def valid(b: int) -> bool:
    return b in _COMP


def stored(seq: bytes) -> bytes:
    """what sbwtgpu_refseqs_get gives for the whole sequence: N for every byte that is not upper-case ACGT"""
    return bytes(b if valid(b) else 78 for b in seq)


def n_invalid(seqs) -> int:
    return sum(1 for s in seqs for b in s if not valid(b))


def packed_words(seq: bytes):
    """(2-bit words, validity words) of one sequence as the object lays them out: 32 bases per uint64, 64 validity bits per
    uint64, ceil(len / 64) units of 64 bases, padding and invalid fields zero"""
    units = (len(seq) + 63) // 64
    bits, val = [0] * (2 * units), [0] * units
    for p, b in enumerate(seq):
        if valid(b):
            code = ((b >> 1) & 3) ^ ((b >> 2) & 1)          # A 0, C 1, G 2, T 3
            bits[p >> 5] |= code << (2 * (p & 31))
            val[p >> 6] |= 1 << (p & 63)
    return bits, val


def orient(read: bytes, strand: int):
    """the oriented read as a list of codes: the byte itself where it is valid, None where it is not (an invalid byte stays
    invalid under the complement)"""
    if strand == 0:
        return [b if valid(b) else None for b in read]
    return [_COMP.get(b) for b in reversed(read)]


def text_at(ref: bytes, p: int):
    """T[p] as the definition sees it: None outside the sequence and on an invalid base"""
    if 0 <= p < len(ref) and valid(ref[p]):
        return ref[p]
    return None


def matches(ref: bytes, p: int, rj) -> bool:
    t = text_at(ref, p)
    return t is not None and rj is not None and t == rj


def mismatches(ref: bytes, r, start: int) -> int:
    return sum(1 for j, rj in enumerate(r) if not matches(ref, start + j, rj))


def sellers_loop(ref: bytes, r, start: int, band: int):
    """(edit, ref_end) from the table as a plain double loop"""
    L = len(r)
    lo, n_cols = start - band, L + 2 * band
    prev = [0] * (n_cols + 1)                               # D[0][t] = 0
    for i in range(1, L + 1):
        cur = [i] + [0] * n_cols                            # D[i][0] = i
        for t in range(1, n_cols + 1):
            sub = prev[t - 1] + (0 if matches(ref, lo + t - 1, r[i - 1]) else 1)
            cur[t] = min(sub, prev[t] + 1, cur[t - 1] + 1)
        prev = cur
    edit = min(prev)
    return edit, lo + prev.index(edit)


def sellers_numpy(ref: bytes, r, start: int, band: int):
    """The same table row by row in numpy: the diagonal and vertical minima elementwise, then the horizontal step as a min-plus
    prefix scan, np.minimum.accumulate(x - idx) + idx."""
    L = len(r)
    lo, n_cols = start - band, L + 2 * band
    win = np.array([text_at(ref, lo + t) or 0 for t in range(n_cols)], dtype=np.int64)      # 0: matches nothing
    idx = np.arange(n_cols + 1, dtype=np.int64)
    prev = np.zeros(n_cols + 1, dtype=np.int64)
    for i in range(1, L + 1):
        rj = r[i - 1] or -1                                                                # -1: matches nothing
        x = np.empty(n_cols + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(prev[:-1] + (win != rj), prev[1:] + 1)
        prev = np.minimum.accumulate(x - idx) + idx
    edit = int(prev.min())
    return edit, lo + int(np.argmax(prev == edit))


def record(refs, read: bytes, rec, band: int, table=sellers_numpy):
    """the sbwtgpu_read_verify of one read; refs: the sequences 0, 1, ... as byte strings; rec: (seq, strand, start)"""
    assert 0 <= band <= MAX_BAND
    seq, strand, start = rec
    if seq < 0 or seq >= len(refs) or strand not in (0, 1) or abs(start) >= START_LIMIT:
        return UNVERIFIED
    if len(read) == 0:
        return (start - band, 0, 0)
    r = orient(read, strand)
    mm = mismatches(refs[seq], r, start)
    if len(read) > MAX_READ:
        return (0, mm, -1)
    edit, end = table(refs[seq], r, start, band)
    return (end, mm, edit)


def records(refs, reads, recs, band: int):
    return [record(refs, rd, rc, band) for rd, rc in zip(reads, recs)]


def cli_columns(rec) -> str:
    """what `sbwt read-hits --refs` appends to a line: mismatches edit ref_end"""
    return "%d %d %d" % (rec[1], rec[2], rec[0])


def rc(read: bytes) -> bytes:
    """the reverse complement as bytes, an invalid byte kept as it is (it stays invalid)"""
    return bytes(_COMP.get(b, b) for b in reversed(read))
