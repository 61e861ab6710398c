"""Definition-level verifier of a plain-matrix SBWT in numpy: are these five bit rows the index of these sequences?

It shares no code with the builders (index_builder.hh, sbwt_build.hip / sbwt_sort.hip) or with oracle/: nothing is
sorted into an index here.  The rows are read back into the label of every column, and the labels are compared with
what the definition says about the input.

From the rows alone
    ones per row -> the C array (SBWT.hh:344-349: C[0] = 1 for the root's ghost `$`, C[c+1] = C[c] + ones of row c);
    column v in [C[c], C[c+1]) ends with c, and its predecessor is the column holding the (v - C[c])-th one of row c;
    walking pred k times spells the label from its last char backwards, `$` from the root on.

A label is packed so that integer order is colex order (Kmer.hh:108-123: last char most significant, `$` = A = 0, on a
tie the shorter label first): (hi, lo, length), the last 32 chars in `hi` (last char in bits 63..62), the ones before
them in `lo`, `length` = chars that are not `$`.

Checked
    1. the ones of the four rows add up to n_nodes - 1, nothing is set beyond column n_nodes - 1;
    2. labels strictly increasing: sorted, and no column twice;
    3. the `$`-free labels are exactly the distinct valid k-mers of the input (windows of upper-case ACGT, never across
       two sequences, of the reverse complements too when asked), and there are n_kmers of them;
    4. the labels with `$` are exactly the root and every proper prefix of every k-mer whose (k-1)-prefix is no k-mer's
       (k-1)-suffix;
    5. ssup is set exactly where the (k-1)-suffix differs from the column before (`$` compared as `$`);
    6. ones sit only on suffix-group starts;
    7. the i-th one of row c sits on the group whose (k-1)-suffix followed by c is the label of column C[c] + i.
       With 1, 2 and 6 this is "bit c of a group start is set exactly when some column's label is that group's suffix
       followed by c": every column but the root is the target of exactly one one (1), equal suffixes are neighbours
       in a sorted list (2), so that one can only sit on the start of the one group with the right suffix (6, 7).

verify_plain_matrix raises VerifyError (an AssertionError) naming the first check that fails, and returns the labels."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

U64 = np.uint64


class VerifyError(AssertionError):
    pass


class Labels(NamedTuple):
    hi: np.ndarray          # uint64: the last min(k, 32) chars, last char in bits 63..62
    lo: Optional[np.ndarray]  # uint64: the chars before those (k > 32), else None
    length: np.ndarray      # uint8: chars that are not `$`


_CODE = np.full(256, 4, dtype=np.uint8)
_CODE[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
_SEP = 10                   # between sequences: any byte that is not ACGT ends a window


def _need(ok, what):
    if not bool(ok):
        raise VerifyError(what)


def _bits(words, n) -> np.ndarray:
    """Bit j of the row as uint8[n]; refuses ones at or beyond column n."""
    w = np.ascontiguousarray(words, dtype=U64)
    nw = (n + 63) // 64
    _need(len(w) >= nw, "a row has fewer than ceil(n_nodes / 64) words")
    b = np.unpackbits(w[:nw].view(np.uint8), bitorder="little")
    _need(not b[n:].any(), "a bit is set at or beyond column n_nodes")
    return b[:n]


# ---- packed (hi, lo) keys ----
def _shl2(hi, lo, chars):
    """The key moved `chars` chars towards the top (dropping the last `chars` chars of the label)."""
    s = 2 * chars
    if lo is None:
        return (hi << U64(s)) if s < 64 else np.zeros_like(hi), None
    if s == 0:
        return hi, lo
    if s < 64:
        return (hi << U64(s)) | (lo >> U64(64 - s)), lo << U64(s)
    return (lo << U64(s - 64)) if s < 128 else np.zeros_like(hi), np.zeros_like(lo)


def _shr2_one(hi, lo):
    """The key moved one char away from the top (room for a new last char)."""
    if lo is None:
        return hi >> U64(2), None
    return hi >> U64(2), (lo >> U64(2)) | (hi << U64(62))


def _clear_first_char(hi, lo, k):
    """Zero the 2 bits of char 0 of a k-char label (what is left is its (k-1)-suffix, same alignment)."""
    if k <= 32:
        return hi & ~(U64(3) << U64(64 - 2 * k)), lo
    return hi, lo & ~(U64(3) << U64(128 - 2 * k))


def _lex_order(hi, lo, length=None):
    keys = [hi] if lo is None else [lo, hi]
    if length is not None:
        keys = [length] + keys
    if len(keys) == 1:
        return np.argsort(keys[0], kind="stable")
    return np.lexsort(keys)


def _differs_from_previous(hi, lo, length=None) -> np.ndarray:
    d = hi[1:] != hi[:-1]
    if lo is not None:
        d |= lo[1:] != lo[:-1]
    if length is not None:
        d |= length[1:] != length[:-1]
    return d


def _sorted_unique(hi, lo, length=None):
    if len(hi) == 0:
        return hi, lo, length
    if lo is None and length is None:
        return np.unique(hi), None, None
    o = _lex_order(hi, lo, length)
    hi, lo, length = hi[o], (None if lo is None else lo[o]), (None if length is None else length[o])
    keep = np.concatenate([[True], _differs_from_previous(hi, lo, length)])
    return hi[keep], (None if lo is None else lo[keep]), (None if length is None else length[keep])


def _strictly_increasing(hi, lo, length) -> bool:
    a, b = slice(0, -1), slice(1, None)
    lt = length[a] < length[b]
    if lo is not None:
        lt = (lo[a] < lo[b]) | ((lo[a] == lo[b]) & lt)
    lt = (hi[a] < hi[b]) | ((hi[a] == hi[b]) & lt)
    return bool(lt.all())


def _is_member(q_hi, q_lo, s_hi, s_lo) -> np.ndarray:
    """For every query key: is it in the sorted, duplicate-free key list s?"""
    if s_lo is None:
        return np.isin(q_hi, s_hi)
    nq = len(q_hi)
    hi, lo = np.concatenate([q_hi, s_hi]), np.concatenate([q_lo, s_lo])
    o = np.lexsort([np.arange(len(hi)) < nq, lo, hi])       # equal keys: the member of s first, then the queries
    hi, lo = hi[o], lo[o]
    from_s = o >= nq
    first = np.concatenate([[True], _differs_from_previous(hi, lo)])
    head = np.maximum.accumulate(np.where(first, np.arange(len(hi)), 0))
    out = np.empty(len(hi), dtype=bool)
    out[o] = from_s[head]
    return out[:nq]


# ---- the input's side ----
def _window_words(code: np.ndarray, m: int) -> np.ndarray:
    """For every start i: sum of code[i + j] << 2j over j < m (m <= 32), by doubling; invalid codes must be 0 here."""
    n_out = len(code) - m + 1
    acc, acc_len = None, 0
    piece, piece_len = code.astype(U64), 1                  # piece[i] = window of piece_len chars at i
    mm = m
    while True:
        if mm & 1:
            if acc is None:
                acc, acc_len = piece, piece_len
            else:
                n = len(code) - (acc_len + piece_len) + 1
                acc = acc[:n] | (piece[acc_len:acc_len + n] << U64(2 * acc_len))
                acc_len += piece_len
        mm >>= 1
        if not mm:
            break
        n = len(piece) - piece_len
        piece = piece[:n] | (piece[piece_len:piece_len + n] << U64(2 * piece_len))
        piece_len *= 2
    assert acc_len == m
    return acc[:n_out]


def input_kmers(seqs: Sequence[bytes], k: int, add_revcomp: bool):
    """The distinct valid k-mers of the input as sorted packed keys (hi, lo)."""
    if len(seqs) == 0:
        text = np.zeros(0, dtype=np.uint8)
    else:
        text = np.frombuffer(bytes([_SEP]).join(bytes(s) for s in seqs), dtype=np.uint8)
    code = _CODE[text]
    if add_revcomp:                                          # the whole text reversed: every sequence's reverse complement
        rc = code[::-1]
        rc = np.where(rc < 4, 3 - rc, 4).astype(np.uint8)
        code = np.concatenate([code, np.array([4], dtype=np.uint8), rc])
    empty = np.zeros(0, dtype=U64)
    if len(code) < k:
        return empty, (None if k <= 32 else empty)
    bad = np.concatenate([[0], np.cumsum(code == 4, dtype=np.int64)])
    start = np.flatnonzero(bad[k:] == bad[:-k])              # windows without an invalid char
    clean = np.where(code == 4, 0, code).astype(np.uint8)
    if k <= 32:
        hi = _window_words(clean, k)[start] << U64(64 - 2 * k)
        lo = None
    else:
        hi = _window_words(clean, 32)[start + (k - 32)]
        lo = _window_words(clean, k - 32)[start] << U64(64 - 2 * (k - 32))
    hi, lo, _ = _sorted_unique(hi, lo)
    return hi, lo


def expected_dummies(u_hi, u_lo, k: int):
    """Root + every proper prefix of every k-mer that no k-mer precedes, as sorted keys (hi, lo, length)."""
    # both as (k-1)-mers with their last char at the top: the slot of a k-th char from the end is zero in either
    pre_hi, pre_lo = _shl2(u_hi, u_lo, 1)                    # chars 0 .. k-2
    suf_hi, suf_lo = _clear_first_char(u_hi, u_lo, k)        # chars 1 .. k-1
    s_hi, s_lo, _ = _sorted_unique(suf_hi, suf_lo)
    orphan = ~_is_member(pre_hi, pre_lo, s_hi, s_lo)
    o_hi, o_lo = u_hi[orphan], (None if u_lo is None else u_lo[orphan])
    his, los, lens = [np.zeros(1, dtype=U64)], [np.zeros(1, dtype=U64)], [np.zeros(1, dtype=np.uint8)]
    for j in range(1, k):                                    # the prefix of j chars: drop the last k - j
        h, l = _shl2(o_hi, o_lo, k - j)
        his.append(h)
        los.append(l if l is not None else np.zeros_like(h))
        lens.append(np.full(len(h), j, dtype=np.uint8))
    hi, lo, length = np.concatenate(his), np.concatenate(los), np.concatenate(lens)
    return _sorted_unique(hi, None if u_lo is None else lo, length)


# ---- the rows' side ----
def labels_from_rows(cols, n_nodes: int, k: int):
    """(Labels, bits of the four rows, C array) read back from the rows."""
    n = int(n_nodes)
    _need(n >= 1, "n_nodes < 1")
    rows = [_bits(c, n) for c in cols]
    ones = [np.flatnonzero(r) for r in rows]
    _need(sum(len(o) for o in ones) == n - 1, "the rows hold %d ones, not n_nodes - 1 = %d"
          % (sum(len(o) for o in ones), n - 1))
    C = np.cumsum([1] + [len(o) for o in ones])              # C[4] = n_nodes
    pred = np.concatenate([np.zeros(1, dtype=np.int64)] + ones)   # the root stays the root
    last = np.concatenate([np.full(1, 4, dtype=np.uint8)] + [np.full(len(o), c, dtype=np.uint8)
                                                             for c, o in enumerate(ones)])
    hi = np.zeros(n, dtype=U64)
    lo = np.zeros(n, dtype=U64) if k > 32 else None
    length = np.zeros(n, dtype=np.uint8)
    cur = np.arange(n, dtype=np.int64)
    for t in range(k):                                       # t-th char from the end
        ch = last[cur]
        real = ch < 4
        v = np.where(real, ch, 0).astype(U64)
        if t < 32:
            hi |= v << U64(62 - 2 * t)
        else:
            lo |= v << U64(62 - 2 * (t - 32))
        length += real
        cur = pred[cur]
    return Labels(hi, lo, length), rows, C


def labels_ascii(lab: Labels, k: int, start: int, stop: int) -> np.ndarray:
    """Columns [start, stop) as a (stop - start, k) array of chars, `$` first: what SBWT::get_kmer returns."""
    out = np.empty((stop - start, k), dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    length = lab.length[start:stop].astype(np.int64)
    for t in range(k):
        w = lab.hi[start:stop] if t < 32 else lab.lo[start:stop]
        ch = acgt[((w >> U64(62 - 2 * (t % 32))) & U64(3)).astype(np.int64)]
        out[:, k - 1 - t] = np.where(t < length, ch, ord("$"))
    return out


def verify_plain_matrix(seqs: Sequence[bytes], k: int, add_revcomp: bool, cols, ssup, n_nodes: int, n_kmers: int
                        ) -> Labels:
    _need(2 <= k <= 64, "k outside 2 .. 64")
    lab, rows, C = labels_from_rows(cols, n_nodes, k)
    n = int(n_nodes)
    hi, lo, length = lab
    _need(length[0] == 0, "column 0 is not the root")
    _need(_strictly_increasing(hi, lo, length), "labels are not strictly increasing in colex order")
    # 3: the k-mers
    full = length == k
    u_hi, u_lo = input_kmers(seqs, k, add_revcomp)
    _need(int(full.sum()) == len(u_hi), "%d k-mer columns, the input has %d distinct k-mers" % (int(full.sum()), len(u_hi)))
    _need(np.array_equal(hi[full], u_hi) and (lo is None or np.array_equal(lo[full], u_lo)),
          "the k-mer columns are not the input's k-mers")
    _need(int(n_kmers) == len(u_hi), "n_kmers = %d, the input has %d distinct k-mers" % (n_kmers, len(u_hi)))
    # 4: the dummies
    d_hi, d_lo, d_len = expected_dummies(u_hi, u_lo, k)
    _need(n - len(u_hi) == len(d_hi), "%d dummy columns, the definition gives %d" % (n - len(u_hi), len(d_hi)))
    _need(np.array_equal(hi[~full], d_hi) and (lo is None or np.array_equal(lo[~full], d_lo))
          and np.array_equal(length[~full], d_len), "the dummy columns are not the prefixes of the predecessor-less k-mers")
    # 5, 6: suffix groups
    s_hi, s_lo = _clear_first_char(hi, lo, k)
    s_len = np.minimum(length, k - 1)
    start = np.concatenate([[True], _differs_from_previous(s_hi, s_lo, s_len)])
    if ssup is not None:
        _need(np.array_equal(_bits(ssup, n).astype(bool), start), "ssup is not set exactly where the (k-1)-suffix changes")
    for c in range(4):
        _need(not rows[c][~start].any(), "row %s has a one that is not on a suffix-group start" % "ACGT"[c])
    # 7: the i-th one of row c leads to column C[c] + i
    for c in range(4):
        src = np.flatnonzero(rows[c])
        t_hi, t_lo = _shr2_one(s_hi[src], None if s_lo is None else s_lo[src])
        t_hi = t_hi | (U64(c) << U64(62))
        v = slice(int(C[c]), int(C[c + 1]))
        _need(np.array_equal(t_hi, hi[v]) and (lo is None or np.array_equal(t_lo, lo[v]))
              and np.array_equal(s_len[src] + 1, length[v]),
              "row %s: a one does not lead to the column labelled suffix + %s" % ("ACGT"[c], "ACGT"[c]))
    return lab


# ---- what the builder tests share ----
def check_build(seqs: Sequence[bytes], k: int, add_revcomp: bool, got, host=None, verify: bool = True
                ) -> Optional[Labels]:
    """`got` (anything with cols, ssup, n_nodes, n_kmers) against the rows of a reference builder, bit for bit on every
    word, and / or against the definition.  Raises VerifyError; returns the verifier's labels when it ran.  The mutation
    tests of test_sbwt_verify.py drive this function, the device builder's tests call it."""
    _need(host is not None or verify, "no reference given")
    if host is not None:
        _need((got.n_nodes, got.n_kmers) == (host.n_nodes, host.n_kmers), "n_nodes, n_kmers = %d, %d; the reference has %d, %d"
              % (got.n_nodes, got.n_kmers, host.n_nodes, host.n_kmers))
        nw = (host.n_nodes + 63) // 64
        for c in range(4):
            _need(len(got.cols[c]) >= nw and np.array_equal(np.asarray(got.cols[c])[:nw], np.asarray(host.cols[c])[:nw]),
                  "row %s differs from the reference builder's" % "ACGT"[c])
        if got.ssup is not None:
            _need(host.ssup is not None and len(got.ssup) >= nw
                  and np.array_equal(np.asarray(got.ssup)[:nw], np.asarray(host.ssup)[:nw]),
                  "ssup differs from the reference builder's")
    if verify:
        return verify_plain_matrix(seqs, k, add_revcomp, got.cols, got.ssup, got.n_nodes, got.n_kmers)
    return None


def split_reads(bases: np.ndarray, off: np.ndarray) -> list:
    buf = bases.tobytes()
    return [buf[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def random_read_set(n_reads: int, read_len: int, k: int, seed: int) -> list:
    """Unrelated random reads as separate sequences: every read start is predecessor-less and brings k-1 dummy columns.
    One position in 30 000 becomes N, one in 30 000 lower case, and reads of k-1, k and k+1 bases are mixed in (one
    each per 1 000 reads)."""
    from sbwt_amd import synth
    bases, off = synth.random_reads(n_reads, read_len, seed)
    n_odd = max(3, len(bases) // 30_000)
    bases = synth.inject(bases, n_odd, ord("N"), seed + 1)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    at = rng.integers(0, len(bases), size=n_odd)
    bases[at] |= 0x20
    seqs = split_reads(bases, off)
    for i in range(0, n_reads, 1000):
        for j, L in enumerate((k - 1, k, k + 1)):
            seqs.insert(int(rng.integers(0, len(seqs) + 1)),
                        synth.random_genome(L, seed + 10 + 3 * i + j).tobytes())
    return seqs


def sampled_read_set(genome_len: int, n_reads: int, seed: int) -> list:
    """150-base reads with 1 % substitutions sampled from synth.coli3_like(genome_len), as separate sequences."""
    from sbwt_amd import synth
    bases, off = synth.sample_reads(synth.coli3_like(genome_len), n_reads, 150, 0.01, seed)
    return split_reads(bases, off)


def repeated_genome_set(genome_len: int, seed: int) -> list:
    """One genome eight times and its reverse complement once (to be built with add_revcomp: 18 copies of a k-mer)."""
    from sbwt_amd import synth
    g = synth.random_genome(genome_len, seed)
    return [g.tobytes()] * 8 + [synth.revcomp(g).tobytes()]


def no_kmer_set(n_seqs: int, k: int) -> list:
    """Sequences without a valid k-mer: all N (longer than k), or k-1 good bases."""
    from sbwt_amd import synth
    short = synth.random_genome(k - 1, 3).tobytes()
    return [b"N" * (k + 9) if i % 2 else short for i in range(n_seqs)]
