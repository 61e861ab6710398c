"""ctypes binding of include/sbwthost.h (libsbwthost.so): the sort-based index builder, the
reference index file format and the FASTA/FASTQ reader.  GPU-free host code either side of the
hot path."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SBWT_HOST_LIB", os.path.join(_HERE, "lib", "libsbwthost.so"))   # override: sanitizer build

EXPORTED_SYMBOLS = [
    "sbwthost_last_error", "sbwthost_build", "sbwthost_bits_free", "sbwthost_bits_info", "sbwthost_bits_words",
    "sbwthost_file_write", "sbwthost_file_read", "sbwthost_file_free", "sbwthost_file_info",
    "sbwthost_file_words", "sbwthost_file_precalc", "sbwthost_read_sequences", "sbwthost_read_sequences_chunked", "sbwthost_free", "sbwthost_write_file",
    "sbwthost_rank_batch", "sbwthost_colors_write", "sbwthost_colors_read",
    "sbwthost_colors_write_wide", "sbwthost_colors_read_wide", "sbwthost_colorsets_write", "sbwthost_colorsets_read",
    "sbwthost_positions_write", "sbwthost_positions_read", "sbwthost_occurrences_write", "sbwthost_occurrences_read",
]

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m sbwt_amd.build`")
    L = C.CDLL(LIB_PATH)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    L.sbwthost_last_error.restype = C.c_char_p
    L.sbwthost_build.argtypes = [C.POINTER(C.c_char_p), C.POINTER(i64), i64, i64, ci, ci, ci, C.POINTER(vp)]
    L.sbwthost_bits_free.argtypes = [vp]
    L.sbwthost_bits_free.restype = None
    L.sbwthost_bits_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(ci)]
    L.sbwthost_bits_words.argtypes = [vp, ci]
    L.sbwthost_bits_words.restype = C.POINTER(C.c_uint64)
    L.sbwthost_file_write.argtypes = [C.c_char_p, i64, vp, vp, vp, vp, vp, C.POINTER(i64), vp, i64, i64, i64]
    L.sbwthost_file_read.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.sbwthost_file_free.argtypes = [vp]
    L.sbwthost_file_free.restype = None
    L.sbwthost_file_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                     C.POINTER(i64), C.POINTER(ci)]
    L.sbwthost_file_words.argtypes = [vp, ci]
    L.sbwthost_file_words.restype = C.POINTER(C.c_uint64)
    L.sbwthost_file_precalc.argtypes = [vp]
    L.sbwthost_file_precalc.restype = C.POINTER(i64)
    L.sbwthost_read_sequences.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
    L.sbwthost_read_sequences_chunked.argtypes = [C.c_char_p, i64, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
    L.sbwthost_free.argtypes = [vp]
    L.sbwthost_free.restype = None
    L.sbwthost_write_file.argtypes = [C.c_char_p, C.c_char_p, i64, ci, ci]
    L.sbwthost_rank_batch.argtypes = [vp, i64, vp, i64, vp]
    L.sbwthost_colors_write.argtypes = [C.c_char_p, vp, i64, i64, i64]
    L.sbwthost_colors_read.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), vp, i64]
    L.sbwthost_colors_write_wide.argtypes = [C.c_char_p, vp, i64, i64, i64]
    L.sbwthost_colors_read_wide.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), vp, i64]
    L.sbwthost_colorsets_write.argtypes = [C.c_char_p, vp, vp, i64, i64, i64, i64]
    L.sbwthost_colorsets_read.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                          vp, i64, vp, i64]
    L.sbwthost_positions_write.argtypes = [C.c_char_p, vp, i64, i64, vp, vp, i64]
    L.sbwthost_positions_read.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), vp, vp, i64, vp, i64]
    L.sbwthost_occurrences_write.argtypes = [C.c_char_p, vp, vp, i64, i64, i64, vp, vp, i64]
    L.sbwthost_occurrences_read.argtypes = [C.c_char_p] + [C.POINTER(i64)] * 4 + [vp, vp, i64, vp, i64, vp, i64]
    _lib = L
    return L


def _err() -> str:
    return lib().sbwthost_last_error().decode(errors="replace")


class IndexBits:
    """A/C/G/T (+ suffix_group_starts) columns of one plain-matrix SBWT, as numpy uint64 words."""

    def __init__(self, cols: List[np.ndarray], ssup: Optional[np.ndarray], n_nodes: int, n_kmers: int, k: int):
        self.cols, self.ssup, self.n_nodes, self.n_kmers, self.k = cols, ssup, n_nodes, n_kmers, k


def build_bits(seqs: Sequence[bytes], k: int, add_revcomp: bool = False, streaming_support: bool = True,
               n_threads: int = 1) -> IndexBits:
    """Sort-based in-memory construction (index_builder.hh)."""
    L = lib()
    seqs = [bytes(s) for s in seqs]
    arr = (C.c_char_p * len(seqs))(*seqs)
    lens = (C.c_int64 * len(seqs))(*[len(s) for s in seqs])
    h = C.c_void_p()
    if L.sbwthost_build(arr, lens, len(seqs), k, int(add_revcomp), int(streaming_support), n_threads, C.byref(h)) != 0:
        raise RuntimeError(_err())
    try:
        n, nk, kk, hs = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        L.sbwthost_bits_info(h, C.byref(n), C.byref(nk), C.byref(kk), C.byref(hs))
        nw = (n.value + 63) // 64
        cols = [np.ctypeslib.as_array(L.sbwthost_bits_words(h, c), shape=(nw,)).copy() for c in range(4)]
        ssup = np.ctypeslib.as_array(L.sbwthost_bits_words(h, 4), shape=(nw,)).copy() if hs.value else None
        return IndexBits(cols, ssup, n.value, nk.value, kk.value)
    finally:
        L.sbwthost_bits_free(h)


class IndexFile:
    def __init__(self, cols, ssup, C_array, precalc, precalc_k, n_nodes, n_kmers, k):
        self.cols, self.ssup, self.C, self.precalc = cols, ssup, C_array, precalc
        self.precalc_k, self.n_nodes, self.n_kmers, self.k = precalc_k, n_nodes, n_kmers, k


def write_index_file(path: str, cols, ssup, C_array, precalc: Optional[np.ndarray], precalc_k: int, n_nodes: int,
                     n_kmers: int, k: int) -> None:
    cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in cols]
    s = np.ascontiguousarray(ssup, dtype=np.uint64) if ssup is not None else None
    pc = np.ascontiguousarray(precalc, dtype=np.int64) if precalc is not None and precalc_k else None
    Carr = (C.c_int64 * 4)(*[int(x) for x in C_array])
    rc = lib().sbwthost_file_write(path.encode(), n_nodes, cols[0].ctypes.data, cols[1].ctypes.data,
                                   cols[2].ctypes.data, cols[3].ctypes.data, s.ctypes.data if s is not None else None,
                                   Carr, pc.ctypes.data if pc is not None else None, precalc_k, n_kmers, k)
    if rc != 0:
        raise RuntimeError(_err())


def read_index_file(path: str) -> IndexFile:
    L = lib()
    h = C.c_void_p()
    if L.sbwthost_file_read(path.encode(), C.byref(h)) != 0:
        raise RuntimeError(_err())
    try:
        n, nk, k, p, hs = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        Carr = (C.c_int64 * 4)()
        L.sbwthost_file_info(h, C.byref(n), C.byref(nk), C.byref(k), C.byref(p), Carr, C.byref(hs))
        nw = (n.value + 63) // 64
        cols = [np.ctypeslib.as_array(L.sbwthost_file_words(h, c), shape=(nw,)).copy() for c in range(4)]
        ssup = np.ctypeslib.as_array(L.sbwthost_file_words(h, 4), shape=(nw,)).copy() if hs.value else None
        precalc = None
        if p.value:
            precalc = np.ctypeslib.as_array(L.sbwthost_file_precalc(h), shape=(4 ** p.value, 2)).copy()
        return IndexFile(cols, ssup, [Carr[i] for i in range(4)], precalc, p.value, n.value, nk.value, k.value)
    finally:
        L.sbwthost_file_free(h)


def read_sequences_chunked(path: str, chunk_bytes: int, n_threads: int):
    """The same reads through the CLI's chunked reader for plain regular files; None when the file cannot be cut."""
    L = lib()
    pb, po, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    rc = L.sbwthost_read_sequences_chunked(path.encode(), chunk_bytes, n_threads, C.byref(pb), C.byref(po), C.byref(n))
    if rc == 1:
        return None
    if rc != 0:
        raise RuntimeError(_err())
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_int64)), shape=(n.value + 1,)).copy()
        total = int(off[-1])
        bases = (np.ctypeslib.as_array(C.cast(pb, C.POINTER(C.c_uint8)), shape=(total,)).copy()
                 if total else np.zeros(0, np.uint8))
        return bases, off
    finally:
        L.sbwthost_free(pb)
        L.sbwthost_free(po)


def read_sequences(path: str):
    """All reads of a FASTA/FASTQ(.gz) file: (bases uint8 array, read_off int64 array)."""
    L = lib()
    pb, po, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    if L.sbwthost_read_sequences(path.encode(), C.byref(pb), C.byref(po), C.byref(n)) != 0:
        raise RuntimeError(_err())
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_int64)), shape=(n.value + 1,)).copy()
        total = int(off[-1])
        bases = (np.ctypeslib.as_array(C.cast(pb, C.POINTER(C.c_uint8)), shape=(total,)).copy()
                 if total else np.zeros(0, np.uint8))
        return bases, off
    finally:
        L.sbwthost_free(pb)
        L.sbwthost_free(po)


def write_file(path: str, data: bytes, gzip_output: bool = False, n_threads: int = 0) -> None:
    """Writes bytes through the CLI's buffered writer (parallel multi-member gzip when gzip_output)."""
    if lib().sbwthost_write_file(path.encode(), data, len(data), int(gzip_output), n_threads) != 0:
        raise RuntimeError(_err())


def rank_batch(bits: np.ndarray, n_bits: int, pos) -> np.ndarray:
    """Host rank directory of the scalar API (rank_support_v5 layout): ones in bits[0, pos) for every position."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    out = np.empty(len(pos), dtype=np.int64)
    if lib().sbwthost_rank_batch(bits.ctypes.data, n_bits, pos.ctypes.data, len(pos), out.ctypes.data) != 0:
        raise RuntimeError(_err())
    return out


def colors_write(path: str, rows, n_colors: int, k: int) -> None:
    """Writes a colour matrix (one uint64 row per column of its index) as a colour file (include/sbwthost.h)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if lib().sbwthost_colors_write(path.encode(), rows.ctypes.data if len(rows) else None, len(rows), n_colors, k) != 0:
        raise RuntimeError(_err())


def colors_read(path: str):
    """(rows uint64[n_columns], n_colors, k) of a colour file."""
    L = lib()
    n, nc, k = C.c_int64(), C.c_int64(), C.c_int64()
    if L.sbwthost_colors_read(path.encode(), C.byref(n), C.byref(nc), C.byref(k), None, 0) != 0:
        raise RuntimeError(_err())
    rows = np.zeros(n.value, dtype=np.uint64)
    if L.sbwthost_colors_read(path.encode(), C.byref(n), C.byref(nc), C.byref(k), rows.ctypes.data if n.value else None, n.value) != 0:
        raise RuntimeError(_err())
    return rows, nc.value, k.value


def colors_write_wide(path: str, rows, n_colors: int, k: int) -> None:
    """Writes a wide colour matrix ((n_columns, ceil(n_colors / 64)) uint64 words) as an "SBWTCOL2" file (include/sbwthost.h)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    words = (n_colors + 63) // 64
    if rows.ndim != 2 or (1 <= n_colors <= 4096 and rows.shape[1] != words):
        raise RuntimeError("rows of shape %s, %d colours need %d words a row" % (rows.shape, n_colors, words))
    if lib().sbwthost_colors_write_wide(path.encode(), rows.ctypes.data if rows.size else None, rows.shape[0], n_colors, k) != 0:
        raise RuntimeError(_err())


def colors_read_wide(path: str):
    """(rows uint64[n_columns, words_per_row], n_colors, k) of an "SBWTCOL2" or "SBWTCOL1" colour file."""
    L = lib()
    n, nc, k, w = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    if L.sbwthost_colors_read_wide(path.encode(), C.byref(n), C.byref(nc), C.byref(k), C.byref(w), None, 0) != 0:
        raise RuntimeError(_err())
    rows = np.zeros((n.value, w.value), dtype=np.uint64)
    if L.sbwthost_colors_read_wide(path.encode(), C.byref(n), C.byref(nc), C.byref(k), C.byref(w), rows.ctypes.data if rows.size else None,
                                   rows.size) != 0:
        raise RuntimeError(_err())
    return rows, nc.value, k.value


def colorsets_write(path: str, ids, table, n_colors: int, k: int) -> None:
    """Writes a colour-set object (ids uint32[n_columns], table uint64[n_sets, ceil(n_colors / 64)]) as an "SBWTCOL3" file
    (include/sbwthost.h); an object that breaks an invariant is refused."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    table = np.ascontiguousarray(table, dtype=np.uint64)
    words = (n_colors + 63) // 64
    if ids.ndim != 1 or table.ndim != 2 or (1 <= n_colors <= 4096 and table.shape[1] != words):
        raise RuntimeError("ids of shape %s and a table of shape %s, %d colours need %d words a row" % (ids.shape, table.shape, n_colors, words))
    if lib().sbwthost_colorsets_write(path.encode(), ids.ctypes.data if len(ids) else None, table.ctypes.data if table.size else None,
                                      len(ids), n_colors, k, table.shape[0]) != 0:
        raise RuntimeError(_err())


def colorsets_read(path: str):
    """(ids uint32[n_columns], table uint64[n_sets, words_per_row], n_colors, k) of an "SBWTCOL3" colour-set file."""
    L = lib()
    n, nc, k, w, ns = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    sizes = (C.byref(n), C.byref(nc), C.byref(k), C.byref(w), C.byref(ns))
    if L.sbwthost_colorsets_read(path.encode(), *sizes, None, 0, None, 0) != 0:
        raise RuntimeError(_err())
    ids = np.empty(n.value, dtype=np.uint32)
    table = np.empty((ns.value, w.value), dtype=np.uint64)
    if L.sbwthost_colorsets_read(path.encode(), *sizes, ids.ctypes.data if n.value else None, n.value, table.ctypes.data, table.size) != 0:
        raise RuntimeError(_err())
    return ids, table, nc.value, k.value


def positions_write(path: str, first, k: int, seq_color, seq_len) -> None:
    """Writes a position table (first uint64[n_columns]) with its sequence list as an "SBWTPOS1" file (include/sbwthost.h)."""
    first = np.ascontiguousarray(first, dtype=np.uint64)
    seq_color = np.ascontiguousarray(seq_color, dtype=np.int32)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.int64)
    if len(seq_color) != len(seq_len):
        raise RuntimeError("%d colours for %d lengths" % (len(seq_color), len(seq_len)))
    if lib().sbwthost_positions_write(path.encode(), first.ctypes.data if len(first) else None, len(first), k,
                                      seq_color.ctypes.data if len(seq_len) else None, seq_len.ctypes.data if len(seq_len) else None,
                                      len(seq_len)) != 0:
        raise RuntimeError(_err())


def positions_read(path: str):
    """(first uint64[n_columns], k, seq_color int32[n_seqs], seq_len int64[n_seqs]) of an "SBWTPOS1" position file."""
    L = lib()
    n, k, ns = C.c_int64(), C.c_int64(), C.c_int64()
    sizes = (C.byref(n), C.byref(k), C.byref(ns))
    if L.sbwthost_positions_read(path.encode(), *sizes, None, None, 0, None, 0) != 0:
        raise RuntimeError(_err())
    first = np.empty(max(n.value, 1), dtype=np.uint64)
    col, ln = np.empty(max(ns.value, 1), dtype=np.int32), np.empty(max(ns.value, 1), dtype=np.int64)
    if L.sbwthost_positions_read(path.encode(), *sizes, col.ctypes.data, ln.ctypes.data, ns.value, first.ctypes.data, n.value) != 0:
        raise RuntimeError(_err())
    return first[: n.value], k.value, col[: ns.value], ln[: ns.value]


def occurrences_write(path: str, off, occ, k: int, seq_color, seq_len) -> None:
    """Writes an occurrence table (off uint64[n_columns + 1], occ uint64[off[-1]]) with its sequence list as an "SBWTOCC1" file
    (include/sbwthost.h)."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    occ = np.ascontiguousarray(occ, dtype=np.uint64)
    seq_color = np.ascontiguousarray(seq_color, dtype=np.int32)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.int64)
    if len(seq_color) != len(seq_len):
        raise RuntimeError("%d colours for %d lengths" % (len(seq_color), len(seq_len)))
    if len(off) < 1:
        raise RuntimeError("off needs n_columns + 1 entries")
    if lib().sbwthost_occurrences_write(path.encode(), off.ctypes.data, occ.ctypes.data if len(occ) else None, len(off) - 1, k, len(occ),
                                        seq_color.ctypes.data if len(seq_len) else None, seq_len.ctypes.data if len(seq_len) else None,
                                        len(seq_len)) != 0:
        raise RuntimeError(_err())


def occurrences_read(path: str):
    """(off uint64[n_columns + 1], occ uint64[n_occ], k, seq_color int32[n_seqs], seq_len int64[n_seqs]) of an "SBWTOCC1" file."""
    L = lib()
    n, k, ns, no = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    sizes = (C.byref(n), C.byref(k), C.byref(ns), C.byref(no))
    if L.sbwthost_occurrences_read(path.encode(), *sizes, None, None, 0, None, 0, None, 0) != 0:
        raise RuntimeError(_err())
    off, occ = np.empty(n.value + 1, dtype=np.uint64), np.empty(max(no.value, 1), dtype=np.uint64)
    col, ln = np.empty(max(ns.value, 1), dtype=np.int32), np.empty(max(ns.value, 1), dtype=np.int64)
    if L.sbwthost_occurrences_read(path.encode(), *sizes, col.ctypes.data, ln.ctypes.data, ns.value, off.ctypes.data, n.value + 1,
                                   occ.ctypes.data, no.value) != 0:
        raise RuntimeError(_err())
    return off, occ[: no.value], k.value, col[: ns.value], ln[: ns.value]
