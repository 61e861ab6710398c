"""The colour layer's definitions in numpy, for indexes of millions of columns (include/sbwtgpu.h, "colours and
pseudoalignment", "wide colour matrices", "colour sets", "the builder"), and the scale world they are applied to.

At most 64 colours are USED: a column's colours are one uint64 key, bit i for used colour i, and a `place` (an increasing list
of real colour numbers, one per used colour) says where bit i lies among the n_colors colours of an object.  From the keys
alone come the canonical (ids, table) of any n_colors, the wide matrix, per_color, n_colored_columns and n_sets; from the
keys and the search results of a batch its records, colour words and counts.  Search results come from the oracle
(tests/oracle.py), which shares no code with the GPU search.  Held against the brute forces of tests/pseudoalign_brute.py,
tests/pseudoalign_wide.py and tests/colorsets_brute.py in tests/test_colors_scale_ref_cpu.py.

Nothing here needs a GPU, and nothing here imports the GPU binding."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from oracle import OracleIndex
from sbwt_amd import synth

K = 31
N_USED = 20
SEGMENT = 256
QUERIES = ((1_000_000, 0), (500_000, 1), (1, 0))
# the records of the 64-colour call and of the wide calls, as the binding declares them
PSEUDOALIGNMENT_DTYPE = np.dtype([("colors", np.uint64), ("n_kmers", np.int32), ("n_found", np.int32)])
READ_FOUND_DTYPE = np.dtype([("n_kmers", np.int32), ("n_found", np.int32)])

_COMP = np.arange(256, dtype=np.uint8)
_COMP[list(b"ACGT")] = list(b"TGCA")
_ONE = np.uint64(1)


def n_words(n_colors: int) -> int:
    return (n_colors + 63) // 64


def concat(seqs: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """(bases, off) of byte arrays"""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return (np.concatenate(seqs) if len(seqs) else np.zeros(0, dtype=np.uint8)), off


def out_offsets(off: np.ndarray, k: int) -> np.ndarray:
    """Window offsets: a read of L bases has max(L - k + 1, 0) windows."""
    oo = np.zeros(len(off), dtype=np.int64)
    np.cumsum(np.maximum(np.diff(off) - k + 1, 0), out=oo[1:])
    return oo


def revcomp_batch(bases: np.ndarray, off: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The whole batch reverse-complemented (A <-> T, C <-> G on upper-case bytes, every other byte kept): the reads in
    reverse order, so that the windows of the result, read backwards, are the windows of the batch."""
    return _COMP[bases[::-1]], int(off[-1]) - off[::-1]


# ---- search results from the oracle ---------------------------------------------------------------------------------------
def strict_oracle(bits, k: int) -> OracleIndex:
    """The oracle WITHOUT the streaming-support marks: every window is then searched on its own with the raw byte
    validated, the rule of sbwtgpu_search_batch (a window holding anything but upper-case ACGT is no hit).  With the marks the
    reference's streaming step upper-cases the byte it steps by, and a lower-case base would count as a hit."""
    return OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], None, bits.n_nodes, k, bits.n_kmers, 8)


class Results(NamedTuple):
    off: np.ndarray                  # window offsets of the reads
    res: np.ndarray                  # column of every window, -1: no hit
    res2: Optional[np.ndarray]       # two strands: column of every window's reverse complement


_IS_ACGT = np.zeros(256, dtype=bool)
_IS_ACGT[list(b"ACGT")] = True


def search(orc: OracleIndex, bases: np.ndarray, off: np.ndarray, both: bool, n_threads: int) -> Results:
    """An oracle with marks (the streaming search, several times as fast) serves batches of upper-case ACGT only, where
    the two searches agree."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    assert not orc.has_streaming_support or _IS_ACGT[bases].all()
    off = np.ascontiguousarray(off, dtype=np.int64)
    oo = out_offsets(off, orc.k)
    res, _ = orc.batch_search(bases, off, oo, n_threads)
    res2 = None
    if both:
        rb, ro = revcomp_batch(bases, off)
        back, _ = orc.batch_search(rb, ro, out_offsets(ro, orc.k), n_threads)
        res2 = back[::-1]
    assert res.min(initial=0) >= -1
    return Results(oo, res, res2)


# ---- keys ------------------------------------------------------------------------------------------------------------------
def mark(n: int, r: Results) -> Tuple[np.ndarray, Tuple[int, int]]:
    """What one add call colours: (a bool per column, (n_windows, n_hit_windows))."""
    m = np.zeros(n, dtype=bool)
    m[r.res[r.res >= 0]] = True
    hit = r.res >= 0
    if r.res2 is not None:
        m[r.res2[r.res2 >= 0]] = True
        hit = hit | (r.res2 >= 0)
    return m, (len(r.res), int(hit.sum()))


def fill_keys(n: int, marks: Sequence[Tuple[int, np.ndarray]]) -> np.ndarray:
    """marks: (used colour, bool per column) of every add call"""
    keys = np.zeros(n, dtype=np.uint64)
    for used, m in marks:
        assert 0 <= used < 64
        keys |= m.astype(np.uint64) << np.uint64(used)
    return keys


def restrict(keys: np.ndarray, used: Sequence[int]) -> np.ndarray:
    """The keys of a colouring in which only the colours `used` have been given."""
    return keys & np.uint64(sum(1 << i for i in used))


def scatter(keys: np.ndarray, place: Sequence[int], n_colors: int) -> np.ndarray:
    """(len(keys), W) words: bit i of a key at real colour place[i]"""
    assert list(place) == sorted(set(place)) and 0 <= place[0] and place[-1] < n_colors
    assert len(place) == 64 or not (keys >> np.uint64(len(place))).any()
    out = np.zeros((len(keys), n_words(n_colors)), dtype=np.uint64)
    for i, c in enumerate(place):
        out[:, c >> 6] |= ((keys >> np.uint64(i)) & _ONE) << np.uint64(c & 63)
    return out


def classes(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(ids, class keys): key 0 is class 0, the other distinct keys are numbered 1, 2, ... by their first column."""
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    nz = np.flatnonzero(uniq != 0)
    order = nz[np.argsort(first[nz], kind="stable")]
    new_id = np.zeros(len(uniq), dtype=np.uint32)
    new_id[order] = np.arange(1, len(order) + 1, dtype=np.uint32)
    return new_id[inv], np.concatenate([np.zeros(1, dtype=np.uint64), uniq[order]])


def canonical(keys: np.ndarray, place: Sequence[int], n_colors: int) -> Tuple[np.ndarray, np.ndarray]:
    """(ids uint32[n], table uint64[n_sets, W]) of the canonical colour-set object"""
    ids, class_keys = classes(keys)
    return ids, scatter(class_keys, place, n_colors)


def matrix(keys: np.ndarray, place: Sequence[int], n_colors: int) -> np.ndarray:
    """The wide matrix, (n, W) uint64."""
    uniq, inv = np.unique(keys, return_inverse=True)
    return scatter(uniq, place, n_colors)[inv.reshape(-1)]


def per_color(keys: np.ndarray, place: Sequence[int], n_colors: int) -> List[int]:
    out = [0] * n_colors
    for i, c in enumerate(place):
        out[c] = int(((keys >> np.uint64(i)) & _ONE).sum())
    return out


def n_colored_columns(keys: np.ndarray) -> int:
    return int((keys != 0).sum())


def n_sets(keys: np.ndarray) -> int:
    return 1 + len(np.setdiff1d(np.unique(keys), np.zeros(1, dtype=np.uint64)))


# ---- pseudoalignment -------------------------------------------------------------------------------------------------------
def window_rows(keys: np.ndarray, r: Results) -> np.ndarray:
    """The key of every window: the colours of its column, with two strands also those of its reverse complement's."""
    padded = np.concatenate([keys, np.zeros(1, dtype=np.uint64)])          # (-1 takes the zero behind the last column)
    rows = padded[r.res]
    if r.res2 is not None:
        rows = rows | padded[r.res2]
    return rows


def _per_read(values: np.ndarray, oo: np.ndarray) -> np.ndarray:
    """Sums over each read's windows (np.add.reduceat over the reads that have windows)."""
    out = np.zeros(len(oo) - 1, dtype=np.int64)
    some = np.flatnonzero(np.diff(oo) > 0)
    if len(some):
        out[some] = np.add.reduceat(values.astype(np.int32), oo[some])
    return out


class ReadCounts(NamedTuple):
    n_kmers: np.ndarray              # int64 per read
    n_found: np.ndarray
    count: np.ndarray                # (n_reads, used colours) int32: count_c


def read_counts(keys: np.ndarray, r: Results, n_used: int) -> ReadCounts:
    rows = window_rows(keys, r)
    count = np.empty((len(r.off) - 1, n_used), dtype=np.int32)
    for i in range(n_used):
        count[:, i] = _per_read((rows >> np.uint64(i)) & _ONE, r.off)
    return ReadCounts(np.diff(r.off), _per_read(rows != 0, r.off), count)


def part(rc: ReadCounts, lo: int, hi: int) -> ReadCounts:
    """reads lo .. hi - 1"""
    return ReadCounts(rc.n_kmers[lo:hi], rc.n_found[lo:hi], rc.count[lo:hi])


def expected(rc: ReadCounts, place: Sequence[int], n_colors: int, threshold_ppm: int, denominator: int, narrow: bool = False,
             counts: bool = False):
    """What the pseudoalign methods return: narrow (the 64-colour call) a PSEUDOALIGNMENT_DTYPE array, otherwise
    (READ_FOUND_DTYPE array, (n_reads, W) uint64 colour words); with counts also the (n_reads, n_colors) int32 array.  Colour c
    is in a read's colours exactly when D > 0 and count_c * 1 000 000 >= threshold_ppm * D, D = n_kmers or n_found."""
    n = len(rc.n_kmers)
    D = rc.n_kmers if denominator else rc.n_found
    words = np.zeros((n, n_words(n_colors)), dtype=np.uint64)
    for i, c in enumerate(place):
        on = (D > 0) & (rc.count[:, i].astype(np.int64) * 1_000_000 >= threshold_ppm * D)
        words[:, c >> 6] |= on.astype(np.uint64) << np.uint64(c & 63)
    rec = np.zeros(n, dtype=PSEUDOALIGNMENT_DTYPE if narrow else READ_FOUND_DTYPE)
    rec["n_kmers"], rec["n_found"] = rc.n_kmers, rc.n_found
    if narrow:
        assert n_colors <= 64
        rec["colors"] = words[:, 0]
    out = (rec,) if narrow else (rec, words)
    if counts:
        cnt = np.zeros((n, n_colors), dtype=np.int32)
        cnt[:, list(place)] = rc.count[:, :len(place)]
        out += (cnt,)
    return out[0] if len(out) == 1 else out


# ---- runs and iterations, as the reducers see them ---------------------------------------------------------------------------
def longest_run(rows: np.ndarray, oo: np.ndarray) -> int:
    """The longest run of one key over a read's FOUND windows (a miss neither counts nor ends a run: k_pa_reduce_sets keeps
    its pending key across windows without a hit)."""
    best = 0
    for r in np.flatnonzero(np.diff(oo) > 0):
        mine = rows[oo[r]:oo[r + 1]]
        mine = mine[mine != 0]
        if len(mine) <= best:
            continue
        cut = np.flatnonzero(mine[1:] != mine[:-1]) + 1
        best = max(best, int(np.diff(np.concatenate([[0], cut, [len(mine)]])).max()))
    return best


def most_keys_in_an_iteration(rows: np.ndarray, oo: np.ndarray, min_windows: int = 64) -> int:
    """The largest number of distinct non-zero keys among windows 64 i .. 64 i + 63 of one read."""
    best = 0
    for r in np.flatnonzero(np.diff(oo) >= min_windows):
        mine = rows[oo[r]:oo[r + 1]]
        mine = np.sort(mine[:len(mine) // 64 * 64].reshape(-1, 64), axis=1)
        distinct = (mine[:, 1:] != mine[:, :-1]).sum(axis=1) + (mine[:, 0] != 0)
        best = max(best, int(distinct.max()))
    return best


# ---- the scale world -------------------------------------------------------------------------------------------------------
def placement(n_colors: int) -> List[int]:
    """The real colours of the 20 used ones, increasing: the first and last bit of the first word, of the words in the middle
    and of the last word where they exist (0, 63, 64, 127, 128, n/2 - 1, n/2, the last word's first bit, n - 1), then the
    smallest numbers not yet taken."""
    assert n_colors >= N_USED
    half, last_word = n_colors // 2, (n_colors - 1) // 64 * 64
    place = {c for c in (0, 63, 64, 127, 128, half - 1, half, last_word, n_colors - 1) if 0 <= c < n_colors}
    c = 1
    while len(place) < N_USED:
        place.add(c)
        c += 1
    assert len(place) == N_USED
    return sorted(place)


class AddCall(NamedTuple):
    used: int
    bases: np.ndarray
    off: np.ndarray
    both: bool


class ScaleWorld:
    """k = 31, forward strands only: a random genome g0 of 1.2 Mbp and eight copies of it at 0.5 % divergence, all nine indexed
    (sequence 0 is g0).  Used colours 0 .. 6: sequences 0 .. 6, one add call each (colour 3 as the reverse complement of its
    sequence with both strands, so its hits come from the second strand's results); 7: sequences 7 and 8 in ONE call of more
    than 2^21 windows; 8 + b: every 256-position segment of g0 whose number has bit b set, b = 0 .. 11."""

    def __init__(self):
        self.k = K
        self.g0 = synth.random_genome(1_200_000, 1)
        self.strains = [synth.mutate(self.g0, 0.005, 100 + i) for i in range(8)]
        self.genomes = [self.g0] + self.strains

    def index_seqs(self) -> List[bytes]:
        return [g.tobytes() for g in self.genomes]

    def add_calls(self) -> List[AddCall]:
        seqs = self.genomes
        calls = []
        for i in range(7):
            s = synth.revcomp(seqs[i]) if i == 3 else seqs[i]
            calls.append(AddCall(i, *concat([s]), i == 3))
        calls.append(AddCall(7, *concat(seqs[7:9]), False))
        n_seg = (len(self.g0) + SEGMENT - 1) // SEGMENT
        assert n_seg < 2 * (1 << 12)
        for b in range(12):
            segs = [self.g0[SEGMENT * s:SEGMENT * (s + 1) + self.k - 1] for s in range(n_seg) if (s >> b) & 1]
            calls.append(AddCall(8 + b, *concat(segs), False))
        assert [c.used for c in calls] == list(range(N_USED))
        return calls

    def quiet_stretch(self) -> np.ndarray:
        """The longest piece of g0 inside one segment in which no strain differs from g0: every window of it is a k-mer
        of all nine sequences and of the same stripes, so all its windows carry one key."""
        differs = np.zeros(len(self.g0), dtype=np.int64)
        for s in self.strains:
            differs |= s != self.g0
        c = np.concatenate([[0], np.cumsum(differs)])
        p = np.arange(len(self.g0) - self.k + 1)
        quiet = (c[p + self.k] - c[p]) == 0                              # window p holds no difference
        edge = np.flatnonzero(~quiet | (p % SEGMENT == 0))               # a run ends at a difference or at a segment's start
        gaps = np.diff(np.concatenate([edge, [len(p)]]))
        at = int(np.argmax(gaps))
        a = int(edge[at]) + (0 if quiet[edge[at]] else 1)
        b = int(edge[at]) + int(gaps[at])
        assert b - a >= 100 and quiet[a:b].all() and a // SEGMENT == (b - 1) // SEGMENT
        return self.g0[a:b + self.k - 1]

    def main_batch(self) -> Tuple[np.ndarray, np.ndarray]:
        """100 000 reads of 150 bases with 1 % substitutions, 20 000 random reads, three reads of 1 000 000 bases cut from
        strains and mutated at 0.5 %, and one read that repeats a segment's 286 bases a thousand times -- a segment's 256
        windows share one key and the 30 windows across a joint miss, so the read is ONE run of 256 000 found windows (the
        stripes change the key of g0's windows every 256 positions: no piece of a strain gives a run longer than that);
        then N, lower-case, NUL and 0xFF bytes at 3 000 places each."""
        b1, o1 = synth.sample_reads(self.genomes, 100_000, 150, 0.01, 201)
        b2, o2 = synth.random_reads(20_000, 150, 202)
        rng = np.random.default_rng(203)
        longs = []
        for j in (1, 4, 7):
            a = int(rng.integers(0, len(self.g0) - 1_000_000))
            longs.append(synth.mutate(self.strains[j][a:a + 1_000_000], 0.005, 204 + j))
        longs.append(np.tile(self.quiet_stretch(), 1500))
        b3, o3 = concat(longs)
        bases = np.concatenate([b1, b2, b3])
        off = np.concatenate([o1, o2[1:] + o1[-1], o3[1:] + o1[-1] + o2[-1]])
        for j, ch in enumerate((ord("N"), ord("a"), ord("g"), 0, 0xFF)):
            bases = synth.inject(bases, 3000, ch, 210 + j)
        return bases, off

    def tiny_batch(self) -> Tuple[np.ndarray, np.ndarray]:
        """4 300 000 reads of 31 to 33 bases from the strains (one to three windows each), 0.2 % substitutions: more reads
        than the reducers' grid of 2^20 blocks x 4 waves takes in one trip."""
        return synth.ragged_reads(self.strains, 4_300_000, 31, 33, 0.002, 220)


class Reference:
    """The keys of the scale world's columns and what follows from them."""

    def __init__(self, world: ScaleWorld, orc: OracleIndex, strict: OracleIndex, n_threads: int):
        """orc: the oracle with marks, for the add calls and the tiny reads (upper-case ACGT only); strict: strict_oracle(),
        for the main batch with its dirty bytes."""
        assert orc.has_streaming_support and not strict.has_streaming_support and orc.n_nodes == strict.n_nodes
        self.world, self.orc, self.strict, self.nt, self.n = world, orc, strict, n_threads, int(orc.n_nodes)
        self.calls = world.add_calls()
        marks = []
        self.add_counts: List[Tuple[int, int]] = []
        for c in self.calls:
            m, cnt = mark(self.n, search(orc, c.bases, c.off, c.both, n_threads))
            marks.append((c.used, m))
            self.add_counts.append(cnt)
        self.keys = fill_keys(self.n, marks)
        # colours 0 .. 7 are given every indexed sequence in full: a column without a colour is a dummy column
        self.dummy = self.keys == 0
        self._uniq, self._inv = np.unique(self.keys, return_inverse=True)
        self._inv = self._inv.reshape(-1)
        self._bit_count = [int(((self.keys >> np.uint64(i)) & _ONE).sum()) for i in range(N_USED)]
        self._cache: Dict = {}

    # -- the keys restricted to some used colours, without a pass over the columns where the classes' keys say it all --
    def n_sets_of(self, used: Sequence[int]) -> int:
        return n_sets(restrict(self._uniq, used))

    def n_colored_of(self, used: Sequence[int]) -> int:
        u = restrict(self._uniq, used) != 0
        return int(u[self._inv].sum())

    def per_color_of(self, used: Sequence[int], place: Sequence[int], n_colors: int) -> List[int]:
        out = [0] * n_colors
        for i in used:
            out[place[i]] = self._bit_count[i]
        return out

    def canonical(self, n_colors: int):
        key = ("canonical", n_colors)
        if key not in self._cache:
            self._cache[key] = canonical(self.keys, placement(n_colors), n_colors)
        return self._cache[key]

    def matrix(self, n_colors: int) -> np.ndarray:
        return scatter(self._uniq, placement(n_colors), n_colors)[self._inv]

    # -- batches --
    def batch(self, name: str) -> Tuple[np.ndarray, np.ndarray]:
        if ("batch", name) not in self._cache:
            self._cache["batch", name] = getattr(self.world, name + "_batch")()
        return self._cache["batch", name]

    def counts(self, name: str, both: bool) -> ReadCounts:
        """n_kmers, n_found and count_c of a batch's reads (the two-strand search reuses the one-strand results)"""
        key = ("counts", name, both)
        if key not in self._cache:
            self._cache[key] = read_counts(self.keys, self.results(name, both), N_USED)
        return self._cache[key]

    def results(self, name: str, both: bool) -> Results:
        key = ("results", name, both)
        if key not in self._cache:
            bases, off = self.batch(name)
            orc = self.strict if name == "main" else self.orc
            if both and ("results", name, False) in self._cache:
                one = self._cache["results", name, False]
                rb, ro = revcomp_batch(bases, off)
                back, _ = orc.batch_search(rb, ro, out_offsets(ro, orc.k), self.nt)
                self._cache[key] = Results(one.off, one.res, back[::-1])
            else:
                self._cache[key] = search(orc, bases, off, both, self.nt)
        return self._cache[key]


def oracles(bits, k: int) -> Tuple[OracleIndex, OracleIndex]:
    """(the oracle with marks, the strict one) of an index's bits"""
    return (OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 8),
            strict_oracle(bits, k))
