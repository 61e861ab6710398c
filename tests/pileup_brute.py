"""The definition of "pileup of aligned reads" (include/sbwtgpu.h) in pure Python on top of
tests/align_brute.py: the filter, the per-base records built column by column in a dict (no difference array: it shares no trick
with the kernel), the scalars, the calls as a plain loop and the two TSV formats of the CLI.

A per-base record is the tuple (depth, nA, nC, nG, nT, n_del, n_ins, n_other); a call is (pos, seq, allele, ref, depth, count,
ref_count); a filter is (min_votes, require_unique, max_edit); the votes of a read are (votes, votes2)."""
import align_brute as ab
import verify_brute as vb

CODE = {65: 0, 67: 1, 71: 2, 84: 3}
DEL, INS = 4, 5
ALLELE_TEXT = "ACGT-+"
NO_FILTER = (0, 0, -1)
JUNK_VOTES = (0x5A5A5A5A, 0x5A5A5A5A)       # what test_gpu_verify.map_records leaves in votes and votes2
SCALARS = ("n_offered", "n_piled", "n_columns", "n_clipped", "n_overhang")
EMPTY = (0, 0, 0, 0, 0, 0, 0, 0)
DEPTH, N_DEL, N_INS, N_OTHER = 0, 5, 6, 7


def is_piled(n_seqs: int, seq: int, votes, edit: int, n_ops: int, filt) -> bool:
    min_votes, require_unique, max_edit = filt
    return (n_ops > 0 and 0 <= seq < n_seqs and votes[0] >= min_votes and (require_unique == 0 or votes[0] > votes[1])
            and (max_edit < 0 or edit <= max_edit))


class Pile:
    """The pileup of what has been added so far on the sequences refs (byte strings)."""

    def __init__(self, refs, n_seqs=None):
        self.refs = refs
        self.n_seqs = len(refs) if n_seqs is None else n_seqs
        self.reset()

    def reset(self):
        self.base = {}                          # (seq, p) -> the record as a list
        for s in SCALARS:
            setattr(self, s, 0)
        self.overhang_columns = 0               # the part of n_overhang that is columns (the rest: anchors of I runs)

    def _at(self, seq, p):
        return self.base.setdefault((seq, p), [0] * 8)

    def add_alignment(self, read: bytes, rec, votes, verify, align, runs, filt=NO_FILTER):
        """one read with its map record (seq, strand, start), its votes, and what the align call gives for it"""
        self.n_offered += 1
        seq, strand, _ = rec
        if not is_piled(self.n_seqs, seq, votes, verify[2], align[1], filt):
            return False
        self.n_piled += 1
        ref, n, r = self.refs[seq], len(self.refs[seq]), vb.orient(read, strand)
        p, j = align[0], 0
        for k, (length, op) in enumerate(runs):
            if op == "I":
                if k == 0 or k == len(runs) - 1:
                    self.n_clipped += length
                elif 0 <= p - 1 < n:
                    self._at(seq, p - 1)[N_INS] += 1
                else:
                    self.n_overhang += 1
                j += length
                continue
            for _ in range(length):
                if not 0 <= p < n:
                    assert op in "XD", (op, p)              # a coordinate outside the sequence matches nothing
                    self.n_overhang += 1
                    self.overhang_columns += 1
                else:
                    c = self._at(seq, p)
                    c[DEPTH] += 1
                    self.n_columns += 1
                    if op == "=":
                        assert vb.matches(ref, p, r[j])
                        c[1 + CODE[ref[p]]] += 1
                    elif op == "X":
                        c[N_OTHER if r[j] is None else 1 + CODE[r[j]]] += 1
                    else:
                        c[N_DEL] += 1
                p += 1
                if op != "D":
                    j += 1
        assert j == len(read) and p == verify[0], (j, p, verify)
        return True

    def add(self, reads, recs, band: int, votes=None, filt=NO_FILTER, alns=None):
        """a batch: verified and aligned by the brute force (alns: ab.alignments' result, when the caller has it), then piled"""
        alns = ab.alignments(self.refs, reads, recs, band) if alns is None else alns
        votes = [JUNK_VOTES] * len(reads) if votes is None else votes
        return [self.add_alignment(rd, rc, vt, v, a, runs, filt) for rd, rc, vt, (v, a, runs) in zip(reads, recs, votes, alns)]

    def record(self, seq: int, p: int):
        return tuple(self.base.get((seq, p), EMPTY))

    def counts(self, seq: int, pos: int = 0, length=None):
        n = len(self.refs[seq])
        length = n - pos if length is None else length
        return [self.record(seq, p) for p in range(pos, pos + length)]

    def scalars(self) -> dict:
        return {s: getattr(self, s) for s in SCALARS}

    def info(self) -> dict:
        return dict(self.scalars(), n_seqs=self.n_seqs, total_bases=sum(len(r) for r in self.refs[:self.n_seqs]))

    def calls(self, min_depth: int = 1, min_alt: int = 1, min_frac_ppm: int = 0):
        assert min_depth >= 1 and min_alt >= 1 and 0 <= min_frac_ppm <= 10 ** 6
        out = []
        for seq in range(self.n_seqs):
            ref = self.refs[seq]
            for p in range(len(ref)):
                if not vb.valid(ref[p]):
                    continue
                c = self.record(seq, p)
                rc = CODE[ref[p]]
                for a in range(6):
                    if a == rc:
                        continue
                    cnt = c[1 + a] if a < 4 else (c[N_DEL] if a == DEL else c[N_INS])
                    if c[DEPTH] >= min_depth and cnt >= min_alt and cnt * 10 ** 6 >= min_frac_ppm * c[DEPTH]:
                        out.append((p, seq, a, rc, c[DEPTH], cnt, c[1 + rc]))
        return out

    # ---- the CLI's two files ----------------------------------------------------------------------------------------------
    def header_line(self) -> str:
        i = self.info()
        return "# " + " ".join("%s=%d" % (k, i[k]) for k in ("n_seqs", "total_bases") + SCALARS) + "\n"

    def pile_tsv(self) -> str:
        """seq pos ref depth A C G T del ins other, one line per base with depth > 0; ref is N at an invalid base"""
        lines = [self.header_line()]
        for seq in range(self.n_seqs):
            ref = self.refs[seq]
            for p in range(len(ref)):
                c = self.record(seq, p)
                if c[DEPTH] > 0:
                    lines.append("\t".join(str(x) for x in (seq, p, chr(ref[p]) if vb.valid(ref[p]) else "N") + c) + "\n")
        return "".join(lines)

    def calls_tsv(self, min_depth: int = 1, min_alt: int = 1, min_frac_ppm: int = 0) -> str:
        """seq pos ref alt depth count, alt one of A C G T - +"""
        lines = [self.header_line()]
        for p, seq, a, rc, depth, cnt, _ in self.calls(min_depth, min_alt, min_frac_ppm):
            lines.append("%d\t%d\t%s\t%s\t%d\t%d\n" % (seq, p, ALLELE_TEXT[rc], ALLELE_TEXT[a], depth, cnt))
        return "".join(lines)


def check_properties(pile: Pile, span_sum: int):
    """the listed properties of the records of a pileup; span_sum: the sum of ref_end - ref_begin over the piled reads"""
    total = 0
    for (seq, p), c in pile.base.items():
        assert 0 <= p < len(pile.refs[seq])
        assert c[DEPTH] == sum(c[1:5]) + c[N_DEL] + c[N_OTHER], (seq, p, c)
        assert c[N_INS] <= c[DEPTH], (seq, p, c)
        total += c[DEPTH]
    assert total == pile.n_columns and total + pile.overhang_columns == span_sum, (total, pile.n_columns, pile.overhang_columns, span_sum)
