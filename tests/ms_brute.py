"""Definition-level matching statistics and LCS array on top of bruteforce.BruteSBWT (tiny inputs only).

Labels are BruteSBWT.nodes (dummies without their '$' padding), in colex order, so "'$' never counts" holds by construction.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

from bruteforce import BruteSBWT

ACGT = set(b"ACGT")


def lcs_array(B: BruteSBWT) -> List[int]:
    out = [0]
    for a, b in zip(B.nodes, B.nodes[1:]):
        d = 0
        while d < min(len(a), len(b)) and a[-1 - d] == b[-1 - d]:
            d += 1
        out.append(d)
    return out


def suffix_intervals(B: BruteSBWT) -> Dict[str, Tuple[int, int]]:
    """Every suffix of every label (the empty one included) -> (first, last) column of the labels that end with it."""
    iv: Dict[str, List[int]] = {}
    for j, lab in enumerate(B.nodes):
        for d in range(len(lab) + 1):
            w = lab[len(lab) - d:]
            e = iv.setdefault(w, [j, j, 0])
            e[0], e[1], e[2] = min(e[0], j), max(e[1], j), e[2] + 1
    for w, (f, l, cnt) in iv.items():
        assert l - f + 1 == cnt, ("labels ending with %r are not contiguous" % w)
    return {w: (f, l) for w, (f, l, _) in iv.items()}


class BruteMS:
    def __init__(self, B: BruteSBWT):
        self.B = B
        self.k = B.k
        self.iv = suffix_intervals(B)

    def read(self, s: bytes):
        """(len, first, second) lists for one read."""
        k = self.k
        n = len(self.B.nodes)
        L, F, S = [], [], []
        run = 0
        for i, ch in enumerate(s):
            run = run + 1 if ch in ACGT else 0
            d = min(k, run)
            while d > 0 and s[i - d + 1:i + 1].decode() not in self.iv:
                d -= 1
            f, l = self.iv[s[i - d + 1:i + 1].decode()] if d > 0 else (0, n - 1)
            L.append(d)
            F.append(f)
            S.append(l)
        return L, F, S


def probe_reads(seqs, k, rng):
    """Exact substrings, substitutions, N / lower case / NUL / other bytes, short and empty reads, low complexity."""
    reads = []
    for s in seqs:
        reads.append(s.encode())
        a = rng.randrange(0, max(1, len(s) - 5))
        reads.append(s[a:a + rng.randint(1, 3 * k + 5)].encode())
        m = bytearray(s.encode())
        for _ in range(max(1, len(m) // 10)):
            m[rng.randrange(len(m))] = ord(rng.choice("ACGT"))
        reads.append(bytes(m))
    m = bytearray(seqs[0].encode())
    for j, ch in enumerate(b"NacgtN\x00\xff$Z"):
        if len(m):
            m[(7 * j + 3) % len(m)] = ch
    reads += [bytes(m), b"", b"A", b"AC"[: max(0, k - 1)], b"A" * (3 * k + 7), b"AC" * (2 * k + 3), b"ACGTTGCA" * 9,
              b"N" * 5, b"\x00ACGT\x00", "".join(rng.choice("ACGT") for _ in range(4 * k + 20)).encode(), b""]
    return reads


def format_ms(lens, first=None, second=None) -> bytes:
    """The CLI's line for one read: one token per base, each followed by a space, then a newline."""
    if first is None:
        return b"".join(b"%d " % int(d) for d in lens) + b"\n"
    return b"".join(b"%d,%d,%d " % (int(d), int(f), int(s)) for d, f, s in zip(lens, first, second)) + b"\n"
