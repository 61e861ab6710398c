"""The colour-set builder (include/sbwtgpu.h, "the builder") in plain Python: ids, table, cnt, the
mark set of the open colour, close and finish as sbwt_colorsets.hip does them, rows being Python integers of any width as in
tests/colorsets_brute.py.  The model also counts what its closes did and says what the builder holds on the device.  Nothing
here needs a GPU."""
from __future__ import annotations

import random
from collections import Counter
from typing import Iterable, List, Optional, Tuple

FIRST_CAPACITY = 64
NEW, OPEN, CLOSED = 0, 1, 2


class Refused(ValueError):
    pass


class Builder:
    """n columns, n_colors colours.  add(color, columns) marks columns for a colour, which opens (closing the colour that was
    open); a closed colour is refused.  order: a random.Random that shuffles the order in which a close hands out new ids --
    finish fixes the numbering, so the result may not depend on it."""

    def __init__(self, n: int, n_colors: int, order: Optional[random.Random] = None):
        self.n, self.n_colors, self.words = n, n_colors, (n_colors + 63) // 64
        self.ids: List[int] = [0] * n
        self.table: List[int] = [0]
        self.cnt: List[int] = [n]
        self.cap = FIRST_CAPACITY
        self.marks = set()
        self.state = [NEW] * n_colors
        self.open: Optional[int] = None
        self.per_color = [0] * n_colors
        self.n_colored = 0
        self.order = order
        self.finished = False
        # what the closes did: sets appended from the empty set, sets split, rows changed in place; times the table grew
        self.from_empty = self.split = self.in_place = self.grown = 0

    # ---- the calls ----
    def add(self, color: int, columns: Iterable[int]) -> None:
        if self.finished:
            raise Refused("finish has consumed the builder")
        if not 0 <= color < self.n_colors:
            raise Refused("color out of range")
        if self.state[color] == CLOSED:
            raise Refused("the sequences of one colour must come in consecutive calls")
        if self.open != color:
            self.close()
            self.open = color
            self.state[color] = OPEN
        columns = set(columns)
        assert all(0 <= j < self.n for j in columns)
        self.marks |= columns

    def close(self) -> None:
        """Merges the open colour's marks: every marked column's set becomes its old set + the colour."""
        if self.open is None:
            return
        c, bit = self.open, 1 << self.open
        assert all(not row & bit for row in self.table)                 # a closed colour is never reopened
        hit = Counter(self.ids[j] for j in self.marks)                  # count
        olds = sorted(hit)
        if self.order is not None:
            self.order.shuffle(olds)
        remap = {}
        for old in olds:                                                # plan
            h = hit[old]
            if old != 0 and h == self.cnt[old]:
                self.table[old] |= bit                                  # every column of the set moves: in place
                self.in_place += 1
            else:
                remap[old] = len(self.table)
                self.table.append(self.table[old] | bit)
                self.cnt.append(h)
                self.cnt[old] -= h
                if old == 0:
                    self.from_empty += 1
                    self.n_colored += h
                else:
                    self.split += 1
        while self.cap < len(self.table):
            self.cap *= 2
            self.grown += 1
        for j in self.marks:                                            # move
            self.ids[j] = remap.get(self.ids[j], self.ids[j])
        self.per_color[c] = len(self.marks)
        self.marks = set()
        self.state[c] = CLOSED
        self.open = None

    def finish(self) -> Tuple[List[int], List[int]]:
        """(ids, table) in canonical form: the sets numbered by the smallest column that carries them."""
        self.close()
        first = {}
        for j, i in enumerate(self.ids):
            if i != 0:
                first.setdefault(i, j)
        assert sorted(first) == list(range(1, len(self.table)))         # every row but 0 is in use
        new_id = {0: 0}
        for rank, i in enumerate(sorted(first, key=first.get)):
            new_id[i] = 1 + rank
        table = [0] * len(self.table)
        for i, row in enumerate(self.table):
            table[new_id[i]] = row
        self.finished = True
        return [new_id[i] for i in self.ids], table

    # ---- what info reports, and what must hold after every close ----
    def info(self) -> dict:
        return {"n_sets": len(self.table), "n_colored_columns": self.n_colored, "per_color": list(self.per_color),
                "device_bytes": 4 * self.n + 8 * ((self.n + 63) // 64) + self.cap * (8 * self.words + 4)}

    def check(self) -> None:
        """the table's rows are pairwise distinct, every row but 0 is in use, cnt counts the columns of every id"""
        assert self.table[0] == 0 and len(set(self.table)) == len(self.table)
        used = Counter(self.ids)
        assert [used.get(i, 0) for i in range(len(self.table))] == self.cnt
        assert all(self.cnt[i] > 0 for i in range(1, len(self.table)))
        assert self.n_colored == self.n - self.cnt[0]
        assert len(self.table) <= self.cap


def build(n: int, n_colors: int, adds, order: Optional[random.Random] = None, check: bool = True):
    """adds: (colour, columns) in call order.  Returns (ids, table, builder)."""
    b = Builder(n, n_colors, order)
    for color, columns in adds:
        was = b.open
        b.add(color, columns)
        if check and was != b.open:
            b.check()
    ids, table = b.finish()
    if check:
        b.check()
    return ids, table, b
