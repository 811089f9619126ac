"""Numpy restatement of the live corpus (include/maxsim.h: msim_live_*, colpali_amd/live.py), independent of colpali_amd.

Slots: a page's slot is its arrival number; its id is id_base + slot, never reused.  `alive[c] == 0` marks a deleted slot.
Compaction: new off[c] = the sum of the lengths of the LIVE slots before c (a slot's length is off[c + 1] - off[c]; a slot that was
compacted away earlier has length 0), so a deleted slot becomes an empty page; live rows keep their order and move down.
Mask: scores[:, c] = -inf where alive[c] == 0.
"""
import numpy as np


class SlotTable:
    """The host bookkeeping of a live corpus: lengths per slot as the blob holds them now, and the tombstones."""

    def __init__(self, id_base=0):
        self.id_base = id_base
        self.lengths = []        # rows each slot owns in the blob now
        self.alive = []

    def add(self, lens):
        first = len(self.lengths)
        for n in lens:
            if n <= 0:
                raise ValueError("a page of 0 rows")
            self.lengths.append(int(n))
            self.alive.append(True)
        return [self.id_base + first + i for i in range(len(lens))]

    def delete(self, ids):
        slots = [i - self.id_base for i in ids]
        for j, s in enumerate(slots):
            if not (0 <= s < len(self.alive)) or not self.alive[s] or s in slots[:j]:
                raise KeyError(s + self.id_base)
        for s in slots:
            self.alive[s] = False

    def compact(self):
        self.lengths = [n if a else 0 for n, a in zip(self.lengths, self.alive)]

    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)

    def survivors(self):
        """Slots of the live pages, in slot order: position p of the packed survivors is slot survivors()[p]."""
        return [s for s, a in enumerate(self.alive) if a]

    @property
    def rows_used(self):
        return int(sum(self.lengths))


def compact_offsets(off, alive):
    """New offsets int64 [n + 1] after compaction."""
    off = np.asarray(off, dtype=np.int64)
    lens = np.where(np.asarray(alive).astype(bool), off[1:] - off[:-1], 0)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def move_list(off, alive):
    """(source row, destination row, rows) of every live page that changes place, in slot order."""
    off = np.asarray(off, dtype=np.int64)
    new = compact_offsets(off, alive)
    return [(int(off[c]), int(new[c]), int(off[c + 1] - off[c])) for c in range(len(off) - 1)
            if alive[c] and off[c + 1] > off[c] and off[c] != new[c]]


def compact_rows(rows, off, alive):
    """The row array after compaction (rows beyond the new total keep whatever they held: only the prefix is specified)."""
    out = np.array(rows, copy=True)
    for src, dst, n in move_list(off, alive):            # slot order, each destination at or below its source: a plain forward copy
        out[dst:dst + n] = np.array(rows[src:src + n], copy=True)
    return out


def moved_bytes(off, alive, row_bytes):
    """Bytes the bounce scheme must move: 2 reads + 2 writes of every row that changes place."""
    return 4 * row_bytes * sum(n for _, _, n in move_list(off, alive))


def mask(scores, alive):
    out = np.array(scores, dtype=np.float32, copy=True)
    out[:, ~np.asarray(alive).astype(bool)[:out.shape[1]]] = -np.inf
    return out


def expected_ids(ref_ids, survivors, id_base=0):
    """Ids of a search over the packed survivors (positions, -1 = padding) mapped back to slot ids."""
    ref_ids = np.asarray(ref_ids, dtype=np.int64)
    table = np.asarray(list(survivors) + [0], dtype=np.int64) + id_base
    return np.where(ref_ids >= 0, table[np.clip(ref_ids, 0, len(table) - 1)], -1)
