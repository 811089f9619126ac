"""Numpy restatement of hard-negative mining (colpali_amd/mine.py, include/maxsim.h: msim_mine_*), independent of colpali_amd.

s fp32 [n_q, n]: the score matrix of the full scan; column c is page id_base + c.  positives: per query a list of GLOBAL ids (ids
outside [id_base, id_base + n), -1 among them, are ignored; duplicates are allowed).

    pos[q]      max of s[q, c] over the in-shard positives (those of live slots when `alive` is given), +inf when there is none
    eligible    c is not a positive of q;  alive is None or alive[c] != 0;  s[q, c] != -inf;
                max_ratio is None or not (s[q, c] > fp32(max_ratio) * pos[q])          -- one fp32 multiply, then the comparison
    order       the eligible columns by (score descending, id ascending)
    window      ranks skip_top .. skip_top + n_neg - 1 of that order; (-inf, -1) where fewer exist
"""
import numpy as np


def as_lists(positives, n_q):
    """Any of the three public forms (arrays on the host) -> a list of id lists: int [n_q], int [n_q, P], or (ids, offsets)."""
    if isinstance(positives, tuple):
        ids, off = (np.asarray(x) for x in positives)
        return [[int(i) for i in ids[off[q]:off[q + 1]]] for q in range(n_q)]
    p = np.asarray(positives)
    if p.ndim == 1:
        return [[int(p[q])] for q in range(n_q)]
    return [[int(i) for i in p[q]] for q in range(n_q)]


def positive_columns(pos_list, n, id_base=0):
    """Per query the sorted set of in-shard positive COLUMNS."""
    return [sorted({i - id_base for i in ids if i >= 0 and 0 <= i - id_base < n}) for ids in pos_list]


def bounds(s, pos_list, id_base=0, alive=None, none=np.inf):
    """pos[q] fp32 [n_q]; `none`: the value of a query without (live, in-shard) positives (+inf; -inf for one shard of several)."""
    s = np.asarray(s, dtype=np.float32)
    out = np.full((s.shape[0],), none, dtype=np.float32)
    for q, cols in enumerate(positive_columns(pos_list, s.shape[1], id_base)):
        cols = [c for c in cols if alive is None or alive[c]]
        if cols:
            out[q] = s[q, cols].max()
    return out


def eligible(s, pos_list, id_base=0, max_ratio=None, alive=None, pos=None):
    """bool [n_q, n].  `pos`: the bounds to use (default: `bounds` of this matrix; a sharded run passes the global ones)."""
    s = np.asarray(s, dtype=np.float32)
    n_q, n = s.shape
    ok = ~np.isneginf(s)
    if alive is not None:
        ok &= np.asarray(alive)[:n].astype(bool)[None, :]
    for q, cols in enumerate(positive_columns(pos_list, n, id_base)):
        ok[q, cols] = False
    if max_ratio is not None:
        if pos is None:
            pos = bounds(s, pos_list, id_base, alive)
        with np.errstate(invalid="ignore"):
            thresh = np.float32(max_ratio) * np.asarray(pos, dtype=np.float32)           # fp32 x fp32 -> fp32
            ok &= ~(s > thresh[:, None])
    return ok


def masked(s, pos_list, id_base=0, max_ratio=None, alive=None, pos=None):
    """The matrix after the mask: -inf in every ineligible column, the original bits elsewhere."""
    s = np.array(s, dtype=np.float32, copy=True)
    s[~eligible(s, pos_list, id_base, max_ratio, alive, pos)] = -np.inf
    return s


def order(s_row, ok_row, id_base=0):
    """The eligible columns of one row as global ids in (score descending, id ascending) order."""
    cols = np.nonzero(ok_row)[0]
    key = sorted(cols.tolist(), key=lambda c: (-float(s_row[c]), c))
    return [c + id_base for c in key]


def mine(s, pos_list, n_neg, id_base=0, max_ratio=None, skip_top=0, alive=None, pos=None):
    """(neg_scores fp32 [n_q, n_neg], neg_ids int64 [n_q, n_neg])"""
    s = np.asarray(s, dtype=np.float32)
    ok = eligible(s, pos_list, id_base, max_ratio, alive, pos)
    n_q = s.shape[0]
    out_s = np.full((n_q, n_neg), -np.inf, dtype=np.float32)
    out_i = np.full((n_q, n_neg), -1, dtype=np.int64)
    for q in range(n_q):
        ids = order(s[q], ok[q], id_base)[skip_top:skip_top + n_neg]
        out_i[q, :len(ids)] = ids
        out_s[q, :len(ids)] = [s[q, i - id_base] for i in ids]
    return out_s, out_i


def gather(blob, off, ids, pad_to, id_base=0):
    """(box [*ids.shape, pad_to, width], lengths int32 [*ids.shape]): rows of page ids[...] - id_base, truncated to pad_to, zeros after."""
    blob, off, ids = np.asarray(blob), np.asarray(off), np.asarray(ids)
    n = len(off) - 1
    box = np.zeros(ids.shape + (pad_to, blob.shape[1]), dtype=blob.dtype)
    lens = np.zeros(ids.shape, dtype=np.int32)
    for at in np.ndindex(*ids.shape):
        c = int(ids[at]) - id_base
        if ids[at] >= 0 and 0 <= c < n:
            m = min(int(off[c + 1] - off[c]), pad_to)
            box[at][:m] = blob[off[c]:off[c] + m]
            lens[at] = m
    return box, lens
