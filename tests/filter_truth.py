"""Filtered search restated in numpy: the contract of `PageFilter`, msim_filter_* (include/maxsim.h) and
`ShardedRetriever.search(filter=)`, written without any of their code.

A filter SPEC is one of
    ("shared", mask [n])                      one bool / uint8 row for every query
    ("per_query", mask [n_q, n])              one row per query
    ("labels", page_labels [n], query_labels [n_q])
"""
import numpy as np


def allowed(spec, n_q, n):
    """bool [n_q, n]: page c may be returned for query q"""
    kind = spec[0]
    if kind == "shared":
        m = np.asarray(spec[1]).astype(bool).reshape(1, n)
        return np.broadcast_to(m, (n_q, n)).copy()
    if kind == "per_query":
        m = np.asarray(spec[1]).astype(bool)
        assert m.shape == (n_q, n)
        return m.copy()
    if kind == "labels":
        pages, queries = np.asarray(spec[1]), np.asarray(spec[2])
        assert pages.shape == (n,) and queries.shape == (n_q,)
        return pages[None, :] == queries[:, None]
    raise ValueError(kind)


def with_alive(ok, alive):
    return ok if alive is None else ok & (np.asarray(alive) != 0)[None, :ok.shape[1]]


def pack(mask):
    """uint32 [rows, ceil(n / 32)]: bit c % 32 of word c / 32 is page c; bits at positions >= n are 0"""
    mask = np.asarray(mask).astype(bool)
    rows, n = mask.shape
    words = np.zeros((rows, (n + 31) // 32), dtype=np.uint32)
    for c in range(n):
        words[:, c // 32] |= mask[:, c].astype(np.uint32) << np.uint32(c % 32)
    return words


def masked(scores, ok):
    """a copy of fp32 `scores` with -inf wherever `ok` is False; every kept entry keeps its bits"""
    out = np.array(scores, dtype=np.float32, copy=True)
    out[~ok] = -np.inf
    return out


def search_truth(scores, ok, k, id_base=0):
    """The result contract: per query the allowed pages whose score is not -inf, by (score descending, id ascending), cut at k,
    padded with (-inf, -1).  -> (fp32 [n_q, k], int64 [n_q, k])"""
    scores = np.asarray(scores, dtype=np.float32)
    n_q, n = scores.shape
    out_s = np.full((n_q, k), -np.inf, dtype=np.float32)
    out_i = np.full((n_q, k), -1, dtype=np.int64)
    for q in range(n_q):
        cols = [c for c in range(n) if ok[q, c] and not np.isneginf(scores[q, c])]
        cols.sort(key=lambda c: (-float(scores[q, c]), c))
        cols = cols[:k]
        out_s[q, :len(cols)] = scores[q, cols]
        out_i[q, :len(cols)] = np.asarray(cols, dtype=np.int64) + id_base
    return out_s, out_i


def list_truth(ok, m_cap, id_base=0):
    """-> (cand int64 [n_q, m_cap] ascending ids padded with -1, counts int32 [n_q] the TRUE counts, status 0 / 1)"""
    n_q, n = ok.shape
    cand = np.full((n_q, m_cap), -1, dtype=np.int64)
    counts = np.zeros((n_q,), dtype=np.int32)
    for q in range(n_q):
        ids = np.flatnonzero(ok[q]).astype(np.int64) + id_base
        counts[q] = ids.size
        keep = ids[:m_cap]
        cand[q, :keep.size] = keep
    return cand, counts, int((counts > m_cap).any())


def ids_truth(ids, ok, id_base=0):
    """a copy of int64 `ids` [n_q, m] with -1 over every id in [id_base, id_base + n) that `ok` does not allow for its row"""
    ids = np.array(ids, dtype=np.int64, copy=True)
    n_q, n = ok.shape
    for q in range(n_q):
        for j in range(ids.shape[1]):
            c = ids[q, j] - id_base
            if ids[q, j] >= 0 and 0 <= c < n and not ok[q, c]:
                ids[q, j] = -1
    return ids


def spec_of(flt, n_q):
    """the SPEC of a colpali_amd.PageFilter (reads its tensors back)"""
    if flt.words is not None:
        words = flt.words.cpu().numpy().view(np.uint32)
        n = len(flt)
        cols = np.arange(n)
        m = ((words[:, cols // 32] >> (cols % 32).astype(np.uint32)) & 1).astype(bool)
        return ("shared", m[0]) if flt.shared else ("per_query", m)
    return ("labels", flt.page_labels.cpu().numpy(), flt.query_labels.cpu().numpy())


def two_stage_truth(coarse, exact, ok, n_candidates, k, id_base=0):
    """`search(prefilter=, filter=)`: the stage-1 scores masked, the top `n_candidates` (a -inf candidate is no candidate), the exact
    scores of those pages, the top k."""
    _, cand = search_truth(coarse, ok, n_candidates, id_base)
    listed = np.zeros_like(ok)
    for q in range(ok.shape[0]):
        listed[q, cand[q][cand[q] >= 0] - id_base] = True
    return search_truth(exact, listed, k, id_base)
