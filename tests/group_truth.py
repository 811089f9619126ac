"""Document-level search restated in numpy: the contract of `PageGroups`, msim_group_reduce / msim_group_select (include/maxsim.h)
and `ShardedRetriever.search(group_by=)`, written without any of their code.

The order everywhere: the higher score first; equal floats tie (-0.0 == +0.0); inside a document the lower page id wins a tie,
between documents the lower document id.  A score of -inf is "not there".
"""
import numpy as np


def _better(s, i, best_s, best_i):
    """(s, i) ranks before (best_s, best_i): plain float comparison, so -0.0 and +0.0 tie"""
    return best_i < 0 or s > best_s or (s == best_s and i < best_i)


def reduce_truth(scores, page_groups, id_base=0):
    """-> (group_ids int64 [G] ascending unique, group_scores fp32 [n_q, G] the winner's own bits, group_pages int64 [n_q, G] its
    GLOBAL id); a document whose pages all score -inf is (-inf, -1)"""
    scores = np.asarray(scores, dtype=np.float32)
    labels = np.asarray(page_groups, dtype=np.int64)
    n_q, n = scores.shape
    assert labels.shape == (n,)
    group_ids = np.unique(labels)
    out_s = np.full((n_q, group_ids.size), -np.inf, dtype=np.float32)
    out_p = np.full((n_q, group_ids.size), -1, dtype=np.int64)
    for q in range(n_q):
        for g, gid in enumerate(group_ids):
            for c in np.flatnonzero(labels == gid):
                s = scores[q, c]
                if not np.isneginf(s) and _better(s, c, out_s[q, g], out_p[q, g]):
                    out_s[q, g], out_p[q, g] = s, c
    out_p[out_p >= 0] += id_base
    return group_ids, out_s, out_p


def _emit(best, k):
    """{document: (score, page)} -> the k best by (score desc, document asc), padded; scores as the top-k returns them (+0.0)"""
    docs = sorted(best, key=lambda d: (-float(best[d][0]), d))[:k]
    out_s = np.full((k,), -np.inf, dtype=np.float32)
    out_g = np.full((k,), -1, dtype=np.int64)
    out_p = np.full((k,), -1, dtype=np.int64)
    for j, d in enumerate(docs):
        out_s[j], out_g[j], out_p[j] = best[d][0] + np.float32(0.0), d, best[d][1]
    return out_s, out_g, out_p


def select_truth(scores, gids, pages, k):
    """rows of (score, document id, page id) -> (scores fp32 [n_q, k], group_ids int64 [n_q, k], page_ids int64 [n_q, k]); an entry
    with a document id < 0 or a score of -inf is no entry"""
    scores = np.asarray(scores, dtype=np.float32)
    gids, pages = np.asarray(gids, dtype=np.int64), np.asarray(pages, dtype=np.int64)
    rows = []
    for q in range(scores.shape[0]):
        best = {}
        for s, g, p in zip(scores[q], gids[q], pages[q]):
            g, p = int(g), int(p)
            if g < 0 or np.isneginf(s):
                continue
            if g not in best or _better(s, p, *best[g]):
                best[g] = (s, p)
        rows.append(_emit(best, k))
    if not rows:
        return np.zeros((0, k), np.float32), np.zeros((0, k), np.int64), np.zeros((0, k), np.int64)
    return tuple(np.stack(x) for x in zip(*rows))


def search_truth(scores, page_groups, k, id_base=0, allowed=None):
    """The result contract of `search(group_by=)`: scores fp32 [n_q, n] of the pages, `allowed` bool [n_q, n] (None: every page) ->
    per query the k best documents, each scored by its best allowed page that is not -inf and returned with that page's GLOBAL id"""
    scores = np.asarray(scores, dtype=np.float32)
    labels = np.asarray(page_groups, dtype=np.int64)
    n_q, n = scores.shape
    rows = []
    for q in range(n_q):
        best = {}
        for c in range(n):
            s = scores[q, c]
            if np.isneginf(s) or (allowed is not None and not allowed[q, c]):
                continue
            d = int(labels[c])
            if d not in best or _better(s, c + id_base, *best[d]):
                best[d] = (s, c + id_base)
        rows.append(_emit(best, k))
    if not rows:
        return np.zeros((0, k), np.float32), np.zeros((0, k), np.int64), np.zeros((0, k), np.int64)
    return tuple(np.stack(x) for x in zip(*rows))
