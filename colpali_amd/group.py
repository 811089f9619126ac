"""Document-level search: pages grouped into documents (PDFs, slide decks, reports), and the top-k DOCUMENTS of a query.

A `PageGroups` is handed to `ShardedRetriever.search(group_by=)` / `LiveCorpus.search(group_by=)`, which answer with the k best
documents -- each scored by its best page, and returned with that page -- instead of the k best pages.  The kernels are
include/maxsim.h: msim_group_* (colpali_amd/csrc/group.hip):

    group_reduce   score matrix [n_q, n] -> (best score, best page) of every document, [n_q, G]: the scan route (reduce, then `topk`)
    group_select   candidate rows of (score, document id, page id) -> the k best documents of every row: behind a rerank, and the
                   merge of a sharded search

Everything lives on the shard's device and is never read on the host, except by `prepare()`.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

SELECT_MAX_M = 4096        # include/maxsim.h: MSIM_GROUP_SELECT_MAX_M, the widest candidate row of msim_group_select
SELECT_MAX_K = 1024        # MSIM_GROUP_SELECT_MAX_K


def _gpu(t: torch.Tensor, what: str) -> torch.device:
    if t.device.type != "cuda":
        raise ValueError(f"{what}: the tensors must live on the GPU (a gfx950 kernel; there is no CPU fallback)")
    return t.device


class PageGroups:
    """For one shard: the document every page belongs to.  `len(groups)` and `groups.id_base` must equal the shard's.

    Build with `from_labels`.  Document ids are GLOBAL: the same id may appear on several shards (a document may straddle a shard
    boundary), and the pages of a document need not be contiguous.  `prepare()` derives, with torch ops on the shard's device,
      * `group_ids`   int64 [G], the document ids present on this shard, ascending and unique;
      * `page_group`  int32 [n], page c belongs to document `group_ids[page_group[c]]`;
      * `offsets` int32 [G + 1] and `pages` int32 [n], the CSR msim_group_reduce reads: the LOCAL page indices of document g are
        `pages[offsets[g] : offsets[g + 1]]`, ascending;
      * `n_groups` (G) and `max_group`, the most pages any document has here.
    It costs one device-to-host synchronisation; `search` calls it on first use, so a caller who wants a hipGraph-capturable
    `search` calls it beforehand.  The object is IMMUTABLE afterwards: its tensors must not be written again."""

    def __init__(self, page_groups: torch.Tensor, id_base: int = 0):
        if not isinstance(page_groups, torch.Tensor) or page_groups.dtype != torch.int64 or page_groups.dim() != 1:
            raise ValueError("page_groups must be a 1-D int64 tensor (the document id of every page)")
        if page_groups.shape[0] >= 2**31:
            raise NotImplementedError("more than 2^31 - 1 pages in one shard")
        self.labels = page_groups.contiguous()
        self.n, self.id_base = int(page_groups.shape[0]), int(id_base)
        self.group_ids: Optional[torch.Tensor] = None
        self.page_group: Optional[torch.Tensor] = None
        self.offsets: Optional[torch.Tensor] = None
        self.pages: Optional[torch.Tensor] = None
        self.n_groups: Optional[int] = None
        self.max_group: Optional[int] = None

    @classmethod
    def from_labels(cls, page_groups: torch.Tensor, id_base: int = 0) -> "PageGroups":
        """page_groups: int64 [n] on the shard's device; entry c is the GLOBAL document id (>= 0) of page id_base + c."""
        return cls(page_groups, id_base)

    def __len__(self) -> int:
        return self.n

    @property
    def device(self) -> torch.device:
        return self.labels.device

    def prepare(self) -> "PageGroups":
        """Build the dense document index and the CSR (one device-to-host synchronisation); afterwards the object must not change."""
        if self.n_groups is not None:
            return self
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("PageGroups.prepare() synchronises with the host: call it once before the capture")
        dev, n = self.device, self.n
        if n and int(self.labels.min().item()) < 0:
            raise ValueError("page_groups holds a negative document id: ids are >= 0 (-1 means 'no document' in every result)")
        group_ids, inverse = torch.unique(self.labels, sorted=True, return_inverse=True)
        g = int(group_ids.shape[0])
        counts = torch.bincount(inverse, minlength=g) if n else torch.zeros((0,), dtype=torch.int64, device=dev)
        offsets = torch.zeros((g + 1,), dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
        self.group_ids = group_ids.contiguous()
        self.page_group = inverse.to(torch.int32).contiguous()
        self.pages = torch.argsort(inverse, stable=True).to(torch.int32).contiguous()      # stable: ascending inside a document
        self.offsets = offsets
        self.max_group = int(counts.max().item()) if g else 0
        self.n_groups = g
        return self

    def doc_ids(self, ids: torch.Tensor) -> torch.Tensor:
        """GLOBAL page ids (int64, any shape, on this device) -> the document id of each; -1 for -1 and for ids outside this shard.
        Torch gathers on the device: no kernel, no synchronisation once prepared."""
        self.prepare()
        if self.n == 0:
            return torch.full_like(ids, -1)
        c = ids - self.id_base
        inside = (ids >= 0) & (c >= 0) & (c < self.n)
        dense = self.page_group[c.clamp(0, self.n - 1)].long()
        return torch.where(inside, self.group_ids[dense], torch.full_like(ids, -1))


def group_reduce(scores: torch.Tensor, groups: PageGroups) -> Tuple[torch.Tensor, torch.Tensor]:
    """The best page of every document for every query (msim_group_reduce): scores fp32 [n_q, n] on the GPU (unit inner stride, any
    row stride) -> (group_scores fp32 [n_q, G], group_pages int64 [n_q, G]); column g is document `groups.group_ids[g]`.  The
    higher score wins, equal floats tie (-0.0 and +0.0 too) and the lower page wins a tie; the score keeps the winner's bits, the
    page is its GLOBAL id; a document whose pages all score -inf is (-inf, -1).  Asynchronous on torch's current stream; with
    prepared groups hipGraph-capturable."""
    if not isinstance(groups, PageGroups):
        raise ValueError("group_reduce: groups must be a PageGroups")
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("group_reduce: scores must be a 2-D fp32 tensor")
    dev = _gpu(scores, "group_reduce")
    n_q, n = scores.shape
    if n > 1 and scores.stride(1) != 1:
        raise ValueError("group_reduce: scores must have unit inner stride")
    if len(groups) != n:
        raise ValueError(f"group_reduce: the groups cover {len(groups)} pages, the scores have {n} columns")
    if groups.device != dev:
        raise ValueError(f"group_reduce: the groups live on {groups.device}, the scores on {dev}")
    groups.prepare()
    g = groups.n_groups
    out_s = torch.empty((n_q, g), dtype=torch.float32, device=dev)
    out_p = torch.empty((n_q, g), dtype=torch.int64, device=dev)
    ld = scores.stride(0) if n_q > 1 else max(n, 1)
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_group_reduce(_lib.ptr(scores), ld, n_q, n, _lib.ptr(groups.offsets), _lib.ptr(groups.pages), g,
                                          int(groups.id_base), _lib.ptr(out_s), _lib.ptr(out_p), max(g, 1),
                                          _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_group_reduce")
    return out_s, out_p


def group_select(scores: torch.Tensor, gids: torch.Tensor, pages: torch.Tensor, k: int, out=None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The k best documents of every candidate row (msim_group_select).  scores fp32, gids int64 (document ids), pages int64 (page
    ids), each [n_q, m] on the GPU; an entry with gid < 0 or a score of -inf is no entry.  Per row the best entry of every document
    by (score desc, page id asc) survives, the survivors are ordered by (score desc, document id asc) and cut at k:
    (scores fp32 [n_q, k], group_ids int64 [n_q, k], page_ids int64 [n_q, k]), padded with (-inf, -1, -1).  m <= 4096, k <= 1024
    (NotImplementedError).  out: optional contiguous (fp32, int64, int64) [n_q, k] tensors to write into.  Asynchronous on torch's
    current stream, hipGraph-capturable."""
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("group_select: scores must be a 2-D fp32 tensor")
    dev = _gpu(scores, "group_select")
    for t, what in ((gids, "gids"), (pages, "pages")):
        if not isinstance(t, torch.Tensor) or t.shape != scores.shape or t.dtype != torch.int64 or t.device != dev:
            raise ValueError(f"group_select: {what} must be int64 with the shape and device of scores")
    n_q, m = scores.shape
    k = int(k)
    if k < 1:
        raise ValueError("group_select: k must be positive")
    if not (scores.is_contiguous() and gids.is_contiguous() and pages.is_contiguous()):      # one row stride for the three
        scores, gids, pages = scores.contiguous(), gids.contiguous(), pages.contiguous()
    if out is not None:
        out_s, out_g, out_p = out
        for t, dt in ((out_s, torch.float32), (out_g, torch.int64), (out_p, torch.int64)):
            if t.shape != (n_q, k) or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError("group_select: out must be contiguous (fp32, int64, int64) [n_q, k] tensors on the scores' device")
    else:
        out_s = torch.empty((n_q, k), dtype=torch.float32, device=dev)
        out_g = torch.empty((n_q, k), dtype=torch.int64, device=dev)
        out_p = torch.empty((n_q, k), dtype=torch.int64, device=dev)
    if m == 0:                                           # the entry returns before it looks at a pointer
        out_s.fill_(float("-inf"))
        out_g.fill_(-1)
        out_p.fill_(-1)
        return out_s, out_g, out_p
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_group_select(_lib.ptr(scores), _lib.ptr(gids), _lib.ptr(pages), n_q, m, max(m, 1), k, _lib.ptr(out_s),
                                          _lib.ptr(out_g), _lib.ptr(out_p), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_group_select")
    return out_s, out_g, out_p
