"""Page filters: which pages of a shard each query may return (one tenant's pages, one collection, the pages a metadata query matched).

A `PageFilter` is handed to `ShardedRetriever.search(filter=)` / `LiveCorpus.search(filter=)`, which answer with the top-k WITHIN the
allowed pages -- not the top-k of the shard filtered afterwards.  The kernels are include/maxsim.h: msim_filter_* (colpali_amd/csrc/
filter.hip):

    filter_pack   bool / uint8 mask -> uint32 words (bit c % 32 of word c / 32 is page c)
    filter_mask   -inf, in place, into every column of a score matrix that is not allowed (the MASK route: scan, mask, top-k)
    filter_list   the allowed pages of every query as an ascending id list (the LIST route: list, rerank, top-k)
    filter_ids    -1 over the disallowed ids of a caller's candidate list (`search(candidates=, filter=)`)

Both forms of a filter live on the shard's device and are never read on the host, except by `prepare()`.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch

from . import _lib

# `search(filter_route="auto")` lists the allowed pages (and reranks the list) instead of scanning and masking only when no query is
# allowed more than this fraction of the shard.  1/5 is a bound, not a measurement: a list entry costs 20 B (8 B id in, 4 B score,
# 8 B id out) against the 4 B per column of the score matrix, so below n / 5 the list route never needs more memory than the mask
# route.  tools/bench_filter.py measured the list route faster than the mask route up to selectivity 0.5 at 4 and at 1000 x 32 queries
# on the headline shard (profiles/filter_summary.md), so the cap is what ships.
LIST_ROUTE_MAX_FRACTION = 1.0 / 5.0


def _gpu(t: torch.Tensor, what: str) -> torch.device:
    if t.device.type != "cuda":
        raise ValueError(f"{what}: the tensors must live on the GPU (a gfx950 kernel; there is no CPU fallback)")
    return t.device


def filter_pack(mask: torch.Tensor) -> torch.Tensor:
    """mask (bool / uint8 [rows, n] on the GPU, unit inner stride, any row stride >= n) -> int32 [rows, ceil(n / 32)] holding the
    uint32 words of msim_filter_pack; bits at positions >= n are 0.  Asynchronous on torch's current stream."""
    dev = _gpu(mask, "filter_pack")
    rows, n = mask.shape
    m8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    ld = m8.stride(0) if rows > 1 else max(n, 1)
    words = torch.zeros((rows, (n + 31) // 32), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_filter_pack(_lib.ptr(m8), ld, rows, n, _lib.ptr(words), max(words.shape[1], 1),
                                         _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_filter_pack")
    return words


class PageFilter:
    """For one shard: which pages each query may return.  `len(filter)` and `filter.id_base` must equal the shard's.

    Two forms (build with `from_mask` / `from_labels`), both resident on the shard's device:
      * bits: `words` int32 [rows, ceil(n / 32)] holding uint32 words, bit c % 32 of word c / 32 is page c; rows == 1: one filter
        shared by every query (`shared`), otherwise one row per query;
      * labels: `page_labels` int32 [n], `query_labels` int32 [n_q]; page c is allowed for query q iff the labels are equal.  No
        [n_q, n] object is ever made.
    `prepare()` computes `max_allowed` -- the largest number of allowed pages of any query -- with one device-to-host
    synchronisation and caches it; `search` calls it on first use, so a caller who wants a hipGraph-capturable `search` calls it
    beforehand.  A filter is IMMUTABLE after `prepare()`: its tensors must not be written again (the list route sizes its candidate
    list by `max_allowed`; a filter that grew afterwards would lose pages)."""

    def __init__(self, n: int, id_base: int, words: Optional[torch.Tensor] = None, page_labels: Optional[torch.Tensor] = None,
                 query_labels: Optional[torch.Tensor] = None, shared: bool = False):
        if (words is None) == (page_labels is None) or (page_labels is None) != (query_labels is None):
            raise ValueError("a PageFilter holds either words or (page_labels, query_labels): use from_mask / from_labels")
        self.n, self.id_base = int(n), int(id_base)
        self.words, self.page_labels, self.query_labels = words, page_labels, query_labels
        self.shared = bool(shared) and words is not None        # one row of bits for every query
        self.max_allowed: Optional[int] = None

    # ------------------------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_mask(cls, mask: torch.Tensor, id_base: int = 0, *, pack_fn: Callable = filter_pack) -> "PageFilter":
        """mask: bool or uint8 (non-zero = allowed), [n] -- one filter shared by every query -- or [n_q, n], one row per query; any
        row stride, unit inner stride.  Packed once into words (msim_filter_pack; `pack_fn` is the hook host-logic tests replace)."""
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("mask must be a bool or uint8 tensor")
        if mask.dim() not in (1, 2):
            raise ValueError(f"mask must have shape [n] (shared) or [n_q, n] (got {tuple(mask.shape)})")
        m2 = mask[None, :] if mask.dim() == 1 else mask
        rows, n = m2.shape
        if rows < 1:
            raise ValueError("a per-query mask needs at least one row")
        if n > 1 and m2.stride(1) != 1:
            raise ValueError("mask must have unit inner stride")
        if n >= 2**31:
            raise NotImplementedError("more than 2^31 - 1 pages in one shard")
        if rows > 1 and m2.stride(0) < n:
            m2 = m2.contiguous()                         # an expanded row
        words = pack_fn(m2)
        if words.shape != (rows, (n + 31) // 32) or words.dtype != torch.int32:
            raise ValueError("pack_fn must return int32 [rows, ceil(n / 32)]")
        return cls(n, id_base, words=words, shared=mask.dim() == 1)

    @classmethod
    def from_labels(cls, page_labels: torch.Tensor, query_labels: torch.Tensor, id_base: int = 0) -> "PageFilter":
        """page_labels int32 [n], query_labels int32 [n_q], on one device: page c is allowed for query q iff
        page_labels[c] == query_labels[q] (the tenant / collection case)."""
        for t, what in ((page_labels, "page_labels"), (query_labels, "query_labels")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
                raise ValueError(f"{what} must be a 1-D int32 tensor")
        if page_labels.device != query_labels.device:
            raise ValueError("page_labels and query_labels live on different devices")
        if page_labels.shape[0] >= 2**31:
            raise NotImplementedError("more than 2^31 - 1 pages in one shard")
        return cls(int(page_labels.shape[0]), id_base, page_labels=page_labels.contiguous(), query_labels=query_labels.contiguous())

    # ------------------------------------------------------------------------------------------------------------------- state
    def __len__(self) -> int:
        return self.n

    @property
    def device(self) -> torch.device:
        return (self.words if self.words is not None else self.page_labels).device

    @property
    def rows(self) -> Optional[int]:
        """Queries the filter was built for (None: shared, any number)."""
        if self.shared:
            return None
        return int(self.words.shape[0] if self.words is not None else self.query_labels.shape[0])

    def prepare(self) -> "PageFilter":
        """Compute and cache `max_allowed` (one device-to-host synchronisation); afterwards the filter must not change."""
        if self.max_allowed is not None:
            return self
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("PageFilter.prepare() synchronises with the host: call it once before the capture")
        if self.n == 0 or (self.rows == 0):
            self.max_allowed = 0
        elif self.words is not None:
            v = self.words.to(torch.int64) & 0xFFFFFFFF                  # popcount of every word
            v = v - ((v >> 1) & 0x55555555)
            v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
            v = (v + (v >> 4)) & 0x0F0F0F0F
            v = ((v * 0x01010101) & 0xFFFFFFFF) >> 24
            self.max_allowed = int(v.sum(dim=1).max().item())
        else:
            pages = torch.sort(self.page_labels).values
            q = self.query_labels
            per = torch.searchsorted(pages, q, right=True) - torch.searchsorted(pages, q, right=False)
            self.max_allowed = int(per.max().item())
        return self

    def _kernel_args(self) -> Tuple[int, int, int, int]:
        """(bits, ld_words, page_labels, query_labels) as msim_filter_* take them"""
        if self.words is not None:
            return _lib.ptr(self.words), 0 if self.shared else max(int(self.words.shape[1]), 1), 0, 0
        return 0, 0, _lib.ptr(self.page_labels), _lib.ptr(self.query_labels)


def _check_filter(flt: PageFilter, n_q: int, n: int, dev: torch.device, what: str) -> None:
    if not isinstance(flt, PageFilter):
        raise ValueError(f"{what}: filter must be a PageFilter")
    if len(flt) != n:
        raise ValueError(f"{what}: the filter covers {len(flt)} pages, {n} were expected")
    if flt.device != dev:
        raise ValueError(f"{what}: the filter lives on {flt.device}, the other tensors on {dev}")
    if flt.rows is not None and flt.rows != n_q:
        raise ValueError(f"{what}: a per-query filter of {flt.rows} rows was given for {n_q} queries")


def _check_alive(alive: Optional[torch.Tensor], n: int, dev: torch.device) -> None:
    if alive is not None and (alive.dtype != torch.uint8 or alive.dim() != 1 or alive.shape[0] < n or alive.device != dev
                              or not alive.is_contiguous()):
        raise ValueError(f"alive must be a contiguous uint8 [>= {n}] tensor on {dev}")


def filter_mask(scores: torch.Tensor, flt: PageFilter, alive: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-inf, in place, into scores[q, c] (fp32 [n_q, n] on the GPU, any row stride) wherever page c is not allowed for query q, or
    `alive[c] == 0` (uint8 [>= n]); nothing else is touched (msim_filter_mask).  Asynchronous on torch's current stream,
    hipGraph-capturable."""
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("filter_mask: scores must be a 2-D fp32 tensor")
    dev = _gpu(scores, "filter_mask")
    n_q, n = scores.shape
    if n > 1 and scores.stride(1) != 1:
        raise ValueError("filter_mask: scores must have unit inner stride")
    _check_filter(flt, n_q, n, dev, "filter_mask")
    _check_alive(alive, n, dev)
    ld = scores.stride(0) if n_q > 1 else max(n, 1)
    bits, ld_words, pl, ql = flt._kernel_args()
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_filter_mask(_lib.ptr(scores), ld, n_q, n, bits, ld_words, pl, ql, _lib.ptr(alive),
                                         _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_filter_mask")
    return scores


def filter_list(flt: PageFilter, n_q: int, m_cap: int, alive: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The allowed (and alive) pages of every query as ascending GLOBAL ids (msim_filter_list):
    (cand int64 [n_q, m_cap], padded with -1; counts int32 [n_q], the true counts; status int32 [1], non-zero when a row held more
    than `m_cap` pages and was cut to its first `m_cap`).  Asynchronous on torch's current stream, hipGraph-capturable."""
    dev = _gpu(flt.words if flt.words is not None else flt.page_labels, "filter_list")
    n_q, m_cap, n = int(n_q), int(m_cap), len(flt)
    if n_q < 0 or m_cap < 0:
        raise ValueError("filter_list: n_q and m_cap must not be negative")
    if n_q * m_cap >= 2**31:
        raise NotImplementedError("filter_list: more than 2^31 - 1 list entries")
    _check_filter(flt, n_q, n, dev, "filter_list")
    _check_alive(alive, n, dev)
    cand = torch.empty((n_q, m_cap), dtype=torch.int64, device=dev)
    counts = torch.empty((n_q,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = torch.empty((max(int(L.msim_filter_list_workspace_bytes(n_q, n)), 16),), dtype=torch.uint8, device=dev)
    if n_q == 0 or n == 0:                               # the entry returns before it looks at a pointer
        cand.fill_(-1)
        counts.zero_()
        ws.zero_()
        return cand, counts, ws[:4].view(torch.int32)
    bits, ld_words, pl, ql = flt._kernel_args()
    with torch.cuda.device(dev):
        rc = L.msim_filter_list(bits, ld_words, pl, ql, _lib.ptr(alive), n_q, n, int(flt.id_base), _lib.ptr(cand), max(m_cap, 1), m_cap,
                                _lib.ptr(counts), _lib.ptr(ws), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_filter_list")
    return cand, counts, ws[:4].view(torch.int32)


def filter_ids(ids: torch.Tensor, flt: PageFilter, alive: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-1, in place, over every entry of `ids` (int64 [n_q, m] GLOBAL ids on the GPU) that lies in the filter's shard and is not
    allowed for its row, or not alive; -1 and ids of other shards stay (msim_filter_ids).  Asynchronous, hipGraph-capturable."""
    if ids.dim() != 2 or ids.dtype != torch.int64:
        raise ValueError("filter_ids: ids must be a 2-D int64 tensor")
    dev = _gpu(ids, "filter_ids")
    n_q, m = ids.shape
    if m > 1 and ids.stride(1) != 1:
        raise ValueError("filter_ids: ids must have unit inner stride")
    if n_q > 1 and ids.stride(0) < m:
        raise ValueError("filter_ids: the rows of ids overlap (an expanded list): pass a copy")
    n = len(flt)
    _check_filter(flt, n_q, n, dev, "filter_ids")
    _check_alive(alive, n, dev)
    ld = ids.stride(0) if n_q > 1 else max(m, 1)
    bits, ld_words, pl, ql = flt._kernel_args()
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_filter_ids(_lib.ptr(ids), ld, n_q, m, n, int(flt.id_base), bits, ld_words, pl, ql, _lib.ptr(alive),
                                        _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_filter_ids")
    return ids
