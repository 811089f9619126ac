"""A live resident shard: pages are added, deleted and compacted in place, and every search sees the change at once.

`LiveCorpus` owns one row blob with spare capacity, the page offsets, a tombstone mask (`alive`) and, on request, an int8 index
(`int8_index()`) and an FP4 index (`fp4_index()`: width 128 and width 320) kept in step.  No scoring kernel changes: every scorer
reads page c through `offsets[c] .. offsets[c + 1]`, so

  * `add` appends rows at the tail of the blob and slots at the tail of the offsets (no reallocation, ever);
  * `delete` clears `alive`; the scores of deleted slots are overwritten with -inf behind the full scan and the int8 / FP4 stage 1
    (msim_live_mask_scores), and deleted candidate ids become -1 before the rerank;
  * `compact` moves the rows of live pages down over the deleted ones (msim_live_compact, colpali_amd/csrc/live_corpus.hip) and turns
    every deleted slot into an empty page.

A page's id is its slot: `id_base + slot`, assigned in order of arrival, never reused, never renumbered -- the rule every kernel
and `shard_topk` already follow.  After any history, `search` returns the scores (bit for bit) of a `ShardedRetriever` over
`pack_passages(surviving pages in slot order, batch_size=None)`, with that corpus' positions mapped back to slots.

`_LiveShard` below is the half that does not depend on what a row is: the slot table and its rules, and `add` / `delete` /
`compact` / `search` / `mine` / `align` up to the few methods that touch the rows.  `LiveCorpus` supplies those for a bf16 / f16 /
f32 blob, `LiveResidualCorpus` (colpali_amd/live_residual.py) for a residual-compressed shard.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .corpus import PackedCorpus, _as_packed, _staging, _widen, host_list_image
from .int8_index import DIM as I8_DIM
from .int8_index import Int8Index, int8_scores
from ._fp4_family import FAMILIES as F4_FAMILIES
from .fp4_index import Fp4Index, fp4_rerank_scores, fp4_scores
from .fp4_wide_index import Fp4WideIndex, fp4_wide_rerank_scores, fp4_wide_scores
from .align import Alignment, align
from .filter import PageFilter, filter_ids, filter_list, filter_mask
from .group import PageGroups, group_reduce, group_select
from .mine import mine_bounds, mine_mask
from .retrieval import ShardedRetriever, _no_page, rerank_scores, topk
from .scoring import maxsim_scores

DEFAULT_BOUNCE_BYTES = 256 << 20     # rows a compaction moves per pair of launches (tools/bench_live.py --bounce-mb)


def mask_scores(scores: torch.Tensor, alive: torch.Tensor) -> torch.Tensor:
    """-inf into column c of every row of `scores` (fp32 [n_q, n], on the GPU) where `alive[c] == 0` (uint8 [n]); in place.
    Asynchronous on torch's current stream, hipGraph-capturable."""
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.device.type != "cuda":
        raise ValueError("scores must be a 2-D fp32 tensor on the GPU (the mask is a gfx950 kernel; there is no CPU fallback)")
    n_q, n = scores.shape
    if alive.dtype != torch.uint8 or alive.dim() != 1 or alive.shape[0] < n or alive.device != scores.device or not alive.is_contiguous():
        raise ValueError(f"alive must be a contiguous uint8 [>= {n}] tensor on {scores.device}")
    if n > 1 and scores.stride(1) != 1:
        raise ValueError("scores must have unit inner stride")
    ld = scores.stride(0) if n_q > 1 else max(n, 1)
    with torch.cuda.device(scores.device):
        rc = _lib.lib().msim_live_mask_scores(_lib.ptr(scores), ld, n_q, n, _lib.ptr(alive), _lib.current_stream_handle(scores.device))
    _lib.check(rc, "msim_live_mask_scores")
    return scores


class _LiveShard:
    """The half `LiveCorpus` and `LiveResidualCorpus` share: the slot table (offsets, `alive`, the host mirrors), its rules -- ids
    are never reused, a device-side delete is read back before the host decides anything, a refusal leaves the shard as it was,
    `check()` compares the device's row count with the host's -- and every search route over the tombstones.  A subclass owns the
    storage and supplies `view`, `_write_rows`, `_move_rows`, `_widths` and the names below."""

    _entry = ""                # the compaction entry behind `_move_rows` (its workspace size, the messages of `check()`)

    @staticmethod
    def _capacity(capacity_rows, capacity_docs) -> Tuple[int, int]:
        capacity_rows, capacity_docs = int(capacity_rows), int(capacity_docs)
        if capacity_rows < 1 or capacity_docs < 1:
            raise ValueError("capacity_rows and capacity_docs must be positive")
        if capacity_rows >= 2**31:
            raise NotImplementedError("more than 2^31 patch rows in one shard")
        return capacity_rows, capacity_docs

    def _init_slots(self, capacity_rows: int, capacity_docs: int, device, id_base: int, *, score_fn, rerank_fn, stage1_fns, select, mask_fn,
                    align_fn, mine_bounds_fn, mine_mask_fn, filter_mask_fn, filter_list_fn, filter_ids_fn, group_reduce_fn,
                    group_select_fn, fp4_rerank_fn=fp4_rerank_scores, fp4_wide_rerank_fn=fp4_wide_rerank_scores) -> None:
        """the slot table and the hooks; the subclass has allocated its rows"""
        self.id_base = int(id_base)
        self.capacity_rows, self.capacity_docs = capacity_rows, capacity_docs
        self.offsets = torch.zeros((capacity_docs + 1,), dtype=torch.int32, device=device)
        self.alive = torch.zeros((capacity_docs + 1,), dtype=torch.uint8, device=device)   # [capacity_docs]: where ids outside the shard land
        self._lengths = np.zeros((capacity_docs,), dtype=np.int64)   # host: rows each slot owns now (0 once compacted away)
        self._alive_h = np.zeros((capacity_docs,), dtype=bool)       # host mirror of `alive` (stale while _dirty)
        self._dirty = False                                          # a device-side delete has not been read back yet
        self.n_slots = 0
        self._rows_used = 0
        self._score_fn, self._rerank_fn = score_fn, rerank_fn
        self._fp4_rerank_fn = fp4_rerank_fn   # (queries, Fp4Index, candidates) -> (scores, ids): the refine stage of search(refine=)
        self._fp4_wide_rerank_fn = fp4_wide_rerank_fn   # the same for an Fp4WideIndex (a 320-wide shard)
        self._stage1_fns = dict(stage1_fns)   # the stage-1 hooks of `ShardedRetriever` whose scores the tombstones mask, by keyword
        self._select, self._mask_fn = select, mask_fn
        self._align_fn = align_fn         # (queries, view(), ids, maps=) -> Alignment
        self._mine_bounds_fn, self._mine_mask_fn = mine_bounds_fn, mine_mask_fn
        self._filter_fns = dict(filter_mask_fn=filter_mask_fn, filter_list_fn=filter_list_fn, filter_ids_fn=filter_ids_fn,
                                group_reduce_fn=group_reduce_fn, group_select_fn=group_select_fn)
        self._compactions = 0
        self._rows_compacted = 0                                     # rows in use right after the last compaction (check())

    @staticmethod
    def _bounce_want(bounce_bytes: Optional[int], row_bytes: int) -> int:
        want = DEFAULT_BOUNCE_BYTES if bounce_bytes is None else int(bounce_bytes)
        if want < row_bytes:
            raise ValueError(f"bounce_bytes={want} holds no row of {row_bytes} bytes")
        return want

    def _alloc_compaction(self, n_plans: int) -> list:
        """everything a compaction needs exists up front (no allocation later): the bounce buffer, a workspace and a row count per
        offset plan; returns the workspaces"""
        ws_bytes = getattr(_lib.lib(), self._entry + "_workspace_bytes")(self.capacity_docs, self.bounce_bytes)
        self._bounce = torch.empty((self.bounce_bytes,), dtype=torch.uint8, device=self.device)
        ws = [torch.zeros((ws_bytes,), dtype=torch.uint8, device=self.device) for _ in range(n_plans)]
        self._rows_used_dev = torch.zeros((n_plans,), dtype=torch.int64, device=self.device)
        return ws

    @staticmethod
    def _source_lengths(src) -> np.ndarray:
        """the page lengths of a packed / compressed corpus a live shard can start from"""
        if src.clamp0 is not None:
            raise ValueError("a live shard has no block zero-padding semantics: pack with batch_size=None (clamp0 must be None)")
        lens = src.lengths.numpy().astype(np.int64)
        if (lens <= 0).any():
            raise ValueError("a live shard holds no page of 0 rows: -inf means 'not there'")
        return lens

    def _adopt(self, offsets: torch.Tensor, lens: np.ndarray) -> None:
        """slots 0 .. n - 1 are the pages whose rows the subclass has just copied in"""
        n = int(lens.size)
        self.offsets[:n + 1].copy_(offsets)
        self.alive[:n].fill_(1)
        self._lengths[:n] = lens
        self._alive_h[:n] = True
        self.n_slots, self._rows_used = n, int(lens.sum())

    # ------------------------------------------------------------------------------------------------------------------ state
    def __len__(self) -> int:
        """Slots handed out so far (live or deleted): the number of documents every view and score matrix has."""
        return self.n_slots

    @property
    def rows_used(self) -> int:
        return self._rows_used

    @property
    def n_live(self) -> int:
        self._sync_host()
        return int(self._alive_h[:self.n_slots].sum())

    def _sync_host(self) -> None:
        """Read the mask back after a device-side delete (one small D2H and a synchronisation)."""
        if not self._dirty:
            return
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a device-side delete is pending: call compact() / add() once outside the capture first")
        n = self.n_slots
        self._alive_h[:n] = self.alive[:n].cpu().numpy().astype(bool)
        self._dirty = False

    def check(self) -> None:
        """Host-side check of what the device found (synchronises): raises if a compaction met broken offsets, or if its row
        count differs from the host's."""
        if self.device.type != "cuda" or not self._compactions:
            return
        self._sync_host()
        status = [int(w[:4].view(torch.int32)[0].item()) for w in (self._ws if isinstance(self._ws, list) else [self._ws])]
        if any(status):
            raise _lib.MaxSimLibraryError(f"{self._entry} found broken offsets (status words {status}): nothing further was moved")
        got = int(self._rows_used_dev[0].item())
        if got != self._rows_compacted:
            raise _lib.MaxSimLibraryError(f"{self._entry} left {got} rows in use, the host expected {self._rows_compacted}")

    # -------------------------------------------------------------------------------------------------------------------- add
    def add(self, pages: Union[torch.Tensor, Sequence[torch.Tensor]]) -> torch.Tensor:
        """Append pages; returns their ids (int64, host).  `pages`: a list of [rows_i, width] tensors or one [n, rows, width] tensor
        (on the device: rows and offsets are written there, nothing synchronises).  Running out of rows or slots raises
        RuntimeError and leaves the shard as it was."""
        if isinstance(pages, torch.Tensor):
            if pages.dim() != 3:
                raise ValueError("a page tensor must be 3-D (n_pages, rows, width)")
            n, per, dim = (int(s) for s in pages.shape)
            if n and per == 0:
                raise ValueError("a page of 0 rows cannot be added: in a live shard -inf means 'not there'")
            lens = np.full((n,), per, dtype=np.int64)
            first = pages
        else:
            pages = list(pages)
            n = len(pages)
            for p in pages:
                if p.dim() != 2:
                    raise ValueError("each page must be 2-D (rows, width)")
                if p.shape[0] == 0:
                    raise ValueError("a page of 0 rows cannot be added: in a live shard -inf means 'not there'")
            lens = np.fromiter((p.shape[0] for p in pages), dtype=np.int64, count=n)
            first = pages[0] if n else None
            dim = int(first.shape[1]) if n else 0
            for p in pages:
                if p.dtype != first.dtype or p.shape[1] != dim:
                    raise RuntimeError("expected pages of one dtype and one embedding width")
        if n == 0:
            return torch.empty((0,), dtype=torch.int64)
        if first.dtype != self.dtype or dim not in self._widths:
            raise RuntimeError(f"this shard holds {self.dtype} pages of width {self._widths[0]}, got {first.dtype} of width {dim}")
        self._sync_host()
        total, n0, r0 = int(lens.sum()), self.n_slots, self._rows_used
        if n0 + n > self.capacity_docs:
            raise RuntimeError(f"live shard is full: {n0} of capacity_docs={self.capacity_docs} slots are taken, {n} more were asked for")
        if r0 + total > self.capacity_rows:
            raise RuntimeError(f"live shard is full: {r0} of capacity_rows={self.capacity_rows} rows are in use, {total} more were "
                               "asked for (compact() hands back the rows of deleted pages)")
        ends = self._write_rows(pages, lens, dim, n0, r0)
        if ends is None:                   # a list: the new offsets come from the host
            ends = torch.from_numpy((r0 + np.cumsum(lens)).astype(np.int32))
        self.offsets[n0 + 1:n0 + n + 1].copy_(ends)
        self.alive[n0:n0 + n].fill_(1)
        self._lengths[n0:n0 + n] = lens
        self._alive_h[n0:n0 + n] = True
        self.n_slots, self._rows_used = n0 + n, r0 + total
        self._added(n0, n0 + n)
        return torch.arange(self.id_base + n0, self.id_base + n0 + n, dtype=torch.int64)

    def _write_rows(self, pages, lens: np.ndarray, dim: int, n0: int, r0: int) -> Optional[torch.Tensor]:
        """Write the rows of the validated `pages` (they fit) from row `r0` on.  For a page tensor, return the new offsets
        (int32 [n], computed on its device); for a list, None."""
        raise NotImplementedError

    def _added(self, lo: int, hi: int) -> None:
        """slots lo .. hi - 1 have just been committed"""

    # ----------------------------------------------------------------------------------------------------------------- delete
    def delete(self, ids) -> None:
        """Clear `alive` for `ids`; every search sees it at once, the rows stay until `compact()`.  A host list (or host tensor):
        unknown, out-of-range or already-deleted ids raise KeyError and nothing is deleted.  An int64 tensor on the device is
        applied without a synchronisation and ids outside the shard are ignored."""
        if isinstance(ids, torch.Tensor) and ids.device.type != "cpu":
            if ids.dtype != torch.int64 or ids.device != self.device:
                raise ValueError(f"device ids must be an int64 tensor on {self.device}")
            idx = ids.reshape(-1) - self.id_base
            idx = torch.where((idx >= 0) & (idx < self.n_slots), idx, torch.full_like(idx, self.capacity_docs))
            self.alive.index_fill_(0, idx, 0)
            self._dirty = True
            return
        slots = [int(i) - self.id_base for i in (ids.tolist() if isinstance(ids, torch.Tensor) else ids)]
        self._sync_host()
        seen = set()
        for s in slots:
            if not (0 <= s < self.n_slots) or not self._alive_h[s] or s in seen:
                raise KeyError(s + self.id_base)
            seen.add(s)
        if not slots:
            return
        self._alive_h[slots] = False
        self.alive.index_fill_(0, torch.tensor(slots, dtype=torch.int64).to(self.device), 0)

    # ---------------------------------------------------------------------------------------------------------------- compact
    def compact(self) -> None:
        """Move the rows of live pages down over the rows of deleted ones, in place and in slot order; a deleted slot becomes an
        empty document; slots (ids) do not move.  Asynchronous on torch's current stream, no allocation in the library call.
        (After a device-side `delete` the mask is read back first: one small D2H and a synchronisation.)"""
        self._sync_host()
        n = self.n_slots
        dead = ~self._alive_h[:n] & (self._lengths[:n] > 0)
        if not dead.any():
            return
        self._move_rows(self._rows_used)
        self._lengths[:n][dead] = 0
        self._rows_used = self._rows_compacted = int(self._lengths[:n].sum())
        self._compactions += 1

    def _move_rows(self, rows_bound: int) -> None:
        """Move every array of rows, and the offsets, on the device; raise (having changed nothing) where that cannot be done."""
        raise NotImplementedError

    # ----------------------------------------------------------------------------------------------------------------- search
    def _masked(self, scores: torch.Tensor) -> torch.Tensor:
        return self._mask_fn(scores, self.alive[:self.n_slots])

    def _score(self, queries, corpus):
        return self._masked(self._score_fn(queries, corpus))

    def _stage1_hooks(self) -> dict:
        """every stage-1 hook this class masks, wrapped: (queries, index) -> its scores with -inf in the deleted slots"""
        return {kw: (lambda queries, index, fn=fn: self._masked(fn(queries, index))) for kw, fn in self._stage1_fns.items()}

    def _live_ids(self, candidates: torch.Tensor) -> torch.Tensor:
        """`candidates` with every id that is outside the shard or deleted replaced by -1 (on the device, no synchronisation)"""
        n = self.n_slots
        idx = candidates - self.id_base
        inside = (idx >= 0) & (idx < n)
        live = self.alive[:max(n, 1)][idx.clamp(0, max(n - 1, 0))] != 0
        return torch.where(inside & live, candidates, torch.full_like(candidates, -1))

    def _rerank(self, queries, corpus, candidates):
        return self._rerank_fn(queries, corpus, self._live_ids(candidates))

    def _fp4_rerank(self, queries, index, candidates):
        return self._fp4_rerank_fn(queries, index, self._live_ids(candidates))

    def _fp4_wide_rerank(self, queries, index, candidates):
        return self._fp4_wide_rerank_fn(queries, index, self._live_ids(candidates))

    def _retriever(self, shard, world, rank, dist, group, **hooks) -> ShardedRetriever:
        return ShardedRetriever(shard, world, rank, dist, group, select=self._select, **hooks)

    def align(self, queries, ids: torch.Tensor, maps: bool = False) -> Alignment:
        """`align` (`residual_align` over a compressed shard, which decodes the listed pages inside the kernel) over the live pages:
        a deleted id is treated as -1 (no page: (-inf, -1)), as `search(candidates=)` treats it; a surviving page's result has the
        bits of the same call over `self.view()`, before and after `compact()`."""
        return self._align_fn(queries, self.view(), self._live_ids(ids), maps=maps)

    def mine(self, queries, positives, n_neg: int, *, max_ratio: Optional[float] = None, skip_top: int = 0, compact: bool = False,
             world: int = 1, rank: int = 0, dist=None, group=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`ShardedRetriever.mine` (`mine_hard_negatives`) over the live pages: the tombstone mask goes into the mining mask, so a
        deleted page is never mined and a deleted positive bounds nothing (it is not there).  The result has the bits of
        `mine_hard_negatives` over a fresh pack of the surviving pages, positions mapped back to slots.  It scans the shard: a
        compressed one needs `score_fn=residual_scores` (NotImplementedError otherwise)."""
        r = self._retriever(self.view(), world, rank, dist, group, score_fn=self._score_fn, mine_bounds_fn=self._mine_bounds_fn,
                            mine_mask_fn=self._mine_mask_fn)
        return r.mine(queries, positives, n_neg, max_ratio=max_ratio, skip_top=skip_top, alive=self.alive[:self.n_slots], compact=compact)

    def search(self, queries, k: int = 10, compact: bool = False, *, candidates: Optional[torch.Tensor] = None, prefilter=None,
               n_candidates: Optional[int] = None, world: int = 1, rank: int = 0, dist=None, group=None,
               filter: Optional[PageFilter] = None, filter_route: str = "auto", group_by: Optional[PageGroups] = None,
               refine: Union[Fp4Index, Fp4WideIndex, None] = None, n_refine: Optional[int] = None):
        """`ShardedRetriever.search` over the live pages: the same arguments, rules and return value; a deleted page is never
        returned, and where fewer than `k` live pages exist the tail is (-inf, -1).  `candidates=` lists may name deleted and foreign
        ids (they become -1 before the rerank).  `prefilter` is the shard's own stage 1 (`LiveCorpus.int8_index()`,
        `LiveCorpus.fp4_index()`, `LiveResidualCorpus.index`), any `Int8Index` / `Fp4Index` / `Fp4WideIndex` over the same slots, or a
        `PackedCorpus` over them (e.g. pooled pages); its scores are masked too, so all `n_candidates` are live pages.
        `filter` covers the slots (`len(filter) == len(self)`, deleted ones included) and is ANDed with the tombstones on both
        routes: the scores of deleted slots are -inf before the filter masks the rest, and a listed id that is deleted is no page to
        the rerank.  `group_by` covers the slots too (`len(group_by) == len(self)`, deleted ones included): a document is scored by
        its surviving pages, and one whose every page is deleted is not returned.  A `PageGroups` is immutable: build a new one over
        all slots after `add`.  Over a compressed shard the routes that read every row (the full scan, the mask route of `filter=`,
        `group_by=` on the scan, `mine`) are refused with `ShardedRetriever`'s NotImplementedError unless `score_fn=residual_scores`.
        `refine` / `n_refine`: the three-stage search of `ShardedRetriever.search`, under its rules (exactly one of `candidates=` /
        `prefilter=`, `n_refine` >= 1 and at most `n_candidates`, ValueError otherwise; an index of the other width than the
        shard's raises NotImplementedError) -- `refine=live.fp4_index()` at width 128 and 320 alike, or any `Fp4Index` (320-wide shard:
        `Fp4WideIndex`) over the same slots (a `LiveResidualCorpus` takes an `Fp4Index` in the same way).  The refine hook
        (`fp4_rerank_fn`; for an `Fp4WideIndex` `fp4_wide_rerank_fn`) sees the list with every deleted or foreign id replaced by
        -1, as the
        rerank does, so a deleted page is never refined, never counted among the `n_refine` survivors and never returned."""
        shard = self.view()
        if self.device.type == "cuda":     # an injected hook packs host queries itself
            queries = _as_packed(queries, self.device, compact=compact)
        r = self._retriever(shard, world, rank, dist, group, score_fn=self._score, rerank_fn=self._rerank,
                            fp4_rerank_fn=self._fp4_rerank, fp4_wide_rerank_fn=self._fp4_wide_rerank, **self._stage1_hooks(), **self._filter_fns)
        if group_by is not None:                 # (-inf, -1, -1) is already the rule there
            return r.search(queries, k, compact, candidates=candidates, prefilter=prefilter, n_candidates=n_candidates, filter=filter,
                            filter_route=filter_route, group_by=group_by, refine=refine, n_refine=n_refine)
        scores, ids = r.search(queries, k, compact, candidates=candidates, prefilter=prefilter, n_candidates=n_candidates,
                               filter=filter, filter_route=filter_route, refine=refine, n_refine=n_refine)
        return _no_page(scores, ids)             # a deleted slot that filled a short row


class LiveCorpus(_LiveShard):
    """One mutable resident shard (see the module docstring).  `capacity_rows` and `capacity_docs` are fixed at construction.

    `score_fn`, `rerank_fn`, `int8_score_fn`, `fp4_score_fn`, `fp4_wide_score_fn`, `fp4_rerank_fn`, `fp4_wide_rerank_fn`, `select`, the `filter_*_fn` and `mask_fn` are the hooks of
    `ShardedRetriever` plus the tombstone mask (`mask_fn(scores, alive) -> scores`); the defaults are the gfx950 kernels
    (`fp4_score_fn=fp6_scores` scores e2m3 query tokens against the FP4 pages, as on `ShardedRetriever`).  The scores of all three
    stage-1 hooks are masked, whichever index is passed as `prefilter=`.  Host-logic tests inject reference scorers and run on the CPU."""

    _entry = "msim_live_compact"

    def __init__(self, capacity_rows: int, capacity_docs: int, device, dtype: torch.dtype = torch.bfloat16, width: int = 128,
                 id_base: int = 0, *, bounce_bytes: Optional[int] = None, score_fn: Callable = maxsim_scores,
                 rerank_fn: Callable = rerank_scores, int8_score_fn: Callable = int8_scores, fp4_score_fn: Callable = fp4_scores,
                 fp4_wide_score_fn: Callable = fp4_wide_scores, select: Callable = topk,
                 mask_fn: Callable = mask_scores, align_fn: Callable = align, mine_bounds_fn: Callable = mine_bounds,
                 mine_mask_fn: Callable = mine_mask, filter_mask_fn: Callable = filter_mask, filter_list_fn: Callable = filter_list,
                 filter_ids_fn: Callable = filter_ids, group_reduce_fn: Callable = group_reduce, group_select_fn: Callable = group_select,
                 fp4_rerank_fn: Callable = fp4_rerank_scores, fp4_wide_rerank_fn: Callable = fp4_wide_rerank_scores):
        capacity_rows, capacity_docs = self._capacity(capacity_rows, capacity_docs)
        _lib.dtype_code(dtype)                                   # raises for anything but bf16 / f16 / f32
        self.device = torch.device(device)
        self.dtype, self.dim = dtype, int(width)
        self.width = _lib.kernel_width(self.dim, dtype)          # physical row width (zero columns appended, as pack_passages)
        self.blob = torch.zeros((capacity_rows, self.width), dtype=dtype, device=self.device)
        self._init_slots(capacity_rows, capacity_docs, self.device, id_base, score_fn=score_fn, rerank_fn=rerank_fn,
                         stage1_fns=dict(int8_score_fn=int8_score_fn, fp4_score_fn=fp4_score_fn, fp4_wide_score_fn=fp4_wide_score_fn),
                         select=select, mask_fn=mask_fn, align_fn=align_fn, mine_bounds_fn=mine_bounds_fn, mine_mask_fn=mine_mask_fn,
                         filter_mask_fn=filter_mask_fn, filter_list_fn=filter_list_fn, filter_ids_fn=filter_ids_fn,
                         group_reduce_fn=group_reduce_fn, group_select_fn=group_select_fn, fp4_rerank_fn=fp4_rerank_fn, fp4_wide_rerank_fn=fp4_wide_rerank_fn)
        self._i8_codes: Optional[torch.Tensor] = None
        self._i8_scales: Optional[torch.Tensor] = None
        self._f4_codes: Optional[torch.Tensor] = None
        self._f4_scales: Optional[torch.Tensor] = None
        row_bytes = self.width * self.blob.element_size()
        self.bounce_bytes = min(self._bounce_want(bounce_bytes, row_bytes), capacity_rows * row_bytes) // 16 * 16
        if self.device.type == "cuda":
            self._ws = self._alloc_compaction(3)                 # one offset plan for the rows, one for the int8 codes, one for the FP4 index
            self._off_tmp = torch.zeros((capacity_docs + 1,), dtype=torch.int32, device=self.device)

    @classmethod
    def from_packed(cls, corpus: PackedCorpus, spare_rows: int, spare_docs: int, **kw) -> "LiveCorpus":
        """A live corpus holding the pages of `corpus` (one device copy) plus room for `spare_rows` rows and `spare_docs` pages."""
        lens = cls._source_lengths(corpus)
        n, rows = int(lens.size), int(lens.sum())
        live = cls(rows + int(spare_rows), n + int(spare_docs), corpus.device, corpus.blob.dtype, int(corpus.blob.shape[1]),
                   corpus.id_base, **kw)
        live.blob[:rows].copy_(corpus.blob[:rows])
        live._adopt(corpus.offsets, lens)
        return live

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write the used prefix of this shard -- rows, slot table, tombstones; the int8 index is rebuilt by `int8_index()` and the FP4
        index by `fp4_index()` after `load`, neither is written -- to `path` (colpali_amd/persist.py)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, capacity_rows=None, capacity_docs=None, *, verify: bool = True, **kw) -> "LiveCorpus":
        """The shard saved at `path`, on `device`, with its saved capacity or a larger one; slot ids, tombstones and the next id
        handed out are the saved shard's; `**kw` go to the constructor (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, capacity_rows=capacity_rows, capacity_docs=capacity_docs, expect=cls, **kw)

    @property
    def _widths(self) -> Tuple[int, ...]:
        return (self.dim, self.width)

    def view(self) -> PackedCorpus:
        """The used prefix as a `PackedCorpus` (zero-copy slices), valid until the next `add` / `compact`.  Every slot is a
        document: a deleted one keeps its rows until `compact()` and is an empty document afterwards."""
        n = self.n_slots
        return PackedCorpus(blob=self.blob[:max(self._rows_used, 1)], offsets=self.offsets[:n + 1], clamp0=None,
                            lengths=torch.from_numpy(self._lengths[:n].copy()), id_base=self.id_base)

    def _write_rows(self, pages, lens, dim, n0, r0):
        """host pages go through the pinned staging upload; a page tensor is copied (on the device: from the caller's memory)"""
        n, total = int(lens.size), int(lens.sum())
        dst = self.blob[r0:r0 + total]
        if isinstance(pages, torch.Tensor):
            src = pages.reshape(total, dim).to(self.device, non_blocking=True)
            dst[:, :dim].copy_(src)
            if dim < self.width:
                dst[:, dim:].zero_()
            return torch.arange(1, n + 1, dtype=torch.int32, device=self.device) * int(lens[0]) + self.offsets[n0]
        image = host_list_image(pages, "pages") if self.device.type == "cuda" and dim == self.width else None
        if image is not None:
            keep, srcs, rows, _, _ = image
            prefix = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(rows * (dim * pages[0].element_size()), out=prefix[1:])
            _staging.of(self.device).upload_image(srcs, prefix, n, dst.view(torch.uint8).view(-1),
                                                  torch.cuda.current_stream(self.device))
            del keep
        else:
            dst.copy_(_widen(torch.cat([p.to(self.device) for p in pages], dim=0)))
        return None

    def _added(self, lo, hi):
        if self._i8_codes is not None:
            self._encode_i8(lo, hi)
        if self._f4_codes is not None:                   # the new pages own the tail of the rows in use
            self._encode_f4(self._rows_used - int(self._lengths[lo:hi].sum()), self._rows_used)

    def _move_rows(self, rows_bound):
        if self.device.type != "cuda":
            raise RuntimeError("compaction is a gfx950 kernel (msim_live_compact): this corpus lives on " + str(self.device))
        n = self.n_slots
        if self._i8_codes is not None:                   # the same moves on the code rows, against a copy of the old offsets
            self._off_tmp[:n + 1].copy_(self.offsets[:n + 1])
            self._compact_rows(self._i8_codes, I8_DIM, rows_bound, self._off_tmp, 1)
            self._i8_scales[:n].masked_fill_(self.alive[:n] == 0, 0.0)      # an empty page has scale 0 (msim_i8_encode_docs)
        if self._f4_codes is not None:                   # ... and on the FP4 code rows and scale bytes, against a fresh copy of them
            self._off_tmp[:n + 1].copy_(self.offsets[:n + 1])
            with torch.cuda.device(self.device):
                rc = _lib.lib().msim_f4_live_compact(_lib.ptr(self._f4_codes), int(self._f4_codes.shape[1]), _lib.ptr(self._f4_scales),
                                                     rows_bound, _lib.ptr(self._off_tmp), _lib.ptr(self.alive), n,
                                                     _lib.ptr(self._rows_used_dev[2:]), _lib.ptr(self._ws[2]), _lib.ptr(self._bounce),
                                                     self.bounce_bytes, _lib.current_stream_handle(self.device))
            _lib.check(rc, "msim_f4_live_compact")
        self._compact_rows(self.blob, self.width * self.blob.element_size(), rows_bound, self.offsets, 0)

    def _compact_rows(self, rows: torch.Tensor, row_bytes: int, bound: int, offsets: torch.Tensor, which: int) -> None:
        with torch.cuda.device(self.device):
            rc = _lib.lib().msim_live_compact(_lib.ptr(rows), row_bytes, bound, _lib.ptr(offsets), _lib.ptr(self.alive), self.n_slots,
                                              _lib.ptr(self._rows_used_dev[which:]), _lib.ptr(self._ws[which]), _lib.ptr(self._bounce),
                                              self.bounce_bytes, _lib.current_stream_handle(self.device))
        _lib.check(rc, "msim_live_compact")

    # ------------------------------------------------------------------------------------------------------------- int8 index
    def _encode_i8(self, lo: int, hi: int, chunk_docs: int = 65536) -> None:
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for a in range(lo, hi, chunk_docs):
                b = min(hi, a + chunk_docs)
                rc = L.msim_i8_encode_docs(_lib.dtype_code(self.dtype), _lib.ptr(self.blob), _lib.ptr(self.offsets[a:]), b - a,
                                           self._rows_used, I8_DIM, _lib.ptr(self._i8_codes), _lib.ptr(self._i8_scales[a:]),
                                           _lib.current_stream_handle(self.device))
                _lib.check(rc, "msim_i8_encode_docs")

    def int8_index(self) -> Int8Index:
        """The int8 token-level index of this corpus, kept in step from the first call on: `add` encodes the new pages only,
        `compact` moves the code rows as it moves the embedding rows.  Its bits equal `Int8Index.build(self.view())`.  Like
        `view()`, the returned object is valid until the next `add` / `compact`."""
        if self._i8_codes is None:
            if self.device.type != "cuda":
                raise RuntimeError("the int8 index is built by gfx950 kernels: this corpus lives on " + str(self.device))
            if self.dtype not in (torch.bfloat16, torch.float16) or self.width != I8_DIM:
                raise NotImplementedError(f"the int8 index takes bfloat16 / float16 pages of width {I8_DIM} "
                                          f"(got {self.dtype}, width {self.width})")
            self._i8_codes = torch.zeros((self.capacity_rows, I8_DIM), dtype=torch.int8, device=self.device)
            self._i8_scales = torch.zeros((self.capacity_docs,), dtype=torch.float32, device=self.device)
            self._encode_i8(0, self.n_slots)
        n = self.n_slots
        return Int8Index(self._i8_codes[:max(self._rows_used, 1)], self._i8_scales[:n], self.offsets[:n + 1], None,
                         torch.from_numpy(self._lengths[:n].copy()), self.id_base)

    # -------------------------------------------------------------------------------------------------------------- fp4 index
    def _encode_f4(self, r0: int, r1: int) -> None:
        """FP4 code rows and scale bytes of blob rows r0 .. r1 - 1, written where they belong (the scale pointer may be unaligned)"""
        if r1 <= r0:
            return
        name = F4_FAMILIES[self.width].encode["e2m1"]
        with torch.cuda.device(self.device):
            rc = getattr(_lib.lib(), name)(_lib.dtype_code(self.dtype), _lib.ptr(self.blob[r0:]), r1 - r0, self.width,
                                           _lib.ptr(self._f4_codes[r0:]), _lib.ptr(self._f4_scales[r0:]),
                                           _lib.current_stream_handle(self.device))
        _lib.check(rc, name)

    def fp4_index(self) -> Union[Fp4Index, Fp4WideIndex]:
        """The FP4 token-level index of this corpus -- an `Fp4Index` at width 128, an `Fp4WideIndex` at width 320 -- kept in step
        from the first call on: `add` encodes the new rows only, `compact` moves the code rows and scale bytes as it moves the
        embedding rows (msim_f4_live_compact).  The first call allocates 65 / 161 bytes per capacity row and encodes the rows in
        use; nothing is allocated later.  Its bits equal `Fp4Index.build(self.view())` / `Fp4WideIndex.build(self.view())`.  Like
        `view()`, the returned object is valid until the next `add` / `compact`."""
        if self._f4_codes is None:
            if self.device.type != "cuda":
                raise RuntimeError("the fp4 index is built by gfx950 kernels: this corpus lives on " + str(self.device))
            if self.dtype not in (torch.bfloat16, torch.float16) or self.width not in F4_FAMILIES:
                raise NotImplementedError(f"the fp4 index takes bfloat16 / float16 pages of width {' or '.join(map(str, F4_FAMILIES))} "
                                          f"(got {self.dtype}, width {self.width})")
            self._f4_codes = torch.zeros((self.capacity_rows, self.width // 2), dtype=torch.uint8, device=self.device)
            self._f4_scales = torch.zeros((self.capacity_rows,), dtype=torch.uint8, device=self.device)
            self._encode_f4(0, self._rows_used)
        n, rows = self.n_slots, max(self._rows_used, 1)
        cls = F4_FAMILIES[self.width].cls
        return cls(self._f4_codes[:rows], self._f4_scales[:rows], self.offsets[:n + 1], None, torch.from_numpy(self._lengths[:n].copy()),
                   self.id_base)

    def drop_fp4_index(self) -> None:
        """Release the FP4 index (65 / 161 bytes per capacity row); a later `fp4_index()` rebuilds it from the rows."""
        self._f4_codes = self._f4_scales = None
