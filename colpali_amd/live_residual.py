"""A live residual-compressed shard: filled from bf16 / f16 pages that are never kept, pages deleted at once, rows handed back in place.

`LiveResidualCorpus` is to `ResidualCorpus` what `LiveCorpus` is to `PackedCorpus`.  It owns the two arrays of a compressed shard
with spare capacity -- `codes` uint16 [capacity_rows] and `residuals` uint8 [capacity_rows, 16 * bits] --, the page offsets and the
tombstone mask, under ONE fixed codec (centroids, cutoffs, weights: train them on a sample that fits, `LiveResidualCorpus.like(rc,
...)`, then stream the corpus in):

  * `add` encodes the new pages straight to the tail of both arrays (msim_res_append, colpali_amd/csrc/residual_live.hip: the centroid
    search and the residual quantisation in one pass; the bits are those of `ResidualCorpus.build`).  Host pages go through the
    pinned staging upload into a fixed ingest buffer of `ingest_rows` rows, in as many rounds as it takes; a device tensor is encoded
    from the caller's memory.  The full-precision rows are never kept;
  * `delete` clears `alive`: deleted candidate ids become -1 before the rerank, and every score matrix (stage 1, the opt-in scan) is
    masked with `mask_scores`;
  * `compact` moves the codes and the residual rows of live pages down over the deleted ones against one offset plan
    (msim_res_live_compact) and turns every deleted slot into an empty page.

A page's id is its slot, `id_base + slot`, never reused.  After any history `view()` holds the bits of `ResidualCorpus.build` over
`pack_passages(surviving pages in slot order, batch_size=None)` with the same codec, and `search` returns the scores (bit for bit) of a
`ShardedRetriever` over that corpus, positions mapped back to slots.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .centroid import CentroidIndex, _check_centroids, centroid_scores
from .corpus import _as_packed, _staging, host_list_image
from .filter import PageFilter, filter_ids, filter_list, filter_mask
from .group import PageGroups, group_reduce, group_select
from .live import DEFAULT_BOUNCE_BYTES, mask_scores
from .mine import mine_bounds, mine_mask
from .align import Alignment
from .residual import DIM, ResidualCorpus, _check_bits, _check_codec, residual_align, residual_rerank_scores
from .retrieval import ShardedRetriever, _no_page, topk
from .scoring import maxsim_scores

DEFAULT_INGEST_ROWS = 1 << 18        # rows of the fixed ingest buffer (64 MiB of bf16): what one round of a host `add` uploads and encodes


def append_encode(live: "LiveResidualCorpus", rows: torch.Tensor, offsets: torch.Tensor, n_pages: int, max_rows: int,
                  dst_row0: int) -> None:
    """The default `encode_fn` (msim_res_append): the pages `offsets` (int32 [n_pages + 1], device, relative to `rows`) cuts out of
    `rows` [n, 128] -> rows dst_row0 .. dst_row0 + n - 1 of `live.codes` and `live.residuals`.  Asynchronous on torch's current
    stream, no allocation."""
    dev = live.device
    if dev.type != "cuda":
        raise RuntimeError("encoding is a gfx950 kernel (msim_res_append): this shard lives on " + str(dev))
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_res_append(_lib.dtype_code(live.dtype), _lib.ptr(rows), _lib.ptr(offsets), n_pages, int(rows.shape[0]), DIM,
                                        max_rows, _lib.ptr(live.centroids), live.n_centroids, _lib.ptr(live.cutoffs), live.bits,
                                        _lib.ptr(live.codes), _lib.ptr(live.residuals), dst_row0, live.capacity_rows, None,
                                        _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_res_append")


def compact_arrays(live: "LiveResidualCorpus", rows_bound: int) -> None:
    """The default `compact_fn` (msim_res_live_compact) over `live.codes`, `live.residuals`, `live.offsets` and `live.alive`."""
    dev = live.device
    if dev.type != "cuda":
        raise RuntimeError("compaction is a gfx950 kernel (msim_res_live_compact): this shard lives on " + str(dev))
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_res_live_compact(_lib.ptr(live.codes), _lib.ptr(live.residuals), live.bits, rows_bound, _lib.ptr(live.offsets),
                                              _lib.ptr(live.alive), live.n_slots, _lib.ptr(live._rows_used_dev), _lib.ptr(live._ws),
                                              _lib.ptr(live._bounce), live.bounce_bytes, _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_res_live_compact")


class LiveResidualCorpus:
    """One mutable compressed shard (see the module docstring).  `capacity_rows`, `capacity_docs`, `ingest_rows` and `bounce_bytes`
    are fixed at construction, and everything a later call needs -- the ingest buffer, the bounce buffer, the workspace -- is
    allocated there: no later call allocates in the library.

    `score_fn`, `rerank_fn`, `centroid_score_fn`, `align_fn`, `select`, the `filter_*_fn`, `group_*_fn`, `mine_*_fn` and `mask_fn` are
    the hooks of `ShardedRetriever` plus the tombstone mask; `encode_fn(live, rows, offsets, n_pages, max_rows, dst_row0)` and
    `compact_fn(live, rows_bound)` write the arrays.  The defaults are the gfx950 kernels; host-logic tests inject reference
    functions and run on the CPU.  As over a `ResidualCorpus`, the routes that scan the shard are refused unless a scorer of the
    compressed rows is handed in: `score_fn=residual_scores`."""

    def __init__(self, centroids: torch.Tensor, cutoffs: torch.Tensor, weights: torch.Tensor, bits: int, capacity_rows: int,
                 capacity_docs: int, id_base: int = 0, *, ingest_rows: Optional[int] = None, bounce_bytes: Optional[int] = None,
                 score_fn: Callable = maxsim_scores, rerank_fn: Callable = residual_rerank_scores,
                 centroid_score_fn: Callable = centroid_scores, select: Callable = topk, mask_fn: Callable = mask_scores,
                 mine_bounds_fn: Callable = mine_bounds, mine_mask_fn: Callable = mine_mask, filter_mask_fn: Callable = filter_mask,
                 filter_list_fn: Callable = filter_list, filter_ids_fn: Callable = filter_ids, group_reduce_fn: Callable = group_reduce,
                 group_select_fn: Callable = group_select, encode_fn: Callable = append_encode, compact_fn: Callable = compact_arrays,
                 align_fn: Callable = residual_align):
        bits = _check_bits(bits)
        _check_centroids(centroids)
        _check_codec(cutoffs, weights, bits)
        capacity_rows, capacity_docs = int(capacity_rows), int(capacity_docs)
        if capacity_rows < 1 or capacity_docs < 1:
            raise ValueError("capacity_rows and capacity_docs must be positive")
        if capacity_rows >= 2**31:
            raise NotImplementedError("more than 2^31 patch rows in one shard")
        dev = centroids.device
        for name, t in (("cutoffs", cutoffs), ("weights", weights)):
            if t.device != dev:
                raise ValueError(f"{name} live on {t.device}, the centroids on {dev}")
        self.centroids, self.cutoffs, self.weights, self.bits = centroids, cutoffs, weights, bits
        self.id_base = int(id_base)
        self.capacity_rows, self.capacity_docs = capacity_rows, capacity_docs
        self.codes = torch.zeros((capacity_rows,), dtype=torch.int16, device=dev).view(torch.uint16)
        self.residuals = torch.zeros((capacity_rows, 16 * bits), dtype=torch.uint8, device=dev)
        self.offsets = torch.zeros((capacity_docs + 1,), dtype=torch.int32, device=dev)
        self.alive = torch.zeros((capacity_docs + 1,), dtype=torch.uint8, device=dev)     # [capacity_docs]: where ids outside the shard land
        self._lengths = np.zeros((capacity_docs,), dtype=np.int64)   # host: rows each slot owns now (0 once compacted away)
        self._alive_h = np.zeros((capacity_docs,), dtype=bool)       # host mirror of `alive` (stale while _dirty)
        self._dirty = False                                          # a device-side delete has not been read back yet
        self.n_slots = 0
        self._rows_used = 0
        self._score_fn, self._rerank_fn, self._centroid_score_fn = score_fn, rerank_fn, centroid_score_fn
        self._select, self._mask_fn = select, mask_fn
        self._mine_bounds_fn, self._mine_mask_fn = mine_bounds_fn, mine_mask_fn
        self._filter_fns = dict(filter_mask_fn=filter_mask_fn, filter_list_fn=filter_list_fn, filter_ids_fn=filter_ids_fn,
                                group_reduce_fn=group_reduce_fn, group_select_fn=group_select_fn)
        self._encode_fn, self._compact_fn = encode_fn, compact_fn
        self._align_fn = align_fn         # (queries, ResidualCorpus, ids, maps=) -> Alignment
        self._compactions = 0
        self._rows_compacted = 0                                     # rows in use right after the last compaction (check())
        self.ingest_rows = min(DEFAULT_INGEST_ROWS if ingest_rows is None else int(ingest_rows), capacity_rows)
        if self.ingest_rows < 1:
            raise ValueError("ingest_rows must be positive")
        row_bytes = 16 * bits + 2                                    # what one row of the shard occupies: its residuals and its code
        want = DEFAULT_BOUNCE_BYTES if bounce_bytes is None else int(bounce_bytes)
        if want < row_bytes:
            raise ValueError(f"bounce_bytes={want} holds no row of {row_bytes} bytes")
        self.bounce_bytes = min(want, (capacity_rows * row_bytes + 15) // 16 * 16)
        self._ingest = torch.zeros((self.ingest_rows, DIM), dtype=centroids.dtype, device=dev)
        if dev.type == "cuda":
            ws_bytes = _lib.lib().msim_res_live_compact_workspace_bytes(capacity_docs, self.bounce_bytes)
            self._bounce = torch.empty((self.bounce_bytes,), dtype=torch.uint8, device=dev)
            self._ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=dev)
            self._rows_used_dev = torch.zeros((1,), dtype=torch.int64, device=dev)

    # ------------------------------------------------------------------------------------------------------------ construction
    @classmethod
    def like(cls, rc: ResidualCorpus, capacity_rows: int, capacity_docs: int, id_base: int = 0, **kw) -> "LiveResidualCorpus":
        """An empty shard with the codec of `rc` (its centroids, cutoffs, weights and bits; the tensors are shared, not copied):
        train on a sample that fits, then stream the corpus in."""
        if not isinstance(rc, ResidualCorpus):
            raise ValueError("rc must be a ResidualCorpus")
        return cls(rc.centroids, rc.cutoffs, rc.weights, rc.bits, capacity_rows, capacity_docs, id_base, **kw)

    @classmethod
    def from_residual(cls, rc: ResidualCorpus, spare_rows: int, spare_docs: int, **kw) -> "LiveResidualCorpus":
        """A live shard holding the pages of `rc` (one device copy of its codes and residuals) plus room for `spare_rows` rows and
        `spare_docs` pages."""
        if not isinstance(rc, ResidualCorpus):
            raise ValueError("rc must be a ResidualCorpus")
        if rc.clamp0 is not None:
            raise ValueError("a live shard has no block zero-padding semantics: pack with batch_size=None (clamp0 must be None)")
        lens = rc.lengths.numpy().astype(np.int64)
        if (lens <= 0).any():
            raise ValueError("a live shard holds no page of 0 rows: -inf means 'not there'")
        n, rows = int(lens.size), int(lens.sum())
        live = cls.like(rc, rows + int(spare_rows), n + int(spare_docs), rc.id_base, **kw)
        live.codes.view(torch.int16)[:rows].copy_(rc.codes.view(torch.int16)[:rows])
        live.residuals[:rows].copy_(rc.residuals[:rows])
        live.offsets[:n + 1].copy_(rc.offsets)
        live.alive[:n].fill_(1)
        live._lengths[:n] = lens
        live._alive_h[:n] = True
        live.n_slots, live._rows_used = n, rows
        return live

    # ------------------------------------------------------------------------------------------------------------------ state
    def __len__(self) -> int:
        """Slots handed out so far (live or deleted): the number of documents every view and score matrix has."""
        return self.n_slots

    @property
    def device(self) -> torch.device:
        return self.codes.device

    @property
    def dtype(self) -> torch.dtype:
        return self.centroids.dtype

    @property
    def n_centroids(self) -> int:
        return int(self.centroids.shape[0])

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
        status = int(self._ws[:4].view(torch.int32)[0].item())
        if status:
            raise _lib.MaxSimLibraryError(f"msim_res_live_compact found broken offsets (status word {status}): nothing further was moved")
        got = int(self._rows_used_dev[0].item())
        if got != self._rows_compacted:
            raise _lib.MaxSimLibraryError(f"msim_res_live_compact left {got} rows in use, the host expected {self._rows_compacted}")

    def view(self) -> ResidualCorpus:
        """The used prefix as a `ResidualCorpus` (zero-copy slices of the codes, residuals and offsets; the codec tensors are the
        shard's own), valid until the next `add` / `compact`.  Every slot is a document: a deleted one keeps its rows until
        `compact()` and is an empty document afterwards."""
        n, rows = self.n_slots, max(self._rows_used, 1)
        return ResidualCorpus(self.centroids, self.codes[:rows], self.residuals[:rows], self.cutoffs, self.weights, self.offsets[:n + 1],
                              None, torch.from_numpy(self._lengths[:n].copy()), self.id_base, self.bits)

    @property
    def index(self) -> CentroidIndex:
        """`view().index`: the centroid-code stage 1 over the same codes; valid until the next `add` / `compact`."""
        return self.view().index

    # -------------------------------------------------------------------------------------------------------------------- add
    def add(self, pages: Union[torch.Tensor, Sequence[torch.Tensor]]) -> torch.Tensor:
        """Encode and append pages; returns their ids (int64, host).  `pages`: a list of [rows_i, 128] tensors (host tensors go
        through the pinned staging upload into the ingest buffer, `ingest_rows` rows per round; a page may straddle rounds) or one
        [n, rows, 128] tensor (on the device: encoded straight from the caller's memory, nothing synchronises).  The rows are not
        kept.  Running out of rows or slots raises RuntimeError and leaves the shard as it was."""
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
            dim = int(first.shape[1]) if n else DIM
            for p in pages:
                if p.dtype != first.dtype or p.shape[1] != dim:
                    raise RuntimeError("expected pages of one dtype and one embedding width")
        if n == 0:
            return torch.empty((0,), dtype=torch.int64)
        if first.dtype != self.dtype or dim != DIM:
            raise RuntimeError(f"this shard holds {self.dtype} pages of width {DIM}, got {first.dtype} of width {dim}")
        self._sync_host()
        total, n0, r0 = int(lens.sum()), self.n_slots, self._rows_used
        if n0 + n > self.capacity_docs:
            raise RuntimeError(f"live shard is full: {n0} of capacity_docs={self.capacity_docs} slots are taken, {n} more were asked for")
        if r0 + total > self.capacity_rows:
            raise RuntimeError(f"live shard is full: {r0} of capacity_rows={self.capacity_rows} rows are in use, {total} more were "
                               "asked for (compact() hands back the rows of deleted pages)")
        dev = self.device
        if isinstance(pages, torch.Tensor):
            src = pages.to(dev, non_blocking=True).reshape(total, DIM)
            src = src if src.is_contiguous() else src.contiguous()
            offs = torch.arange(0, n + 1, dtype=torch.int32, device=dev) * per
            self._encode_fn(self, src, offs, n, per, r0)
            self.offsets[n0 + 1:n0 + n + 1].copy_(offs[1:] + self.offsets[n0])
        else:
            self._add_list(pages, lens, dim, r0)
            ends = torch.from_numpy((r0 + np.cumsum(lens)).astype(np.int32))
            self.offsets[n0 + 1:n0 + n + 1].copy_(ends)
        self.alive[n0:n0 + n].fill_(1)
        self._lengths[n0:n0 + n] = lens
        self._alive_h[n0:n0 + n] = True
        self.n_slots, self._rows_used = n0 + n, r0 + total
        return torch.arange(self.id_base + n0, self.id_base + n0 + n, dtype=torch.int64)

    def _add_list(self, pages, lens: np.ndarray, dim: int, r0: int) -> None:
        """rounds of at most `ingest_rows` rows: every round is a run of pieces (a whole page, or the part of one that fits), loaded
        into the ingest buffer and encoded from there as pages of their own -- a row's code and residual do not depend on its page"""
        dev = self.device
        image = host_list_image(pages, "pages") if dev.type == "cuda" else None
        row_bytes = DIM * self._ingest.element_size()
        page, at, done = 0, 0, 0                                    # the next piece starts at row `at` of page `page`
        n = len(pages)
        while page < n:
            pieces, room = [], self.ingest_rows
            while page < n and room > 0:
                take = min(int(lens[page]) - at, room)
                pieces.append((page, at, take))
                room -= take
                at += take
                if at == int(lens[page]):
                    page, at = page + 1, 0
            rows = self.ingest_rows - room
            cuts = np.zeros(len(pieces) + 1, dtype=np.int64)
            np.cumsum([t for _, _, t in pieces], out=cuts[1:])
            if image is not None:
                keep, srcs, _, _, _ = image
                piece_src = np.asarray([int(srcs[p]) + a * row_bytes for p, a, _ in pieces], dtype=np.uint64)
                _staging.of(dev).upload_image(piece_src, cuts * row_bytes, len(pieces), self._ingest.view(torch.uint8).view(-1)[:rows * row_bytes],
                                              torch.cuda.current_stream(dev))
            else:
                self._ingest[:rows].copy_(torch.cat([pages[p][a:a + t] for p, a, t in pieces], dim=0))
            offs = torch.from_numpy(cuts.astype(np.int32)).to(dev)
            self._encode_fn(self, self._ingest[:rows], offs, len(pieces), int(max(t for _, _, t in pieces)), r0 + done)
            done += rows

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
        """Move the codes and residual rows of live pages down over those of deleted ones, in place and in slot order; a deleted
        slot becomes an empty document; slots (ids) do not move.  Asynchronous on torch's current stream, no allocation in the
        library call.  (After a device-side `delete` the mask is read back first: one small D2H and a synchronisation.)"""
        self._sync_host()
        n = self.n_slots
        dead = ~self._alive_h[:n] & (self._lengths[:n] > 0)
        if not dead.any():
            return
        self._compact_fn(self, self._rows_used)
        self._lengths[:n][dead] = 0
        self._rows_used = self._rows_compacted = int(self._lengths[:n].sum())
        self._compactions += 1

    # ----------------------------------------------------------------------------------------------------------------- search
    def _masked(self, scores: torch.Tensor) -> torch.Tensor:
        return self._mask_fn(scores, self.alive[:self.n_slots])

    def _score(self, queries, corpus):
        return self._masked(self._score_fn(queries, corpus))

    def _centroid_score(self, queries, index):
        return self._masked(self._centroid_score_fn(queries, index))

    def _live_ids(self, candidates: torch.Tensor) -> torch.Tensor:
        """`candidates` with every id that is outside the shard or deleted replaced by -1 (on the device, no synchronisation)"""
        n = self.n_slots
        idx = candidates - self.id_base
        inside = (idx >= 0) & (idx < n)
        live = self.alive[:max(n, 1)][idx.clamp(0, max(n - 1, 0))] != 0
        return torch.where(inside & live, candidates, torch.full_like(candidates, -1))

    def _rerank(self, queries, corpus, candidates):
        return self._rerank_fn(queries, corpus, self._live_ids(candidates))

    def _retriever(self, shard, world, rank, dist, group, **hooks) -> ShardedRetriever:
        r = ShardedRetriever(shard, world, rank, dist, group, select=self._select, **hooks)
        r._res_refuses = self._score_fn is maxsim_scores        # the rule of a ResidualCorpus: scanned on request only
        return r

    def align(self, queries, ids: torch.Tensor, maps: bool = False) -> Alignment:
        """`residual_align` over the live pages, as `LiveCorpus.align`: a deleted id is treated as -1 (no page: (-inf, -1)), as
        `search(candidates=)` treats it; a surviving page's result has the bits of `residual_align(queries, self.view(), ids)`, before
        and after `compact()`.  The listed pages are decoded inside the kernel: nothing is decompressed."""
        return self._align_fn(queries, self.view(), self._live_ids(ids), maps=maps)

    def mine(self, queries, positives, n_neg: int, *, max_ratio: Optional[float] = None, skip_top: int = 0, compact: bool = False,
             world: int = 1, rank: int = 0, dist=None, group=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`ShardedRetriever.mine` over the live pages, as `LiveCorpus.mine`: the tombstone mask goes into the mining mask.  It scans
        the shard, so it needs `score_fn=residual_scores` (NotImplementedError otherwise)."""
        r = self._retriever(self.view(), world, rank, dist, group, score_fn=self._score_fn, mine_bounds_fn=self._mine_bounds_fn,
                            mine_mask_fn=self._mine_mask_fn)
        return r.mine(queries, positives, n_neg, max_ratio=max_ratio, skip_top=skip_top, alive=self.alive[:self.n_slots], compact=compact)

    def search(self, queries, k: int = 10, compact: bool = False, *, candidates: Optional[torch.Tensor] = None, prefilter=None,
               n_candidates: Optional[int] = None, world: int = 1, rank: int = 0, dist=None, group=None,
               filter: Optional[PageFilter] = None, filter_route: str = "auto", group_by: Optional[PageGroups] = None):
        """`ShardedRetriever.search` over `view()` with the arguments and rules of `LiveCorpus.search`: a deleted page is never
        returned, and where fewer than `k` live pages exist the tail is (-inf, -1).  `candidates=` lists may name deleted and foreign
        ids (they become -1 before the residual rerank); `prefilter` is `self.index`, or a `PackedCorpus` over the same slots; its
        scores are masked.  The full scan, the mask route of `filter=`, `group_by=` on the scan and `mine` read every row of the
        shard: a default instance refuses them with `ShardedRetriever`'s NotImplementedError, `score_fn=residual_scores` opens them
        (the matrix is masked too).  `align` is a method of its own."""
        shard = self.view()
        if self.device.type == "cuda":     # an injected hook packs host queries itself
            queries = _as_packed(queries, self.device, compact=compact)
        r = self._retriever(shard, world, rank, dist, group, score_fn=self._score, rerank_fn=self._rerank,
                            centroid_score_fn=self._centroid_score, **self._filter_fns)
        if group_by is not None:                 # (-inf, -1, -1) is already the rule there
            return r.search(queries, k, compact, candidates=candidates, prefilter=prefilter, n_candidates=n_candidates, filter=filter,
                            filter_route=filter_route, group_by=group_by)
        scores, ids = r.search(queries, k, compact, candidates=candidates, prefilter=prefilter, n_candidates=n_candidates,
                               filter=filter, filter_route=filter_route)
        return _no_page(scores, ids)             # a deleted slot that filled a short row
