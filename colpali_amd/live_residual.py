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

The slot table and everything that follows from it alone -- the validation and the commit of `add`, `delete`, the bookkeeping of
`compact`, `check`, `search`, `mine`, `align` -- is `_LiveShard` (colpali_amd/live.py), shared with `LiveCorpus`; this file holds
the compressed storage, the encoding of new rows and the call that moves them.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from .centroid import CentroidIndex, _check_centroids, centroid_scores
from .corpus import _staging, host_list_image
from .filter import filter_ids, filter_list, filter_mask
from .fp4_index import fp4_rerank_scores
from .group import group_reduce, group_select
from .live import _LiveShard, mask_scores
from .mine import mine_bounds, mine_mask
from .residual import DIM, ResidualCorpus, _check_bits, _check_codec, _require_kind, residual_align, residual_rerank_scores
from .retrieval import ShardedRetriever, topk
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


class LiveResidualCorpus(_LiveShard):
    """One mutable compressed shard (see the module docstring).  `capacity_rows`, `capacity_docs`, `ingest_rows` and `bounce_bytes`
    are fixed at construction, and everything a later call needs -- the ingest buffer, the bounce buffer, the workspace -- is
    allocated there: no later call allocates in the library.

    `score_fn`, `rerank_fn`, `centroid_score_fn`, `fp4_rerank_fn`, `align_fn`, `select`, the `filter_*_fn`, `group_*_fn`, `mine_*_fn` and `mask_fn` are
    the hooks of `ShardedRetriever` plus the tombstone mask; `encode_fn(live, rows, offsets, n_pages, max_rows, dst_row0)` and
    `compact_fn(live, rows_bound)` write the arrays.  The defaults are the gfx950 kernels; host-logic tests inject reference
    functions and run on the CPU.  As over a `ResidualCorpus`, the routes that scan the shard are refused unless a scorer of the
    compressed rows is handed in: `score_fn=residual_scores`."""

    _entry = "msim_res_live_compact"
    _widths = (DIM,)

    def __init__(self, centroids: torch.Tensor, cutoffs: torch.Tensor, weights: torch.Tensor, bits: int, capacity_rows: int,
                 capacity_docs: int, id_base: int = 0, *, ingest_rows: Optional[int] = None, bounce_bytes: Optional[int] = None,
                 score_fn: Callable = maxsim_scores, rerank_fn: Callable = residual_rerank_scores,
                 centroid_score_fn: Callable = centroid_scores, select: Callable = topk, mask_fn: Callable = mask_scores,
                 mine_bounds_fn: Callable = mine_bounds, mine_mask_fn: Callable = mine_mask, filter_mask_fn: Callable = filter_mask,
                 filter_list_fn: Callable = filter_list, filter_ids_fn: Callable = filter_ids, group_reduce_fn: Callable = group_reduce,
                 group_select_fn: Callable = group_select, encode_fn: Callable = append_encode, compact_fn: Callable = compact_arrays,
                 align_fn: Callable = residual_align, fp4_rerank_fn: Callable = fp4_rerank_scores):
        bits = _check_bits(bits)
        _check_centroids(centroids)
        _check_codec(cutoffs, weights, bits)
        capacity_rows, capacity_docs = self._capacity(capacity_rows, capacity_docs)
        dev = centroids.device
        for name, t in (("cutoffs", cutoffs), ("weights", weights)):
            if t.device != dev:
                raise ValueError(f"{name} live on {t.device}, the centroids on {dev}")
        self.centroids, self.cutoffs, self.weights, self.bits = centroids, cutoffs, weights, bits
        self.codes = torch.zeros((capacity_rows,), dtype=torch.int16, device=dev).view(torch.uint16)
        self.residuals = torch.zeros((capacity_rows, 16 * bits), dtype=torch.uint8, device=dev)
        self._init_slots(capacity_rows, capacity_docs, dev, id_base, score_fn=score_fn, rerank_fn=rerank_fn,
                         stage1_fns=dict(centroid_score_fn=centroid_score_fn),       # the single stage-1 hook this class masks
                         select=select, mask_fn=mask_fn, align_fn=align_fn, mine_bounds_fn=mine_bounds_fn, mine_mask_fn=mine_mask_fn,
                         filter_mask_fn=filter_mask_fn, filter_list_fn=filter_list_fn, filter_ids_fn=filter_ids_fn,
                         group_reduce_fn=group_reduce_fn, group_select_fn=group_select_fn, fp4_rerank_fn=fp4_rerank_fn)
        self._encode_fn, self._compact_fn = encode_fn, compact_fn
        self.ingest_rows = min(DEFAULT_INGEST_ROWS if ingest_rows is None else int(ingest_rows), capacity_rows)
        if self.ingest_rows < 1:
            raise ValueError("ingest_rows must be positive")
        row_bytes = 16 * bits + 2                                    # what one row of the shard occupies: its residuals and its code
        self.bounce_bytes = min(self._bounce_want(bounce_bytes, row_bytes), (capacity_rows * row_bytes + 15) // 16 * 16)
        self._ingest = torch.zeros((self.ingest_rows, DIM), dtype=centroids.dtype, device=dev)
        if dev.type == "cuda":
            self._ws = self._alloc_compaction(1)[0]                  # one offset plan, both arrays moved against it

    # ------------------------------------------------------------------------------------------------------------ construction
    @classmethod
    def like(cls, rc: ResidualCorpus, capacity_rows: int, capacity_docs: int, id_base: int = 0, **kw) -> "LiveResidualCorpus":
        """An empty shard with the codec of `rc` (its centroids, cutoffs, weights and bits; the tensors are shared, not copied):
        train on a sample that fits, then stream the corpus in."""
        _require_kind(rc, ResidualCorpus, "the live form")             # a ResidualWideCorpus: NotImplementedError, no live form at 320
        return cls(rc.centroids, rc.cutoffs, rc.weights, rc.bits, capacity_rows, capacity_docs, id_base, **kw)

    @classmethod
    def from_residual(cls, rc: ResidualCorpus, spare_rows: int, spare_docs: int, **kw) -> "LiveResidualCorpus":
        """A live shard holding the pages of `rc` (one device copy of its codes and residuals) plus room for `spare_rows` rows and
        `spare_docs` pages."""
        _require_kind(rc, ResidualCorpus, "the live form")             # a ResidualWideCorpus: NotImplementedError, no live form at 320
        lens = cls._source_lengths(rc)
        n, rows = int(lens.size), int(lens.sum())
        live = cls.like(rc, rows + int(spare_rows), n + int(spare_docs), rc.id_base, **kw)
        live.codes.view(torch.int16)[:rows].copy_(rc.codes.view(torch.int16)[:rows])
        live.residuals[:rows].copy_(rc.residuals[:rows])
        live._adopt(rc.offsets, lens)
        return live

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write the used prefix of this shard -- rows, slot table, tombstones, codec and centroids -- to `path` (colpali_amd/persist.py)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, capacity_rows=None, capacity_docs=None, *, verify: bool = True, **kw) -> "LiveResidualCorpus":
        """The shard saved at `path`, on `device`, with its saved capacity or a larger one; slot ids, tombstones and the next id
        handed out are the saved shard's; `**kw` go to the constructor (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, capacity_rows=capacity_rows, capacity_docs=capacity_docs, expect=cls, **kw)

    # ------------------------------------------------------------------------------------------------------------------ state
    @property
    def device(self) -> torch.device:
        return self.codes.device

    @property
    def dtype(self) -> torch.dtype:
        return self.centroids.dtype

    @property
    def n_centroids(self) -> int:
        return int(self.centroids.shape[0])

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
    def _write_rows(self, pages, lens, dim, n0, r0):
        """Encode the pages to the tail of both arrays; the rows are not kept.  A list goes through the ingest buffer, `ingest_rows`
        rows per round (host tensors by the pinned staging upload; a page may straddle rounds); a page tensor on the device is
        encoded straight from the caller's memory."""
        if not isinstance(pages, torch.Tensor):
            return self._add_list(pages, lens, dim, r0)
        n, per, dev = int(lens.size), int(lens[0]), self.device
        src = pages.to(dev, non_blocking=True).reshape(n * per, DIM)
        src = src if src.is_contiguous() else src.contiguous()
        offs = torch.arange(0, n + 1, dtype=torch.int32, device=dev) * per
        self._encode_fn(self, src, offs, n, per, r0)
        return offs[1:] + self.offsets[n0]

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

    # ---------------------------------------------------------------------------------------------------------------- compact
    def _move_rows(self, rows_bound):
        self._compact_fn(self, rows_bound)

    # ----------------------------------------------------------------------------------------------------------------- search
    def _retriever(self, shard, world, rank, dist, group, **hooks) -> ShardedRetriever:
        r = super()._retriever(shard, world, rank, dist, group, **hooks)
        r._res_refuses = self._score_fn is maxsim_scores        # the rule of a ResidualCorpus: scanned on request only
        return r
