"""Token-to-patch alignment of search hits: which page row matched each query token, and the similarity maps behind it.

The reference draws similarity maps from a dense image tensor the caller holds
(colpali_engine/interpretability/similarity_map_utils.py:9-55); in a serving process the pages live in the resident
`PackedCorpus` / `LiveCorpus`.  `align` takes the ids a search returned -- the candidate-list interface of `rerank` -- and
explains every hit in one launch (include/maxsim.h: msim_align_candidates, kernel K1a, colpali_amd/csrc/maxsim_align.hip):
per query token the best similarity and the page row that attains it, and on request the whole [tokens, rows] block.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from .corpus import PackedCorpus, _as_packed, _dtype_width, _id_list
from .scoring import _require_gpu

MAX_QUERY_TOKENS = 128


@dataclass
class Alignment:
    """What `align` returns.  T = the longest query of the call, R = `max_rows`.

    best_sim fp32 [n_q, m, T]: max_j <q_i, d_j> over the rows of page ids[q, j]; best_row int32 [n_q, m, T]: the first row
    (relative to the page) that attains it.  Under the page's clamp0 flag a token whose maximum is negative reports (0.0, -1) (the
    reference's zero padding row wins); an entry without a page (id -1, off the shard, deleted) or a page of 0 rows reports
    (-inf, -1); a token slot past the query's end reports (0.0, -1).  An entry whose page is longer than R is NaN / -1.
    ids int64 [n_q, m]: the id each entry resolved to, -1 where there was no page.
    sims fp32 [n_q, m, T, R] or None: <q_i, d_j>, -inf in the columns past the page's end and the slots past the query's end;
    best_sim is the maximum of its row bit for bit (before the clamp)."""

    best_sim: torch.Tensor
    best_row: torch.Tensor
    ids: torch.Tensor
    sims: Optional[torch.Tensor] = None
    query_lengths: Optional[torch.Tensor] = None      # int64 [n_q], host
    page_lengths: Optional[torch.Tensor] = None       # int64 [len(corpus)], host: rows of page id_base + c
    id_base: int = 0

    def similarity_maps(self, q: int, j: int, n_patches: Tuple[int, int], rows=None) -> torch.Tensor:
        """The similarity map of entry (q, j): fp32 [len(query q), n_patches_x, n_patches_y], the axis order of
        colpali_engine/interpretability/similarity_map_utils.py:46-52 ("(h w) -> w h").  `rows` selects the page rows that are image
        patches -- a slice or a bool mask over the page's rows, default all of them; their number must be n_patches_x * n_patches_y
        (ValueError otherwise, as the reference).  Reads the entry's id back to the host (one synchronisation)."""
        if self.sims is None:
            raise ValueError("this Alignment holds no maps: call align(..., maps=True)")
        if self.query_lengths is None or self.page_lengths is None:
            raise ValueError("this Alignment does not know its queries' and pages' lengths")
        nx, ny = n_patches
        page = int(self.ids[q, j]) - self.id_base
        if int(self.ids[q, j]) < 0 or not (0 <= page < self.page_lengths.numel()):
            raise ValueError(f"entry ({q}, {j}) has no page")
        n_rows = int(self.page_lengths[page])
        if n_rows > self.sims.shape[3]:
            raise ValueError(f"the page of entry ({q}, {j}) has {n_rows} rows, the maps were made with max_rows={self.sims.shape[3]}")
        sim = self.sims[q, j, :int(self.query_lengths[q]), :n_rows]
        if rows is not None:
            if isinstance(rows, torch.Tensor):
                if rows.dtype != torch.bool or rows.shape != (n_rows,):
                    raise ValueError(f"rows must be a slice or a bool mask over the page's {n_rows} rows")
                rows = rows.to(sim.device)
            elif not isinstance(rows, slice):
                raise ValueError(f"rows must be a slice or a bool mask over the page's {n_rows} rows")
            sim = sim[:, rows]
        if sim.shape[1] != nx * ny:
            raise ValueError(
                f"The number of patches ({nx} x {ny} = {nx * ny}) "
                f"does not match the number of non-padded image tokens ({sim.shape[1]}).")
        return sim.reshape(-1, ny, nx).permute(0, 2, 1)


def resolve_ids(ids: torch.Tensor, id_base: int, n: int) -> torch.Tensor:
    """`ids` with every id outside [id_base, id_base + n) replaced by -1: what Alignment.ids holds."""
    idx = ids - id_base
    return torch.where((ids >= 0) & (idx >= 0) & (idx < n), ids, torch.full_like(ids, -1))


def align(queries, corpus: PackedCorpus, ids: torch.Tensor, *, maps: bool = False, max_rows: Optional[int] = None) -> Alignment:
    """Explain search hits: for every entry (q, j) of `ids` (int64 [n_q, m] GLOBAL ids on the corpus' device, -1 = none -- what
    `search` / `rerank` return) and every token of query q, the best-matching row of page ids[q, j] and its similarity;
    `maps=True` adds the whole similarity block (see `Alignment`).

    queries: a `PackedQueries`, a host list of [len_i, dim] tensors or a [n_q, Lq, dim] tensor, packed as `rerank` packs them;
    bfloat16 / float16, width 128 or 320, at most 128 tokens per query (NotImplementedError otherwise; RuntimeError when queries and
    corpus differ in dtype; ValueError for ids of the wrong shape, dtype or device).  `max_rows` bounds the rows of a listed page
    (default: the corpus' longest page, known on the host); a longer page comes back NaN / -1.
    The bits of a similarity depend on its token row and page row alone: the same (query, page) gives the same bits at any list
    position, in any batch and under any m.  Asynchronous on torch's current stream; with a `PackedQueries` there is no host
    synchronisation and the call is hipGraph-capturable.
    A `ResidualCorpus` goes to `residual_align` (width 128; the bits of this call over `corpus.decompress()`, the pages decoded
    inside the kernel), a `ResidualWideCorpus` to `residual_wide_align` (width 320, under the same rule)."""
    from .residual import ResidualCorpus, residual_align      # residual imports this module's Alignment
    from .residual_wide import ResidualWideCorpus, residual_wide_align

    if isinstance(corpus, ResidualCorpus):
        return residual_align(queries, corpus, ids, maps=maps, max_rows=max_rows)
    if isinstance(corpus, ResidualWideCorpus):
        return residual_wide_align(queries, corpus, ids, maps=maps, max_rows=max_rows)
    dev = _require_gpu(corpus.device)
    q_dtype, dim = _dtype_width(queries)
    if q_dtype != corpus.blob.dtype:
        raise RuntimeError(f"expected queries and passages of one dtype, got {q_dtype} and {corpus.blob.dtype}")
    if q_dtype not in (torch.bfloat16, torch.float16) or dim not in (128, 320) or corpus.blob.shape[1] != dim:
        raise NotImplementedError(f"align takes bfloat16 / float16 embeddings of width 128 or 320 (got {q_dtype}, width {dim}, "
                                  f"corpus width {corpus.blob.shape[1]})")
    queries = _as_packed(queries, dev, layout="flat")
    if queries.device != dev:
        raise ValueError("queries and corpus live on different devices")
    n_q = len(queries)
    ids, m, ld = _id_list(ids, n_q, dev, "ids")
    q_lens = queries.lengths.to(torch.int64)
    T = int(q_lens.max()) if n_q else 0
    if T > MAX_QUERY_TOKENS:
        raise NotImplementedError(f"align takes queries of at most {MAX_QUERY_TOKENS} tokens (got one of {T})")
    n = len(corpus)
    if max_rows is None:
        max_rows = int(corpus.lengths.max()) if n else 0
    max_rows = int(max_rows)
    if max_rows < 0:
        raise ValueError(f"max_rows={max_rows} is negative")
    best_sim = torch.empty((n_q, m, T), dtype=torch.float32, device=dev)
    best_row = torch.empty((n_q, m, T), dtype=torch.int32, device=dev)
    sims = torch.empty((n_q, m, T, max_rows), dtype=torch.float32, device=dev) if maps else None
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_align_candidates(
            _lib.dtype_code(q_dtype), _lib.ptr(queries.tokens), _lib.ptr(queries.offsets), n_q, int(queries.tokens.shape[0]), T,
            _lib.ptr(corpus.blob), _lib.ptr(corpus.offsets), _lib.ptr(corpus.clamp0), n, int(corpus.blob.shape[0]), dim,
            _lib.ptr(ids), m, ld, int(corpus.id_base), _lib.ptr(best_sim), _lib.ptr(best_row), _lib.ptr(sims), max_rows,
            _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_align_candidates")
    return Alignment(best_sim, best_row, resolve_ids(ids, int(corpus.id_base), n), sims, q_lens, corpus.lengths, int(corpus.id_base))
