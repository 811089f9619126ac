"""Sharded-corpus retrieval: fused MaxSim per shard, deterministic top-k, RCCL merge.

The reference has no sharded retrieval (its scorer is single-device and returns the full
[n_q, n_p] matrix on the CPU, colpali_engine/utils/processing_utils.py:180-186; its only top-k
API is the experimental get_topk_plaid, :189-219).  This module is the MI355X-native piece
BASELINE.json config 4 asks for: the pre-embedded corpus is sharded by contiguous id ranges, one
process per GPU; each rank scores its resident shard and keeps its best k per query; ONE
all-gather of [n_q, k] (score f32, id i64) over RCCL/xGMI and a k-way merge give every rank the
global top-k.  The order is total -- (score descending, id ascending) -- so the answer does not
depend on the number of shards.
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Optional, Tuple, Union

import torch

from . import _lib
from .align import Alignment, align
from .binary_index import BinaryIndex, binary_scores
from ._fp4_family import Index as Fp4FamilyIndex
from .fp4_index import Fp4Index, fp4_rerank_scores, fp4_scores, fp6_rerank_scores, fp6_scores
from .fp4_wide_index import Fp4WideIndex, fp4_wide_rerank_scores, fp4_wide_scores, fp6_wide_rerank_scores, fp6_wide_scores
from .corpus import PackedCorpus, PackedQueries, _as_packed, _dtype_width, _id_list, _rerank_args
from .fde import FdeIndex, fde_scores
from .fde_wide import FdeWideIndex, fde_wide_scores
from . import filter as _filter
from .filter import PageFilter, filter_ids, filter_list, filter_mask
from .group import SELECT_MAX_M, PageGroups, group_reduce, group_select
from .centroid import CentroidIndex, centroid_scores
from .int8_index import Int8Index, int8_scores
from .mine import check_mine_args, mine_bounds, mine_mask, mine_masked, select_window
from .residual import ResidualCorpus, residual_align, residual_rerank_scores, residual_scores
from .residual_wide import (CentroidWideIndex, ResidualWideCorpus, centroid_wide_scores, residual_wide_align, residual_wide_rerank_scores,
                            residual_wide_scores)
from .scoring import _require_gpu, maxsim_scores


def shard_range(n_total: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous id range [lo, hi) of `rank`; the first n_total % world ranks hold one more."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    q, r = divmod(n_total, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


TOPK_MAX_K = 8192                 # include/maxsim.h: MSIM_TOPK_DEEP_MAX_K -- the longest list `topk` (and every route through it) selects
_TOPK_SEGMENT_MAX_K = 1024        # msim_topk_f32's own limit: up to here nothing changed


def topk(scores: torch.Tensor, k: int, id_base: int = 0, ids: Optional[torch.Tensor] = None,
         out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-wise top-k on the GPU, ordered by (score desc, id asc); pads with (-inf, -1).  1 <= k <= TOPK_MAX_K (8192).

    scores: fp32 [n_q, n] (device). ids: optional int64 [n_q, n] candidate ids (default id_base + column).
    out: optional preallocated contiguous (fp32 [n_q, k], int64 [n_q, k]) to write into.
    """
    L = _lib.lib()
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.device.type != "cuda":
        raise ValueError("scores must be a 2-D fp32 tensor on the GPU")
    if scores.stride(1) != 1 and scores.shape[1] > 1:
        scores = scores.contiguous()
    n_q, n = scores.shape
    ld = scores.stride(0) if n_q > 1 else max(n, 1)
    if ids is not None:
        if ids.shape != scores.shape or ids.dtype != torch.int64 or ids.device != scores.device:
            raise ValueError("ids must be int64 with the shape/device of scores")
        if not ids.is_contiguous() or ld != max(n, 1):
            ids = ids.contiguous()
            scores = scores.contiguous()
            ld = max(n, 1)
    dev = scores.device
    if out is not None:
        out_s, out_i = out
        if (out_s.shape != (n_q, k) or out_i.shape != (n_q, k) or out_s.dtype != torch.float32 or out_i.dtype != torch.int64
                or not out_s.is_contiguous() or not out_i.is_contiguous() or out_s.device != dev or out_i.device != dev):
            raise ValueError("out must be contiguous (fp32 [n_q, k], int64 [n_q, k]) tensors on the scores' device")
    else:
        out_s = torch.empty((n_q, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((n_q, k), dtype=torch.int64, device=dev)
    # k <= 1024: the chained-segment kernels; above, up to TOPK_MAX_K, the radix select (include/maxsim.h: msim_topk_deep_f32) --
    # the same order bit for bit; beyond that the deep entry refuses (NotImplementedError through _lib.check)
    name, entry, ws_bytes = (("msim_topk_f32", L.msim_topk_f32, L.msim_topk_workspace_bytes) if k <= _TOPK_SEGMENT_MAX_K else
                             ("msim_topk_deep_f32", L.msim_topk_deep_f32, L.msim_topk_deep_workspace_bytes))
    ws = _lib.workspace(ws_bytes(n_q, n, k), dev)
    with torch.cuda.device(dev):
        rc = entry(_lib.ptr(scores), _lib.ptr(ids), n_q, n, ld, k, id_base, _lib.ptr(out_s), _lib.ptr(out_i),
                   _lib.ptr(ws), _lib.current_stream_handle(dev))
    _lib.check(rc, name)
    return out_s, out_i


def _rank_major_rows(part: torch.Tensor) -> torch.Tensor:
    """[world, n_q, k] -> [n_q, world * k]: every query's entries, rank after rank"""
    world, n_q, k = part.shape
    return part.permute(1, 0, 2).reshape(n_q, world * k).contiguous()


def merge_gathered(all_s: torch.Tensor, all_i: torch.Tensor, k: int,
                   select: Callable = topk) -> Tuple[torch.Tensor, torch.Tensor]:
    """[world, n_q, k] gathered candidates -> global [n_q, k]."""
    return select(_rank_major_rows(all_s), k, 0, _rank_major_rows(all_i))


def _dist(dist=None):
    """the collective library: the one handed in, or torch.distributed"""
    if dist is None:
        import torch.distributed as dist  # noqa: PLW0642 - the default collective library
    return dist


def _gather_rows(n_q: int, k: int, n_ids: int, device: torch.device, world: int, dist, group, fill: Callable):
    """THE message of the retrieval collectives: every rank's [n_q, k] entries -- fp32 scores and `n_ids` int64 blocks -- as
    [n_q, world * k] tensors, the same on every rank, after ONE all-gather (RCCL over xGMI under the nccl backend).  A rank's message
    is [scores fp32 n_q*k | pad to 8 | n_ids x int64 n_q*k]: 4 + 8 * n_ids bytes per entry.  `fill(scores, *ids)` writes this
    rank's entries into [n_q, k] views of it (a kernel may write them in place)."""
    sb, ib = n_q * k * 4, n_q * k * 8
    sbp = (sb + 7) // 8 * 8
    parts = [(0, sb, torch.float32)] + [(sbp + j * ib, sbp + (j + 1) * ib, torch.int64) for j in range(n_ids)]
    mine = torch.empty((sbp + n_ids * ib,), dtype=torch.uint8, device=device)
    fill(*(mine[lo:hi].view(dtype).view(n_q, k) for lo, hi, dtype in parts))
    flat = torch.empty((world * mine.numel(),), dtype=torch.uint8, device=device)      # rank-major concatenation
    _dist(dist).all_gather_into_tensor(flat, mine, group=group)
    gathered = flat.view(world, mine.numel())
    return [_rank_major_rows(gathered[:, lo:hi].view(dtype).view(world, n_q, k)) for lo, hi, dtype in parts]


def shard_topk(scores: torch.Tensor, k: int, id_base: int, world: int = 1, dist=None, group=None,
               select: Callable = topk, force_collective: bool = False,
               ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-shard top-k of a local score matrix, then (world > 1) all-gather + merge.

    `scores` [n_q, n_local]: column j is document id_base + j, or ids[q, j] when `ids` is given (int64 [n_q, n_local], -1 = no
    document: reranked candidate lists).  Returns the same global
    (scores [n_q, k], ids [n_q, k]) on every rank.  `force_collective=True` sends a single rank through the
    message packing, the all-gather (RCCL under the `nccl` backend) and the strided-view merge as well: the
    multi-GPU code path, exercised on the one GPU a test box has (the result is the same by construction).
    """
    if world <= 1 and not force_collective:
        return select(scores, k, id_base, ids)

    def fill(my_s, my_i):
        if select is topk:
            topk(scores, k, id_base, ids, out=(my_s, my_i))                 # the selection kernel writes the message in place
        else:
            loc_s, loc_i = select(scores, k, id_base, ids)
            my_s.copy_(loc_s)
            my_i.copy_(loc_i)
    cand_s, cand_i = _gather_rows(scores.shape[0], k, 1, scores.device, max(world, 1), dist, group, fill)
    return select(cand_s, k, 0, cand_i)


def _no_page(scores: torch.Tensor, *ids: torch.Tensor):
    """-inf is "no page" (or no document), whatever filled the row: (scores, *ids with -1 wherever the score is -inf)"""
    none = scores == float("-inf")
    return (scores, *(torch.where(none, torch.full_like(i, -1), i) for i in ids))


def rerank_scores(queries, corpus: PackedCorpus, candidates: torch.Tensor, *, ref_rounding: bool = False,
                  out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaxSim of listed candidates (include/maxsim.h: msim_fwd_candidates at width 128, msim_fwd_candidates_wide at width 320):
    (scores fp32 [n_q, m], ids int64 [n_q, m]).

    Entry (q, j) is scored against document candidates[q, j] (a GLOBAL id) of `corpus`; an id of -1 or outside
    [id_base, id_base + len(corpus)) comes back as (-inf, -1).  `rerank` is the public form; this one is what
    `ShardedRetriever` calls per shard (its `rerank_fn`).  bfloat16 / float16, width 128 or 320 (ColQwen3), queries of at most
    128 tokens; anything else raises NotImplementedError."""
    dev = _require_gpu(corpus.device)
    q_dtype, dim = _dtype_width(queries)
    if q_dtype != corpus.blob.dtype:        # as maxsim_scores: torch.einsum raises on mixed dtypes too
        raise RuntimeError(f"expected queries and passages of one dtype, got {q_dtype} and {corpus.blob.dtype}")
    if q_dtype not in (torch.bfloat16, torch.float16) or dim not in (128, 320) or corpus.blob.shape[1] != dim:
        raise NotImplementedError(f"rerank takes bfloat16 / float16 embeddings of width 128 or 320 (got {q_dtype}, width {dim}, "
                                  f"corpus width {corpus.blob.shape[1]})")
    queries = _as_packed(queries, dev, layout="flat")
    if queries.device != dev:
        raise ValueError("queries and corpus live on different devices")
    n_q, n = len(queries), len(corpus)
    L = _lib.lib()
    with torch.cuda.device(dev):
        candidates, m, ld_cand, out, ids, ws = _rerank_args(
            n_q, dev, candidates, out, lambda m: (L.msim_fwd_candidates_workspace_bytes(n_q, m, n) if dim == 128
                                                  else L.msim_fwd_candidates_wide_workspace_bytes(n_q, m, n, dim)))
        entry = L.msim_fwd_candidates if dim == 128 else L.msim_fwd_candidates_wide
        rc = entry(_lib.dtype_code(q_dtype), _lib.ptr(queries.tokens), _lib.ptr(queries.offsets),
                   queries.offsets_host.data_ptr(), n_q, _lib.ptr(corpus.blob), _lib.ptr(corpus.offsets),
                   _lib.ptr(corpus.clamp0), n, dim, _lib.ptr(candidates), m, ld_cand, int(corpus.id_base),
                   _lib.ptr(out), max(m, 1), _lib.ptr(ids), _lib.MSIM_FLAG_REF_ROUNDING if ref_rounding else 0,
                   _lib.ptr(ws), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_fwd_candidates" if dim == 128 else "msim_fwd_candidates_wide")
    return out, ids


def rerank(queries, corpus: PackedCorpus, candidates: torch.Tensor, k: Optional[int] = None, *, ref_rounding: bool = False,
           out=None):
    """Exact MaxSim of each query against ITS candidate documents only -- the second stage of a two-stage search.

    queries: a `PackedQueries`, a host list of [len_i, dim] tensors or a [n_q, Lq, dim] tensor (packed as
    `ShardedRetriever.search` does), dim = 128 or 320 (ColQwen3), bfloat16 / float16, at most 128 tokens per query;
    candidates: int64 [n_q, m] GLOBAL ids on the corpus' device (-1 = none).
    k=None: fp32 [n_q, m] scores aligned with `candidates`; scores[q, j] has the bits of
    `maxsim_scores(queries, corpus)[q, candidates[q, j] - corpus.id_base]`, and an empty or out-of-corpus entry is -inf.
    k set: (scores [n_q, k], ids [n_q, k]) of `topk` over the listed documents -- (score desc, id asc), padded with
    (-inf, -1); an id listed twice in a row is scored twice and may appear twice.
    out: the fp32 [n_q, m] score tensor (k=None) or the (scores, ids) pair `topk` writes (k set).
    Asynchronous on torch's current stream; with a `PackedQueries` the call is hipGraph-capturable (no host synchronisation, no
    allocation inside the library call).
    `corpus` may be a `ResidualCorpus`: the listed pages are then scored straight from their compressed rows
    (`residual_rerank_scores`; width 128, no `ref_rounding`), with the bits `rerank` gives over `corpus.decompress()`; or a
    `ResidualWideCorpus` (`residual_wide_rerank_scores`; width 320, no `ref_rounding`), under the same rule."""
    scorer = partial(rerank_scores, ref_rounding=ref_rounding)
    if isinstance(corpus, (ResidualCorpus, ResidualWideCorpus)):
        if ref_rounding:
            raise NotImplementedError(f"ref_rounding over a {type(corpus).__name__}: the residual rerank has no reference-rounding form")
        scorer = residual_wide_rerank_scores if isinstance(corpus, ResidualWideCorpus) else residual_rerank_scores
    if k is None:
        return scorer(queries, corpus, candidates, out=out)[0]
    scores, ids = scorer(queries, corpus, candidates)
    return topk(scores, k, 0, ids, out=out)


# the hooks' defaults: what `ShardedRetriever._pack` packs the queries for
_KERNELS = (maxsim_scores, residual_scores, rerank_scores, residual_rerank_scores, fde_scores, int8_scores, centroid_scores, binary_scores,
            fp4_scores, fp6_scores, fp4_wide_scores, fp4_rerank_scores, fp6_rerank_scores, fp4_wide_rerank_scores, align,
            residual_align, fde_wide_scores, fp6_wide_scores, fp6_wide_rerank_scores, centroid_wide_scores, residual_wide_rerank_scores,
            residual_wide_scores, residual_wide_align)


class ShardedRetriever:
    """One instance per process/GPU; holds this rank's resident shard of the corpus.  The shard may be a `ResidualCorpus`: the
    default `rerank_fn` is then `residual_rerank_scores` and `search(candidates=)` / `search(prefilter=, n_candidates=)` work as over
    a `PackedCorpus` (`prefilter=shard.index`, or any other index over the same pages); everything that scans, reads or returns
    full-precision rows -- the full scan, `filter=`, `group_by=`, `align`, `mine` -- raises NotImplementedError.  Scanning such a
    shard decodes every row of it and is opt-in: with `score_fn=residual_scores` (or any other scorer over a `ResidualCorpus`; the
    default `maxsim_scores` is not one) the routes that need only the score matrix or the rerank open -- the full scan, `filter=`
    on the mask, list and auto routes (the list route runs the residual rerank), `group_by=` on every route, `filter=` with
    `candidates=` / `prefilter=`, and `mine` -- each with the bits of the same call over `shard.decompress()`.  `align` is opened
    the same way, by its own hook: `align_fn=residual_align` decodes the listed pages inside the alignment kernel; with the default
    `align_fn` it keeps raising.  A `ResidualWideCorpus` (width 320) works the same way: the default `rerank_fn` is
    `residual_wide_rerank_scores`, `prefilter=shard.index` is its `CentroidWideIndex`, `refine=` takes an `Fp4WideIndex`, and
    `score_fn=residual_wide_scores` opens the same scanning routes -- the full scan, `filter=` on the mask, list and auto routes,
    `group_by=` on every route, `filter=` with `candidates=` / `prefilter=`, and `mine` -- each with the bits of the same call over
    `shard.decompress()` scored by the flat kernel every ragged batch runs (`search`'s note on width 320 says where a scan of the
    decompressed pages runs another kernel).  `align` is opened by `align_fn=residual_wide_align` (`residual_align` exists at width
    128 only and refuses such a shard); with the default `align_fn` it keeps raising, whatever `score_fn`."""

    def __init__(self, shard: PackedCorpus, world: int = 1, rank: int = 0, dist=None, group=None,
                 score_fn: Callable = maxsim_scores, select: Callable = topk, force_collective: bool = False,
                 rerank_fn: Callable = rerank_scores, fde_score_fn: Callable = fde_scores,
                 int8_score_fn: Callable = int8_scores, centroid_score_fn: Callable = centroid_scores, binary_score_fn: Callable = binary_scores, fp4_score_fn: Callable = fp4_scores, fp4_wide_score_fn: Callable = fp4_wide_scores, align_fn: Callable = align, mine_bounds_fn: Callable = mine_bounds,
                 mine_mask_fn: Callable = mine_mask, filter_mask_fn: Callable = filter_mask, filter_list_fn: Callable = filter_list,
                 filter_ids_fn: Callable = filter_ids, group_reduce_fn: Callable = group_reduce, group_select_fn: Callable = group_select,
                 fp4_rerank_fn: Callable = fp4_rerank_scores, fp4_wide_rerank_fn: Callable = fp4_wide_rerank_scores,
                 fde_wide_score_fn: Callable = fde_wide_scores, centroid_wide_score_fn: Callable = centroid_wide_scores):
        if isinstance(shard, ResidualCorpus) and rerank_fn is rerank_scores:
            rerank_fn = residual_rerank_scores
        if isinstance(shard, ResidualWideCorpus) and rerank_fn is rerank_scores:
            rerank_fn = residual_wide_rerank_scores
        self.shard, self.world, self.rank = shard, world, rank
        self.dist, self.group = (_dist(dist) if world > 1 else dist), group
        self._score, self._select = score_fn, select
        # a compressed shard is scanned on request only: a scorer of its own must be handed in (residual_scores / residual_wide_scores)
        self._res_refuses = isinstance(shard, (ResidualCorpus, ResidualWideCorpus)) and score_fn is maxsim_scores
        self._rerank = rerank_fn          # (queries, corpus, candidates) -> (scores [n_q, m], ids [n_q, m]), (-inf, -1) off the shard
        self._fde_score = fde_score_fn    # (queries, FdeIndex) -> fp32 [n_q, len(index)]: stage 1 of prefilter=<FdeIndex>
        self._fde_wide_score = fde_wide_score_fn  # (queries, FdeWideIndex) -> fp32 [n_q, len(index)]: stage 1 of prefilter=<FdeWideIndex>
        self._int8_score = int8_score_fn  # (queries, Int8Index) -> fp32 [n_q, len(index)]: stage 1 of prefilter=<Int8Index>
        self._centroid_score = centroid_score_fn  # (queries, CentroidIndex) -> fp32 [n_q, len(index)]: stage 1 of prefilter=<CentroidIndex>
        self._centroid_wide_score = centroid_wide_score_fn  # (queries, CentroidWideIndex) -> fp32 [n_q, len(index)]: stage 1 of prefilter=<CentroidWideIndex>
        self._binary_score = binary_score_fn  # (queries, BinaryIndex) -> fp32 [n_q, len(index)]: stage 1 of prefilter=<BinaryIndex>
        # the FP4 family's hooks by the index's width (Fp4Index: 128, Fp4WideIndex: 320): (stage 1 of prefilter=<index>: (queries,
        # index) -> fp32 [n_q, len(index)]; the refine stage of refine=<index>: (queries, index, candidates) -> (scores, ids) [n_q, m])
        self._fp4_hooks = {128: (fp4_score_fn, fp4_rerank_fn), 320: (fp4_wide_score_fn, fp4_wide_rerank_fn)}
        self._align = align_fn            # (queries, corpus, ids, maps=) -> Alignment, (-inf, -1) off the shard
        self._mine_bounds = mine_bounds_fn    # (scores, csr, id_base, local=, alive=) -> fp32 [n_q]: the best in-shard positive of each query
        self._mine_mask = mine_mask_fn        # (scores, csr, id_base, bounds, max_ratio, alive) -> scores, -inf where ineligible
        self._filter_mask = filter_mask_fn    # (scores, PageFilter, alive) -> scores, -inf where the page is not allowed
        self._filter_list = filter_list_fn    # (PageFilter, n_q, m_cap, alive) -> (cand int64 [n_q, m_cap], counts, status)
        self._filter_ids = filter_ids_fn      # (ids, PageFilter, alive) -> ids, -1 where an in-shard id is not allowed (in place)
        self._group_reduce = group_reduce_fn  # (scores, PageGroups) -> (fp32 [n_q, G], int64 [n_q, G]): every document's best page
        self._group_select = group_select_fn  # (scores, gids, pages, k) -> the k best documents of every candidate row
        self.force_collective = force_collective

    def search(self, queries, k: int = 10, compact: bool = False, *, candidates: Optional[torch.Tensor] = None,
               prefilter=None, n_candidates: Optional[int] = None, filter: Optional[PageFilter] = None,
               filter_route: str = "auto", group_by: Optional[PageGroups] = None, refine: Union[Fp4Index, Fp4WideIndex, None] = None,
               n_refine: Optional[int] = None):
        """queries (replicated on every rank): a `PackedQueries`, a list of [len_i, 128] tensors, or a [n_q, Lq, 128] tensor.
        A host list is packed into the flat layout (ragged lengths, zero rows dropped on the way into the staging buffer).  A dense
        DEVICE tensor is scored as it stands unless `compact=True`: dropping its zero padding rows needs the per-query counts on the
        host (one small D2H + a synchronisation), which would make a call that is otherwise fully asynchronous and hipGraph-capturable
        block the host (round-4 advisor finding).  Callers with heavily padded query boxes pass `compact=True`, or pack once with
        `pack_queries` and hand the `PackedQueries` over; the scores are the same either way (a zero row adds exactly 0).

        Reranking (`rerank`): `candidates` -- int64 [n_q, m] GLOBAL ids, the same on every rank -- scores each query against its listed
        documents only: every rank reranks the ids it holds, then the same all-gather and merge run.  `prefilter` -- a `PackedCorpus`
        over the same documents as the shard (same count, same id_base; any rows per document, e.g. pooled pages) -- makes the list
        here: stage 1 scores the prefilter and keeps the GLOBAL top `n_candidates` (one all-gather: the list is the same on every rank,
        so the answer does not depend on the number of shards), stage 2 reranks that list exactly on the full-resolution shard.
        `prefilter` may also be an `FdeIndex` of the shard (same count, same id_base): stage 1 is then the fixed-dimensional-encoding
        GEMM (`fde_scores`), under the same rules; or an `Int8Index` of the shard or of its pooled pages: stage 1 is then the int8
        token-level scan (`int8_scores`); or a `CentroidIndex` of the shard: stage 1 is then the centroid-code scan
        (`centroid_scores`).  With world > 1 every rank must build its `CentroidIndex` from the SAME centroids: stage-1 scores of
        different centroid sets are not comparable, and the global top `n_candidates` is taken across the shards.  Or a
        `BinaryIndex` of the shard or of its pooled pages: stage 1 is then the 1-bit sign scan (`binary_scores`); it has no trained
        parameter, so its scores are comparable across shards as they stand.  Or an `Fp4Index` of the shard or of its pooled
        pages: stage 1 is then the FP4 scan (`fp4_scores`), comparable across shards in the same way.  Or, over a 320-wide shard,
        an `Fp4WideIndex` of it: stage 1 is then `fp4_wide_scores`, under the same rules, and stage 2 the 320-wide rerank; or an
        `FdeWideIndex` of it: stage 1 is then the encoding GEMM at width 320 (`fde_wide_scores`); or a `CentroidWideIndex` of it:
        stage 1 is then the centroid-code scan behind the 320-wide query table (`centroid_wide_scores`), under the rules of a
        `CentroidIndex` -- with world > 1 every rank must build it from the SAME centroids.  An `FdeIndex` or a `CentroidIndex` over
        a 320-wide shard, or an `FdeWideIndex` or a `CentroidWideIndex` over a 128-wide one, raises ValueError.

        Filtered search: `filter` -- a `PageFilter` over this shard (same count, same id_base, same device; ValueError otherwise, and
        for a per-query filter whose rows differ from the number of queries) -- restricts every query to its allowed pages.  For each
        query the result is the allowed pages whose full-scan score is not -inf, ordered by (score descending, id ascending), cut
        at k and padded with (-inf, -1); the scores carry the bits of `maxsim_scores(queries, shard)`.  An id is -1 WHEREVER the
        score is -inf: unlike the unfiltered search, an empty (0-row) page never comes back with its id.  The answer does not depend
        on the number of shards.  Two routes give that answer, chosen by `filter_route`:
          "mask"  the scan as without a filter, -inf over the columns that are not allowed (`filter_mask`), the top-k.  Every dtype
                  and width the scan takes.
          "list"  the allowed pages of every query as an id list (`filter_list`, `filter.max_allowed` wide), `rerank_scores` on that
                  list, the top-k: only the allowed pages are read.  The formats of `rerank` (bfloat16 / float16, width 128 or 320,
                  queries of at most 128 tokens; NotImplementedError otherwise); not with `candidates=` / `prefilter=` (ValueError).
          "auto"  "list" when the formats fit, neither `candidates=` nor `prefilter=` is given, n_q x max_allowed < 2^31 and
                  max_allowed <= len(shard) x `filter.LIST_ROUTE_MAX_FRACTION`; "mask" otherwise.
        At width 128 the two routes are bit-identical.  At width 320 the rerank carries the bits of the flat scan kernel every ragged
        batch runs; a scan of ONE query length and at most four 32-token tiles runs another kernel, whose token sum is a butterfly:
        against such a scan the list route agrees to the bound include/maxsim.h states for msim_fwd_candidates_wide, not bit for bit.
        With `prefilter=` the filter masks the stage-1 scores, so all `n_candidates` are allowed pages, and a candidate whose stage-1
        score is -inf becomes -1 (it is not reranked); stage 2 is unchanged.  With `candidates=` the disallowed ids of this shard
        become -1 before the rerank (`filter_ids`).  `search` calls `filter.prepare()` on first use (one host synchronisation); with
        a prepared filter and a `PackedQueries` the call is hipGraph-capturable.

        Document-level search: `group_by` -- a `PageGroups` over this shard (same count, same id_base, same device; ValueError
        otherwise) -- makes the call return the k best DOCUMENTS instead of the k best pages: (scores, group_ids, page_ids), each
        [n_q, k].  A document's score is the score of its best page among those the route may return (allowed by `filter`, listed
        by `candidates=` / kept by `prefilter=`, live in a `LiveCorpus`, and not scoring -inf); the order is (score descending,
        document id ascending); `page_ids` is that best page -- the lower id on a tie --, ready for `align`; the padding is
        (-inf, -1, -1), and -inf always comes with -1 / -1.  The scores carry the bits of the route's scorer.  Without `group_by`
        nothing changes: the return stays (scores, ids).  The routes:
          full scan    the scan, `group_reduce` (every document's best page, [n_q, G] in ascending document-id order), the `topk`
                       over the documents -- its column order is the tie order.
          candidates= / prefilter=   stage 1 and the rerank run unchanged: candidates stay PAGES and `n_candidates` counts PAGES, not
                       documents; the reranked list is mapped to document ids and `group_select` keeps the k best documents.  Lists
                       of at most 4096 entries (NotImplementedError beyond).
          filter=      "mask" masks, then reduces; "list" lists, reranks, then `group_select`: "auto" takes it only when its rule
                       above holds AND max_allowed <= 4096, an explicit "list" beyond raises NotImplementedError.  The two routes give
                       the same bits and ids wherever they do without `group_by`.
        With world > 1 (or `force_collective`) every rank computes its local top-k documents, ONE all-gather carries
        [scores | pad to 8 | document ids | page ids] (20 bytes per entry) and `group_select` runs over the world x k gathered
        entries (world x k <= 4096, ValueError otherwise).  This is exact: a document's global score is the maximum of its per-rank
        scores, so it is attained on the rank R that holds its best page.  If the document is in the global top k it is in R's
        local top k: any document ranked above it on R has a local score no better than its global one, so it ranks above it
        globally as well, and there are fewer than k of those.  Its best entry therefore reaches the merge, which deduplicates
        documents that several ranks sent.  The answer does not depend on the number of shards, also where a document's pages
        straddle a boundary.  `search` calls `group_by.prepare()` on first use (one host synchronisation); with prepared groups
        and a `PackedQueries` the call is hipGraph-capturable.

        Three-stage search: `refine` -- an `Fp4Index` over a 128-wide shard's pages or an `Fp4WideIndex` over a 320-wide shard's
        (same count, same id_base, same device; ValueError otherwise) -- puts the FP4 rows between a cheap first stage and the
        exact rerank.  It needs exactly one of `candidates=` /
        `prefilter=` (ValueError otherwise) and `n_refine` >= 1, at most `n_candidates` with `prefilter=` (ValueError otherwise;
        `n_refine` without `refine` is a ValueError too).  Once the candidate list exists -- from stage 1, filtered, or the caller's
        list behind `filter_ids` -- the refine hook (`fp4_rerank_fn`, default `fp4_rerank_scores`; `fp6_rerank_scores` codes the query
        tokens as e2m3; for an `Fp4WideIndex` `fp4_wide_rerank_fn`, default `fp4_wide_rerank_scores`) scores the listed pages of
        this shard from their 65-byte (width 320: 161-byte) FP4 rows, and the top `n_refine` of those scores
        are kept through the same all-gather and merge as every other list: the refined list is identical on every rank and does
        not depend on the number of shards.  An entry the refine stage scored -inf (no page, an empty page) becomes -1 and is not
        reranked.  The exact rerank then runs on the `n_refine` survivors, unchanged, so every returned score is still the exact
        one.  With `group_by=`, `n_refine` counts PAGES and the 4096-entry limit applies to `n_refine`, not to `n_candidates`.  A
        `ResidualCorpus` shard (or, with an `Fp4WideIndex`, a `ResidualWideCorpus` one) works as it does with `prefilter=`: the last
        stage is its own rerank.  An index of the other width
        -- an `Fp4WideIndex` on a 128-wide shard, an `Fp4Index` on a 320-wide one -- raises NotImplementedError.  With
        `refine=None` every route runs exactly as it did.

        How long a list may be: every selection here is `topk`, which takes 1 .. `TOPK_MAX_K` = 8192 entries (NotImplementedError
        beyond) -- `k`, `n_candidates` and `n_refine` alike, on the scan, behind `candidates=` / `prefilter=` / `refine=`, on the
        filter's mask route, on a live shard, and for the per-rank message and the world x k wide merge of a sharded search.  Up
        to 1024 the kernels are the ones that always ran; above, the radix select (`msim_topk_deep_f32`) gives the same order bit
        for bit.  Two limits are not `topk`'s and stay: `group_by=` selects documents with `group_select` (lists of at most 4096
        pages, k <= 1024), and the filter's "list" route lists at most 4096 allowed pages per query."""
        if n_candidates is not None and prefilter is None:
            raise ValueError("n_candidates goes with prefilter=")
        n_refine = self._check_refine(refine, n_refine, candidates, prefilter, n_candidates)
        if self._res_refuses:
            if filter is not None or group_by is not None:
                self._no_rows("search(filter=) and search(group_by=)")
            if candidates is None and prefilter is None:
                self._no_rows("the full scan")
        groups = self._check_groups(group_by, k)
        if filter is not None:
            return self._search_filtered(queries, k, compact, candidates, prefilter, n_candidates, filter, filter_route, groups,
                                         refine, n_refine)
        if filter_route != "auto":
            raise ValueError("filter_route goes with filter=")
        if candidates is not None or prefilter is not None:
            return self._search_candidates(queries, k, compact, candidates, prefilter, n_candidates, groups=groups, refine=refine,
                                           n_refine=n_refine)
        scores = self._score(self._pack(queries, compact, self._score), self.shard)
        if groups is not None:
            return self._group_scan(scores, k, groups)
        return self._topk(scores, k, self.shard.id_base)

    def _pack(self, queries, compact: bool, *fns: Callable, layout: str = "auto"):
        """The queries as the hooks in play (`fns`) take them: packed (`_as_packed`) when one of them is a kernel of ours; an injected
        stand-in receives the caller's queries untouched and packs them itself if it has to."""
        if any(f in _KERNELS for f in fns):
            return _as_packed(queries, self.shard.device, layout=layout, compact=compact)
        return queries

    def _topk(self, scores: torch.Tensor, k: int, id_base: int, ids: Optional[torch.Tensor] = None):
        """this shard's top-k, then the merge across the ranks (`shard_topk`)"""
        return shard_topk(scores, k, id_base, self.world, self.dist, self.group, self._select, force_collective=self.force_collective,
                          ids=ids)

    def _check_covers(self, what: str, x, noun: str = "pages", lives: Optional[str] = None):
        """`x` -- group_by, filter or prefilter -- must cover the shard: same count, same id_base and, for what the kernels read
        next to the scores (`lives` words that message), the same device"""
        shard = self.shard
        if len(x) != len(shard) or x.id_base != shard.id_base:
            raise ValueError(f"{what} {len(x)} {noun} from id {x.id_base}; the shard holds {len(shard)} from id {shard.id_base}: "
                             f"it must cover the same {noun}")
        if lives is not None and x.device != shard.device:
            raise ValueError(f"the {lives} on {x.device}, the shard on {shard.device}")

    def _check_refine(self, refine, n_refine, candidates, prefilter, n_candidates) -> Optional[int]:
        """the rules of `search(refine=, n_refine=)`; returns n_refine as an int (None without refine)"""
        if refine is None:
            if n_refine is not None:
                raise ValueError("n_refine goes with refine=")
            return None
        width = getattr(self.shard, "width", 128)
        if width == 320 and isinstance(refine, Fp4WideIndex):
            pass                                                         # the wide pair: fp4_wide_rerank_fn
        elif isinstance(refine, Fp4WideIndex) or width != 128:
            raise NotImplementedError("refine takes an Fp4Index of a 128-wide shard")
        elif not isinstance(refine, Fp4Index):
            raise ValueError("refine must be an Fp4Index")
        if (candidates is None) == (prefilter is None):
            raise ValueError("refine= cuts a candidate list: it needs exactly one of candidates= / prefilter=")
        self._check_covers("refine covers", refine, lives="refine index lives")
        if n_refine is None or int(n_refine) < 1:
            raise ValueError("refine= needs n_refine >= 1")
        if prefilter is not None and n_candidates is not None and int(n_refine) > int(n_candidates):
            raise ValueError(f"n_refine={int(n_refine)} exceeds the list of n_candidates={int(n_candidates)} pages it is cut from")
        return int(n_refine)

    def _no_rows(self, what: str):
        if isinstance(self.shard, ResidualWideCorpus):
            raise NotImplementedError(f"{what} over a ResidualWideCorpus: the shard keeps no full-precision rows and only candidate "
                                      "lists are scored from the compressed ones -- use search(candidates=) or "
                                      "search(prefilter=shard.index, n_candidates=), or shard.decompress() for a PackedCorpus; "
                                      "ShardedRetriever(shard, score_fn=residual_wide_scores) opts in to scanning the compressed rows "
                                      "(the full scan, filter=, group_by= and mine).  align needs rows either way; `residual_align` "
                                      "exists at width 128 only: at width 320 pass align_fn=residual_wide_align, which decodes the "
                                      "listed pages inside the alignment kernel")
        raise NotImplementedError(f"{what} over a ResidualCorpus: the shard keeps no full-precision rows and only candidate lists are "
                                  "scored from the compressed ones -- use search(candidates=) or search(prefilter=shard.index, "
                                  "n_candidates=), or shard.decompress() for a PackedCorpus; ShardedRetriever(shard, "
                                  "score_fn=residual_scores) opts in to scanning the compressed rows (the full scan, filter=, "
                                  "group_by= and mine; align needs rows either way: ShardedRetriever(shard, "
                                  "align_fn=residual_align) decodes the listed pages inside the alignment kernel)")

    # ------------------------------------------------------------------------------------------------- document-level search
    def _check_groups(self, groups, k) -> Optional[PageGroups]:
        if groups is None:
            return None
        if not isinstance(groups, PageGroups):
            raise ValueError("group_by must be a PageGroups")
        self._check_covers("group_by covers", groups, lives="groups live")
        collective = self.world > 1 or self.force_collective
        if collective and max(self.world, 1) * int(k) > SELECT_MAX_M:
            raise ValueError(f"group_by with world={max(self.world, 1)} and k={k}: the merge selects among world x k gathered "
                             f"entries, at most {SELECT_MAX_M}")
        return groups.prepare()

    def _group_scan(self, scores: torch.Tensor, k: int, groups: PageGroups):
        """a score matrix over the shard's pages -> this shard's best k documents, then the merge"""
        n_q, g = scores.shape[0], groups.n_groups
        if g == 0:
            top_s = torch.full((n_q, k), float("-inf"), dtype=torch.float32, device=scores.device)
            gid = torch.full((n_q, k), -1, dtype=torch.int64, device=scores.device)
            page = gid.clone()
        else:
            doc_s, doc_p = self._group_reduce(scores, groups)
            top_s, col = self._select(doc_s, k, 0, None)               # columns are in ascending document-id order: the tie order
            c = col.clamp(0, g - 1)
            gid = torch.where(col >= 0, groups.group_ids[c], torch.full_like(col, -1))
            page = torch.where(col >= 0, torch.gather(doc_p, 1, c), torch.full_like(col, -1))
        return self._group_merge(*_no_page(top_s, gid, page), k)

    def _group_list(self, scores: torch.Tensor, ids: torch.Tensor, k: int, groups: PageGroups):
        """reranked (scores, page ids) rows -> this shard's best k documents, then the merge"""
        if scores.shape[1] > SELECT_MAX_M:
            raise NotImplementedError(f"group_by over a list of {scores.shape[1]} pages: group_select takes at most {SELECT_MAX_M}")
        return self._group_merge(*self._group_select(scores, groups.doc_ids(ids), ids, k), k)

    def _group_merge(self, top_s, gid, page, k: int):
        """(world > 1) ONE all-gather of every rank's k best documents, and the grouped selection over the world x k entries"""
        if self.world <= 1 and not self.force_collective:
            return _no_page(top_s, gid, page)

        def fill(*views):
            for view, mine in zip(views, (top_s, gid, page)):
                view.copy_(mine)
        gathered = _gather_rows(top_s.shape[0], k, 2, top_s.device, max(self.world, 1), self.dist, self.group, fill)
        return _no_page(*self._group_select(*gathered, k))

    def align(self, queries, ids: torch.Tensor, maps: bool = False) -> Alignment:
        """Explain hits (`align`): for every entry of `ids` -- int64 [n_q, m] GLOBAL ids, the same on every rank, e.g. what `search`
        returned -- the best-matching page row of every query token and its similarity.  Every rank aligns the ids it holds; with
        world > 1 one element-wise MAX all-reduce of (best_sim, best_row, ids) follows: a rank that does not hold an id contributes
        (-inf, -1, -1), so every rank ends up with the holder's result (best_row is relative to the page, whichever rank holds it).
        `maps=True` is for a single shard: the maps of a sharded corpus stay on the rank that holds the page (ValueError).
        Over a `ResidualCorpus` the default `align_fn` refuses (NotImplementedError); `align_fn=residual_align` decodes the listed
        pages inside the kernel and gives the bits of the same call over `shard.decompress()`.  Over a `ResidualWideCorpus` the
        hook is `align_fn=residual_wide_align`, under the same rule."""
        if isinstance(self.shard, (ResidualCorpus, ResidualWideCorpus)) and self._align is align:  # opt-in, as the scan: align_fn=residual_align / residual_wide_align
            self._no_rows("align")
        if maps and self.world > 1:
            raise ValueError("maps=True with world > 1: similarity maps are made by the rank that holds the page; call align() on "
                             "its shard")
        out = self._align(self._pack(queries, False, self._align, layout="flat"), self.shard, ids, maps=maps)
        if self.world > 1:
            for t in (out.best_sim, out.best_row, out.ids):
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.group)
            out.page_lengths = None        # this shard's page lengths do not describe the other ranks' pages
        return out

    def mine(self, queries, positives, n_neg: int, *, max_ratio: Optional[float] = None, skip_top: int = 0,
             alive: Optional[torch.Tensor] = None, compact: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Hard negatives over the whole sharded corpus (`mine_hard_negatives`: same rule, same arguments, the same result on every
        rank): (neg_scores fp32 [n_q, n_neg], neg_ids int64 [n_q, n_neg]).  `positives` (replicated, GLOBAL ids) may live on any
        shard: each rank takes the maximum over the positives it holds (-inf where it holds none), ONE all-reduce MAX of fp32 [n_q]
        makes that the global bound of the `max_ratio` rule, each rank masks and selects its best `skip_top + n_neg` locally, and the
        all-gather + merge of `search` runs over those; the `skip_top` window is cut after the merge, so the answer does not depend
        on the number of shards.  `alive`: this shard's uint8 tombstones.  Queries are packed as `search` packs them."""
        if self._res_refuses:
            self._no_rows("mine")
        n_neg, skip_top, max_ratio = check_mine_args(n_neg, skip_top, max_ratio)
        scores = self._score(self._pack(queries, compact, self._score), self.shard)
        if alive is not None and alive.device != scores.device:
            raise ValueError("alive and the shard live on different devices")
        reduce_max = None
        if self.world > 1:
            def reduce_max(t):
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.group)
        masked = mine_masked(scores, positives, int(self.shard.id_base), max_ratio, alive, self._mine_bounds, self._mine_mask, reduce_max)
        return select_window(masked, int(self.shard.id_base), n_neg, skip_top, self._topk)

    def _list_formats_fit(self, queries) -> bool:
        """what `rerank_scores` takes: bfloat16 / float16, width 128 or 320, at most 128 tokens per query (host metadata only)"""
        q_dtype, dim = _dtype_width(queries)
        if q_dtype != self.shard.dtype or q_dtype not in (torch.bfloat16, torch.float16) or dim not in (128, 320) or self.shard.width != dim:
            return False
        if isinstance(queries, PackedQueries):
            return len(queries) == 0 or int(queries.lengths.max()) <= 128
        if isinstance(queries, torch.Tensor):
            return int(queries.shape[1]) <= 128
        return all(int(q.shape[0]) <= 128 for q in queries)

    def _search_filtered(self, queries, k, compact, candidates, prefilter, n_candidates, flt, route, groups=None, refine=None,
                         n_refine=None):
        if route not in ("auto", "mask", "list"):
            raise ValueError(f"filter_route={route!r}: 'auto', 'mask' or 'list'")
        if not isinstance(flt, PageFilter):
            raise ValueError("filter must be a PageFilter")
        shard = self.shard
        self._check_covers("filter covers", flt, lives="filter lives")
        two_stage = candidates is not None or prefilter is not None
        if two_stage:
            if route == "list":
                raise ValueError("filter_route='list' lists the allowed pages itself: it does not go with candidates= / prefilter=")
            if groups is not None:
                return self._search_candidates(queries, k, compact, candidates, prefilter, n_candidates, flt, groups, refine, n_refine)
            top_s, top_i = self._search_candidates(queries, k, compact, candidates, prefilter, n_candidates, flt, refine=refine,
                                                   n_refine=n_refine)
        else:
            queries = self._pack(queries, compact, self._score)
            n_q = len(queries)
            self._check_filter_rows(flt, n_q)
            flt.prepare()
            fits = self._list_formats_fit(queries)
            if route == "list" and not fits:
                q_dtype, dim = _dtype_width(queries)
                raise NotImplementedError(f"filter_route='list' reranks the listed pages: rerank takes bfloat16 / float16 embeddings of "
                                          f"width 128 or 320 and queries of at most 128 tokens (got {q_dtype}, width {dim}, corpus "
                                          f"{shard.dtype} of width {shard.width})")
            if route == "list" and groups is not None and flt.max_allowed > SELECT_MAX_M:
                raise NotImplementedError(f"filter_route='list' with group_by: a query is allowed {flt.max_allowed} pages, group_select "
                                          f"takes lists of at most {SELECT_MAX_M}")
            if route == "auto":
                route = "list" if (fits and n_q * flt.max_allowed < 2**31
                                   and flt.max_allowed <= len(shard) * _filter.LIST_ROUTE_MAX_FRACTION
                                   and (groups is None or flt.max_allowed <= SELECT_MAX_M)) else "mask"
            if route == "list":
                cand = self._filter_list(flt, n_q, max(flt.max_allowed, 1), None)[0]
                scores, ids = self._rerank(queries, shard, cand)
                if groups is not None:
                    return self._group_list(scores, ids, k, groups)
                top_s, top_i = self._topk(scores, k, 0, ids)
            else:
                scores = self._filter_mask(self._score(queries, shard), flt, None)
                if groups is not None:
                    return self._group_scan(scores, k, groups)
                top_s, top_i = self._topk(scores, k, shard.id_base)
        return _no_page(top_s, top_i)

    @staticmethod
    def _check_filter_rows(flt, n_q):
        if flt.rows is not None and flt.rows != n_q:
            raise ValueError(f"a per-query filter of {flt.rows} rows was given for {n_q} queries")

    def _search_candidates(self, queries, k, compact, candidates, prefilter, n_candidates, flt=None, groups=None, refine=None,
                           n_refine=None):
        if candidates is not None and prefilter is not None:
            raise ValueError("pass either candidates= or prefilter=, not both")
        if groups is not None:
            m = int(n_refine) if refine is not None else int(n_candidates) if prefilter is not None and n_candidates is not None else (
                int(candidates.shape[-1]) if isinstance(candidates, torch.Tensor) and candidates.dim() == 2 else 0)
            if m > SELECT_MAX_M:
                raise NotImplementedError(f"group_by over a list of {m} pages: group_select takes at most {SELECT_MAX_M}")
        if prefilter is not None:
            if not isinstance(prefilter, (PackedCorpus, FdeIndex, Int8Index, CentroidIndex, BinaryIndex, Fp4Index, Fp4WideIndex,
                                          FdeWideIndex, CentroidWideIndex)):
                raise ValueError("prefilter must be a PackedCorpus, an FdeIndex, an Int8Index, a CentroidIndex or a BinaryIndex, or an Fp4Index or an Fp4WideIndex"
                                 ", or an FdeWideIndex, or a CentroidWideIndex")
            if isinstance(prefilter, (FdeIndex, FdeWideIndex)):
                width = getattr(self.shard, "width", 128)                 # the two classes differ by the shard's 320 only
                if (width == 320) != isinstance(prefilter, FdeWideIndex):
                    raise ValueError(f"prefilter is an {type(prefilter).__name__}, the shard is {width} wide: a 320-wide shard takes "
                                     "an FdeWideIndex, any other an FdeIndex")
            if isinstance(prefilter, (CentroidIndex, CentroidWideIndex)):
                width = getattr(self.shard, "width", 128)
                if (width == 320) != isinstance(prefilter, CentroidWideIndex):
                    raise ValueError(f"prefilter is a {type(prefilter).__name__}, the shard is {width} wide: a 320-wide shard takes "
                                     "a CentroidWideIndex, any other a CentroidIndex")
            self._check_covers("prefilter holds", prefilter, "documents")
            if n_candidates is None or int(n_candidates) < 1:
                raise ValueError("prefilter= needs n_candidates >= 1")
        stage1 = (self._fde_score if isinstance(prefilter, FdeIndex) else self._fde_wide_score if isinstance(prefilter, FdeWideIndex)
                  else self._int8_score if isinstance(prefilter, Int8Index)
                  else self._centroid_score if isinstance(prefilter, CentroidIndex)
                  else self._centroid_wide_score if isinstance(prefilter, CentroidWideIndex)
                  else self._binary_score if isinstance(prefilter, BinaryIndex)
                  else self._fp4_hooks[prefilter.family.dim][0] if isinstance(prefilter, Fp4FamilyIndex) else self._score)
        fine = self._fp4_hooks[refine.family.dim][1] if refine is not None else None
        queries = self._pack(queries, compact, self._rerank, *((stage1,) if prefilter is not None else ()),
                             *((fine,) if refine is not None else ()))
        if flt is not None:
            self._check_filter_rows(flt, len(queries))
        if prefilter is not None:
            coarse = stage1(queries, prefilter)                          # stage 1: the cheap corpus, or the encodings
            if flt is not None:
                coarse = self._filter_mask(coarse, flt, None)            # all n_candidates are allowed pages
            cand_s, candidates = self._topk(coarse, int(n_candidates), prefilter.id_base)
            if flt is not None:                                          # a masked column that filled a short list is not reranked
                candidates = _no_page(cand_s, candidates)[1]
        elif flt is not None:
            mine = _id_list(candidates, len(queries), self.shard.device, "candidates")[0]
            if mine is candidates:                                       # filter_ids writes in place: never into the caller's list
                mine = mine.clone(memory_format=torch.contiguous_format)
            candidates = self._filter_ids(mine, flt, None)
        if refine is not None:                                           # the FP4 rows cut the list: this shard's entries, then the merge
            fine_s, fine_i = fine(queries, refine, candidates)
            candidates = _no_page(*self._topk(fine_s, n_refine, 0, fine_i))[1]
        scores, ids = self._rerank(queries, self.shard, candidates)      # the last stage: exact, this shard's candidates only
        if groups is not None:
            return self._group_list(scores, ids, k, groups)
        return self._topk(scores, k, 0, ids)


def _query_box(queries_embeddings: torch.Tensor, shard) -> torch.Tensor:
    """the [n, Lq, dim] box an index's `search` is handed, on the shard's device and in its dtype"""
    q = queries_embeddings.to(device=shard.device, dtype=shard.dtype).contiguous()
    if q.dim() != 3:
        raise ValueError("queries_embeddings must be [n_queries, query_length, dim]")
    return q


def _hit_rows(top_s: torch.Tensor, top_i: torch.Tensor):
    """FastPlaid's result shape: per query a list of (document id, score) tuples, best first; the (-inf, -1) padding is dropped"""
    top_s, top_i = top_s.cpu().tolist(), top_i.cpu().tolist()
    return [[(int(i), float(s)) for s, i in zip(row_s, row_i) if i >= 0] for row_s, row_i in zip(top_s, top_i)]


class ExactMaxSimIndex:
    """What `create_plaid_index` returns here: the resident packed corpus behind the interface the reference's
    `get_topk_plaid` talks to -- `index.search(queries_embeddings=[n, Lq, dim], top_k=k)` (processing_utils.py:217-220).
    The reference delegates that call to the third-party `fast_plaid.search.FastPlaid` (not vendored in the reference
    checkout, unpinned: README.md:108-111 `pip install --no-deps fast-plaid fastkmeans`), an APPROXIMATE centroid-pruned
    index; this one is exact: fused MaxSim over every page + the deterministic (score desc, id asc) top-k.  `search`
    returns FastPlaid's published result shape: per query a list of (document id, score) tuples, best first."""

    def __init__(self, corpus: PackedCorpus, world: int = 1, rank: int = 0, dist=None, group=None):
        self.retriever = ShardedRetriever(corpus, world, rank, dist, group)

    def search(self, queries_embeddings: torch.Tensor, top_k: int = 10):
        q = _query_box(queries_embeddings, self.retriever.shard)
        return _hit_rows(*self.retriever.search(q, k=top_k, compact=True))     # padded blocks from get_topk_plaid: the result is read back anyway


class ResidualMaxSimIndex:
    """What `create_plaid_index(nbits=2 | 4)` returns: a `ResidualCorpus` (a `ResidualWideCorpus` for 320-wide pages) -- centroid codes plus a few residual bits per dimension,
    no full-precision embedding, as in the FastPlaid index the reference builds -- behind the same `search(queries_embeddings,
    top_k)` interface and result shape as `ExactMaxSimIndex`.  A search is approximate in the way PLAID is: centroid stage 1
    (`centroid_scores`) keeps the top `min(n_candidates, n)` pages, the residual rerank scores them from the compressed rows, the
    deterministic (score desc, id asc) top-k follows."""

    def __init__(self, corpus: ResidualCorpus, n_candidates: int = 1024, world: int = 1, rank: int = 0, dist=None, group=None):
        if int(n_candidates) < 1:
            raise ValueError("n_candidates must be >= 1")
        self.n_candidates = int(n_candidates)
        self.retriever = ShardedRetriever(corpus, world, rank, dist, group)

    def search(self, queries_embeddings: torch.Tensor, top_k: int = 10):
        rc = self.retriever.shard
        q = _query_box(queries_embeddings, rc)
        # one shard: no more candidates than pages (with world > 1 the list is global, and a short one is padded with -1)
        m = self.n_candidates if self.retriever.world > 1 else max(min(self.n_candidates, len(rc)), 1)
        return _hit_rows(*self.retriever.search(q, k=top_k, compact=True, prefilter=rc.index, n_candidates=m))


def create_plaid_index(ps, device=None, *, nbits: Optional[int] = None, n_centroids: int = 1024, n_candidates: int = 1024):
    """Drop-in for `BaseVisualRetrieverProcessor.create_plaid_index` (processing_utils.py:226-244): same arguments; builds
    the resident packed corpus instead of a FastPlaid index (see ExactMaxSimIndex).  Like the reference -- which hands
    FastPlaid the unpadded pages -- no block zero-padding semantics apply here (`batch_size=None`).
    `nbits=None` (the default) is that exact index.  `nbits` = 2 or 4 builds what FastPlaid builds instead, a compressed index:
    the pages are packed, `n_centroids` centroids and the residual codec are trained on them, a `ResidualCorpus` is built, the
    full-precision pack is dropped, and a `ResidualMaxSimIndex` (stage 1 keeps `n_candidates` pages) comes back.  320-wide
    (ColQwen3) pages give the same index over a `ResidualWideCorpus`."""
    from .corpus import pack_passages
    from .scoring import _require_gpu, get_torch_device

    if nbits is not None and (isinstance(nbits, bool) or nbits not in (2, 4)):
        raise ValueError(f"nbits must be None, 2 or 4 (got {nbits!r})")
    if len(ps) == 0:
        raise ValueError("No passages provided")
    dev = _require_gpu(device or get_torch_device("auto"))
    corpus = pack_passages(list(ps) if not isinstance(ps, torch.Tensor) else ps, dev, batch_size=None)
    if nbits is None:
        return ExactMaxSimIndex(corpus)
    kind = ResidualWideCorpus if corpus.width == 320 else ResidualCorpus
    rc = kind.build(corpus, bits=int(nbits), n_centroids=n_centroids)
    del corpus                                    # the compressed shard is all that stays resident
    return ResidualMaxSimIndex(rc, n_candidates)


def get_topk_plaid(qs, plaid_index, k: int = 10, batch_size: int = 128, device=None):
    """Drop-in for `BaseVisualRetrieverProcessor.get_topk_plaid` (processing_utils.py:189-223): the same loop over
    blocks of `batch_size` queries, `pad_sequence(padding_value=0)` per block, one `plaid_index.search(...)` per block,
    and the same return value: the list of per-block results."""
    from .scoring import get_torch_device

    device = device or get_torch_device("auto")
    if len(qs) == 0:
        raise ValueError("No queries provided")
    scores_list = []
    for i in range(0, len(qs), batch_size):
        block = qs[i: i + batch_size]
        qs_batch = torch.nn.utils.rnn.pad_sequence(list(block), batch_first=True, padding_value=0).to(device)
        scores_list.append(plaid_index.search(queries_embeddings=qs_batch, top_k=k))
    return scores_list
