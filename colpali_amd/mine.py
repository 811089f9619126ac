"""Hard-negative mining with the model's own late-interaction score, and the page gather that feeds the explicit-negative losses.

The reference mines its negatives with a bi-encoder (scripts/compute_hardnegs.py: `einsum("bd,cd->bc")` + `topk(100)`) because a
MaxSim scan of the corpus was too slow there; here the scan is `maxsim_scores` over the resident `PackedCorpus`.  Mining is that
scan, a mask (include/maxsim.h: msim_mine_bounds, msim_mine_mask; colpali_amd/csrc/mine.hip) and the deterministic `topk`:

    s[q, c]   the scores of the full scan, the bits of `maxsim_scores(queries, corpus)`
    pos[q]    the maximum of s[q, c] over the query's positives that lie in the shard (and, under `alive`, are alive), +inf when
              it has none
    column c is ELIGIBLE for q when  c is not a positive of q,
                                     `alive` is None or alive[c] != 0,
                                     s[q, c] is not -inf (a page of 0 rows),
                                     `max_ratio` is None or  not (s[q, c] > fp32(max_ratio) * pos[q])
    result    the eligible columns ordered by (score descending, id ascending), ranks skip_top .. skip_top + n_neg - 1;
              where fewer exist the tail is (-inf, -1)

The `max_ratio` rule is the reference's false-negative filter (loss/bi_encoder_losses.py:58-59, `scores > filter_threshold *
pos_scores`): one fp32 multiply and that comparison.  SIGN QUIRK, kept as the reference has it: with pos[q] < 0 the threshold
`max_ratio * pos[q]` lies ABOVE the positive's score (0.95 x -10 = -9.5), so a page may outscore the positive by up to 5 % of |pos|
and still be kept.  `gather_pages` then slices the chosen pages out of the packed blob into the zero-padded box
`ColbertNegativeCELoss` / `ColbertPairwiseNegativeCELoss` take as `neg_doc_embeddings`.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .corpus import PackedCorpus
from .scoring import _require_gpu, maxsim_scores

Positives = Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]


def positives_csr(positives: Positives, n_q: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The three forms of `positives` as one CSR pair on `device`: (ids int64 [nnz], offsets int32 [n_q + 1]).

    int64 [n_q] (one per query, -1 = none), int64 [n_q, P] (padded with -1), or an (ids, offsets) pair already in that form.
    Only shapes and dtypes are checked (ValueError); the ids are never read on the host: -1, ids outside the shard and duplicates
    are dealt with on the device.  Tensors already on `device` are used as they are: no copy, no synchronisation."""
    device = torch.device(device)
    if isinstance(positives, (tuple, list)):
        if len(positives) != 2 or not all(isinstance(t, torch.Tensor) for t in positives):
            raise ValueError("CSR positives are a pair (ids int64 [nnz], offsets int32 [n_q + 1])")
        ids, offsets = positives
        if ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError(f"CSR positive ids must be an int64 [nnz] tensor (got {ids.dtype}, {tuple(ids.shape)})")
        if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] != n_q + 1:
            raise ValueError(f"CSR offsets must be an int32 [n_q + 1 = {n_q + 1}] tensor (got {offsets.dtype}, {tuple(offsets.shape)})")
        return ids.to(device).contiguous(), offsets.to(device).contiguous()
    if not isinstance(positives, torch.Tensor) or positives.dtype != torch.int64:
        raise ValueError("positives must be an int64 tensor [n_q] or [n_q, P], or a CSR pair (ids int64, offsets int32)")
    if positives.dim() not in (1, 2) or positives.shape[0] != n_q:
        raise ValueError(f"positives must have shape [n_q = {n_q}] or [n_q = {n_q}, P] (got {tuple(positives.shape)})")
    per = 1 if positives.dim() == 1 else int(positives.shape[1])
    if n_q * per >= 2**31:
        raise NotImplementedError("more than 2^31 - 1 positives in one call")
    ids = positives.to(device).reshape(-1).contiguous()
    offsets = torch.arange(0, (n_q + 1) * per, per, dtype=torch.int32, device=device) if per else \
        torch.zeros((n_q + 1,), dtype=torch.int32, device=device)
    return ids, offsets


def _scores_ld(scores: torch.Tensor, what: str) -> int:
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.device.type != "cuda":
        raise ValueError(f"{what}: scores must be a 2-D fp32 tensor on the GPU (a gfx950 kernel; there is no CPU fallback)")
    n_q, n = scores.shape
    if n > 1 and scores.stride(1) != 1:
        raise ValueError(f"{what}: scores must have unit inner stride")
    return scores.stride(0) if n_q > 1 else max(n, 1)


def _check_csr(csr, n_q: int, device, what: str):
    ids, offsets = csr
    if (ids.dtype != torch.int64 or offsets.dtype != torch.int32 or offsets.shape != (n_q + 1,) or ids.device != device
            or offsets.device != device or not ids.is_contiguous() or not offsets.is_contiguous()):
        raise ValueError(f"{what}: positives must be the (ids int64 [nnz], offsets int32 [n_q + 1]) pair of positives_csr on {device}")
    return ids, offsets


def _check_alive(alive: Optional[torch.Tensor], n: int, dev) -> None:
    if alive is not None and (alive.dtype != torch.uint8 or alive.dim() != 1 or alive.shape[0] < n or alive.device != dev
                              or not alive.is_contiguous()):
        raise ValueError(f"alive must be a contiguous uint8 [>= {n}] tensor on {dev}")


def mine_bounds(scores: torch.Tensor, csr, id_base: int = 0, *, local: bool = False,
                alive: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pos[q] of the module docstring (msim_mine_bounds): fp32 [n_q], the maximum of scores[q, c] over the in-shard positives of q
    (`csr`: what `positives_csr` returns; with `alive`, uint8 [>= n], those of live slots only), +inf where there is none -- or
    -inf with `local=True`, which is what one shard of several contributes to the all-reduce MAX (`ShardedRetriever.mine`).
    Asynchronous on torch's current stream, hipGraph-capturable."""
    ld = _scores_ld(scores, "mine_bounds")
    n_q, n = scores.shape
    ids, offsets = _check_csr(csr, n_q, scores.device, "mine_bounds")
    _check_alive(alive, n, scores.device)
    bounds = torch.empty((n_q,), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        rc = _lib.lib().msim_mine_bounds(_lib.ptr(scores), ld, n_q, n, _lib.ptr(ids), _lib.ptr(offsets), ids.numel(), int(id_base),
                                         _lib.ptr(alive), 1 if local else 0, _lib.ptr(bounds), _lib.current_stream_handle(scores.device))
    _lib.check(rc, "msim_mine_bounds")
    return bounds


def mine_mask(scores: torch.Tensor, csr, id_base: int = 0, bounds: Optional[torch.Tensor] = None, max_ratio: Optional[float] = None,
              alive: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-inf, in place, into every INELIGIBLE column of `scores` (fp32 [n_q, n] on the GPU; msim_mine_mask): the positives of `csr`,
    the slots with alive[c] == 0 (uint8 [>= n]) and, when `max_ratio` is given, the columns with scores[q, c] > max_ratio * bounds[q]
    (`bounds`: `mine_bounds` of the same matrix BEFORE the mask, or its all-reduced maximum).  Nothing else is touched.
    Asynchronous on torch's current stream, hipGraph-capturable."""
    ld = _scores_ld(scores, "mine_mask")
    n_q, n = scores.shape
    dev = scores.device
    ids, offsets = _check_csr(csr, n_q, dev, "mine_mask")
    if max_ratio is None:
        bounds = None
    elif (bounds is None or bounds.dtype != torch.float32 or bounds.shape != (n_q,) or bounds.device != dev or not bounds.is_contiguous()):
        raise ValueError(f"mine_mask: max_ratio needs bounds, a contiguous fp32 [n_q = {n_q}] tensor on {dev}")
    _check_alive(alive, n, dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_mine_mask(_lib.ptr(scores), ld, n_q, n, _lib.ptr(bounds), float(max_ratio or 0.0), _lib.ptr(alive),
                                       _lib.ptr(ids), _lib.ptr(offsets), ids.numel(), int(id_base), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_mine_mask")
    return scores


def check_mine_args(n_neg: int, skip_top: int, max_ratio: Optional[float]) -> Tuple[int, int, Optional[float]]:
    n_neg, skip_top = int(n_neg), int(skip_top)
    if n_neg < 1:
        raise ValueError(f"n_neg={n_neg}: at least one negative per query")
    if skip_top < 0:
        raise ValueError(f"skip_top={skip_top} is negative")
    if max_ratio is not None:
        max_ratio = float(max_ratio)
        if not (max_ratio > 0.0 and math.isfinite(max_ratio)):
            raise ValueError(f"max_ratio={max_ratio}: a finite ratio above 0 (the reference's filter_threshold is 0.95)")
    return n_neg, skip_top, max_ratio


def select_window(masked: torch.Tensor, id_base: int, n_neg: int, skip_top: int, shard_select: Callable):
    """Ranks skip_top .. skip_top + n_neg - 1 of every masked row: `shard_select(masked, k, id_base)` -> the (score desc, id asc)
    top k = skip_top + n_neg, cut AFTER the selection (and after the merge of several shards); an entry of score -inf is no page."""
    top_s, top_i = shard_select(masked, skip_top + n_neg, id_base)
    top_s, top_i = top_s[:, skip_top:], top_i[:, skip_top:]
    top_i = torch.where(top_s == float("-inf"), torch.full_like(top_i, -1), top_i)     # an ineligible column that filled a short row
    return top_s.contiguous(), top_i


def mine_masked(scores: torch.Tensor, positives: Positives, id_base: int, max_ratio: Optional[float], alive: Optional[torch.Tensor],
                bounds_fn: Callable, mask_fn: Callable, reduce_max: Optional[Callable] = None) -> torch.Tensor:
    """`scores` with every ineligible column at -inf (in place): bounds -> (all-reduce MAX over the shards) -> mask.  The hooks are
    `mine_bounds` / `mine_mask` or stand-ins with their signatures (host-logic tests); `reduce_max(t)` all-reduces fp32 [n_q] in
    place.  With several shards a query none of whose positives scored above -inf anywhere is bounded as one without positives."""
    csr = positives_csr(positives, scores.shape[0], scores.device)
    bounds = None
    if max_ratio is not None:
        bounds = bounds_fn(scores, csr, id_base, local=reduce_max is not None, alive=alive)
        if reduce_max is not None:
            reduce_max(bounds)
            bounds = torch.where(bounds == float("-inf"), torch.full_like(bounds, float("inf")), bounds)    # no rank holds a positive
    return mask_fn(scores, csr, id_base, bounds, max_ratio, alive)


def mine_hard_negatives(queries, corpus: PackedCorpus, positives: Positives, n_neg: int, *, max_ratio: Optional[float] = None,
                        skip_top: int = 0, alive: Optional[torch.Tensor] = None,
                        scores: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The `n_neg` hardest negatives of every query over the resident corpus, by the model's own MaxSim score:
    (neg_scores fp32 [n_q, n_neg], neg_ids int64 [n_q, n_neg]), GLOBAL ids, (score descending, id ascending); the rule is the
    module docstring's.  `gather_pages(corpus, neg_ids)` is the `neg_doc_embeddings` of the explicit-negative losses.

    queries: anything `maxsim_scores` takes (a `PackedQueries` or a contiguous [n_q, Lq, width] device tensor); corpus: a GPU
    `PackedCorpus` of any dtype and width the full scan takes (RuntimeError for a CPU corpus: the kernels are gfx950 only), or a
    `ResidualCorpus` or a `ResidualWideCorpus`: the scan is then `residual_scores` / `residual_wide_scores` over its compressed rows
    (its query forms and formats).
    positives: GLOBAL ids (`corpus.id_base + column`) as an int64 [n_q] tensor (-1 = none), an int64 [n_q, P] tensor padded with
    -1, or a CSR pair (ids int64 [nnz], offsets int32 [n_q + 1]); an id outside the shard is ignored on the device -- no error, no
    synchronisation; duplicates are allowed.  ValueError for another dtype or shape.
    max_ratio: drop the pages that score above `max_ratio x (the best positive's score)` -- likely false negatives; the reference's
    0.95 rule, sign quirk included (module docstring); a finite value above 0.  skip_top: leave out the `skip_top` best eligible pages.
    alive: uint8 [>= n] on the corpus' device, 0 = never mine this slot (`LiveCorpus.mine` passes its tombstones).
    scores: the fp32 [n_q, n] matrix of `maxsim_scores(queries, corpus)` if the caller has it already (it is copied, not modified);
    the scan is then skipped and `queries` may be None.  neg_scores carries the scan's bits.
    Asynchronous on torch's current stream; given a `PackedQueries` (or `scores=`) and device positives there is no host
    synchronisation and the call is hipGraph-capturable (no allocation inside the library calls)."""
    from .retrieval import topk              # retrieval imports this module

    dev = _require_gpu(corpus.device)
    n_neg, skip_top, max_ratio = check_mine_args(n_neg, skip_top, max_ratio)
    n = len(corpus)
    if scores is None:
        from .residual import ResidualCorpus, residual_scores
        from .residual_wide import ResidualWideCorpus, residual_wide_scores

        s = (residual_scores(queries, corpus) if isinstance(corpus, ResidualCorpus)
             else residual_wide_scores(queries, corpus) if isinstance(corpus, ResidualWideCorpus) else maxsim_scores(queries, corpus))
    else:
        if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[1] != n:
            raise ValueError(f"scores must be the fp32 [n_q, n = {n}] matrix of maxsim_scores(queries, corpus)")
        if scores.device != dev:
            raise ValueError("scores and corpus live on different devices")
        s = scores.clone(memory_format=torch.contiguous_format)
    if alive is not None and alive.device != dev:
        raise ValueError("alive and corpus live on different devices")
    masked = mine_masked(s, positives, int(corpus.id_base), max_ratio, alive, mine_bounds, mine_mask)
    return select_window(masked, int(corpus.id_base), n_neg, skip_top, topk)


def gather_pages(corpus: PackedCorpus, ids: torch.Tensor, pad_to: Optional[int] = None,
                 out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The listed pages as one zero-padded box (msim_gather_pages): (box [*ids.shape, L_pad, width] of the corpus' dtype,
    lengths int32 [*ids.shape]).  `gather_pages(corpus, neg_ids)` is the `neg_doc_embeddings [B, n_neg, L_neg, dim]` of
    `ColbertNegativeCELoss` / `ColbertPairwiseNegativeCELoss`.

    ids: int64 GLOBAL ids of any shape.  L_pad = `pad_to`, or the corpus' longest page (host metadata: no synchronisation).
    Rows past a page's length, and the whole page for id -1 or an id outside the shard, are exactly zero -- what the reference's
    padded positions hold -- and `lengths` is 0 for such a slot.
    A page longer than `pad_to`: with `ids` on the HOST the listed pages are checked against `corpus.lengths` and ValueError is
    raised; with `ids` on the device nothing is read back: the page is TRUNCATED to its first `pad_to` rows and `lengths` reports
    the truncated count.
    out: a contiguous [*ids.shape, L_pad, width] tensor to write into (every byte of it is written).
    Asynchronous on torch's current stream; with device ids there is no host synchronisation and the call is hipGraph-capturable.
    A `ResidualCorpus` goes to `residual_gather_pages`, a `ResidualWideCorpus` (width 320) to `residual_wide_gather_pages`: the bytes
    of this call over `corpus.decompress()`, decoded into the box."""
    from .residual import ResidualCorpus, residual_gather_pages
    from .residual_wide import ResidualWideCorpus, residual_wide_gather_pages

    if isinstance(corpus, ResidualCorpus):
        return residual_gather_pages(corpus, ids, pad_to, out)
    if isinstance(corpus, ResidualWideCorpus):
        return residual_wide_gather_pages(corpus, ids, pad_to, out)
    dev = _require_gpu(corpus.device)
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
        raise ValueError("ids must be an int64 tensor")
    n = len(corpus)
    if pad_to is None:
        pad_to = int(corpus.lengths.max()) if n else 0
    pad_to = int(pad_to)
    if pad_to < 0:
        raise ValueError(f"pad_to={pad_to} is negative")
    if ids.device.type == "cpu":
        idx = ids.reshape(-1).numpy() - int(corpus.id_base)
        inside = idx[(ids.reshape(-1).numpy() >= 0) & (idx >= 0) & (idx < n)]
        lens = corpus.lengths.numpy()[inside]
        if lens.size and int(lens.max()) > pad_to:
            bad = int(inside[int(np.argmax(lens))]) + int(corpus.id_base)
            raise ValueError(f"page {bad} has {int(lens.max())} rows, pad_to={pad_to}")
        ids = ids.to(dev)
    elif ids.device != dev:
        raise ValueError("ids and corpus live on different devices")
    flat = ids.reshape(-1).contiguous()
    width = int(corpus.blob.shape[1])
    shape = tuple(ids.shape) + (pad_to, width)
    if out is None:
        out = torch.empty(shape, dtype=corpus.blob.dtype, device=dev)
    elif out.shape != shape or out.dtype != corpus.blob.dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {corpus.blob.dtype} tensor of shape {shape} on {dev}")
    lengths = torch.empty(tuple(ids.shape), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().msim_gather_pages(_lib.ptr(corpus.blob), width * corpus.blob.element_size(), int(corpus.blob.shape[0]),
                                          _lib.ptr(corpus.offsets), n, int(corpus.id_base), _lib.ptr(flat), flat.numel(), pad_to,
                                          _lib.ptr(out), _lib.ptr(lengths), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_gather_pages")
    return out, lengths
