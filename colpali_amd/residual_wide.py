"""The residual-compressed shard at width 320 (ColQwen3): the centroid-code first stage and PLAID's second half over 640-byte rows.

`CentroidWideIndex` is to `CentroidIndex`, and `ResidualWideCorpus` to `ResidualCorpus`, what `Fp4WideIndex` is to `Fp4Index`: the
same contracts with 128 replaced by 320, on kernels of their own (include/maxsim.h: msim_cent_wide_*, msim_res_wide_*;
colpali_amd/csrc/residual_wide.hip).  A row costs 2 bytes of centroid code plus 40 * bits bytes of residual -- 82 bytes at 2 bits,
162 at 4, instead of 640 -- and no full-precision row is kept.

    encode   code[r] = argmax_k <row_r, C_k> (one fp32 MFMA chain over the ten 32-wide k-steps; the lowest k wins equal values)
             e_k = fl32(float(x_k) - float(C[c]_k));  bucket b_k = #{cutoffs t : t <= e_k}
    pack     dimension k = bits [k * bits, k * bits + bits) of the row's 40 * bits bytes, a little-endian bit string
    decode   xhat_k = round_to_dtype(float(C[c]_k) + weights[b_k])   -- one rounding, NO renormalisation

`centroid_wide_scores` is the wide query table followed by the scan of `centroid_scores` (the scan reads the table and the codes
alone, so it is the same kernel for both widths).  `residual_wide_rerank_scores` reranks candidate lists straight from the
compressed rows: every score has the bits `rerank_scores` gives the same query against `rc.decompress()`.  Stage 1 is `rc.index`:
`ShardedRetriever(rc).search(q, k, prefilter=rc.index, n_candidates=m)`; `refine=<Fp4WideIndex>` (built from the corpus before it
is freed) puts the FP4 rows between the two.  `residual_wide_scores` is the full scan of such a shard (include/maxsim.h:
msim_res_wide_scores; colpali_amd/csrc/residual_wide_scan.hip): a page is decoded once per group of up to 8 queries, never written
to memory, and entry (q, c) has the rerank's bits.  The default retriever only scans on request:
`ShardedRetriever(rc, score_fn=residual_wide_scores)` opens the full scan, `filter=`, `group_by=` and `mine`, as
`score_fn=residual_scores` does at width 128; `mine_hard_negatives(q, rc, ...)` dispatches to it.

`residual_wide_align` and `residual_wide_gather_pages` are `align` and `gather_pages` over such a shard, the listed pages decoded
inside the kernel that consumes them (include/maxsim.h: msim_res_wide_align_candidates, msim_res_wide_gather_pages;
colpali_amd/csrc/residual_wide_align.hip): the bits of the same call over `rc.decompress()`, no decoded copy in memory, no host read
of the list.  `align(queries, rc, ids)` and `gather_pages(rc, ids)` dispatch to them;
`ShardedRetriever(rc, align_fn=residual_wide_align)` opens the retriever's `align`.

The host layer is the one of widths 128 (colpali_amd/centroid.py: `_CentroidCodes`, colpali_amd/residual.py: `_ResidualRows`); the
classes here bind the width and the wide entries.  They are siblings of the 128 classes, not subclasses: the 128 scan
(`residual_scores`), the 128 `residual_align` / `residual_gather_pages` and what exists at width 128 only -- `LiveResidualCorpus` --
refuse them by their type, as `residual_wide_scores`, `residual_wide_align` and `residual_wide_gather_pages` refuse a
`ResidualCorpus`, and no kernel of one width ever sees a row of the other.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .centroid import _CentroidCodes, _require_kind, _scores
from .residual import WIDE_DIM as DIM
from .residual import _align_rows, _gather_rows, _rerank_scores, _ResidualRows, _scan_scores


class CentroidWideIndex(_CentroidCodes):
    """The centroid-code copy of one resident 320-wide shard: `centroids` [K, 320] (bf16 / f16, K a multiple of 256 in 256 .. 2048),
    `codes` uint16 [rows] in the corpus's row order, the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n] or
    None), copied; `lengths` (int64 [n], host) and `id_base` as the corpus's.  `build(corpus, centroids=None, n_centroids=1024,
    iters=8, sample_rows=2^18, seed=0, chunk_docs=65536)` trains by spherical k-means with the wide encode kernel when no centroids
    are given; `nbytes`, `save` and `load` as `CentroidIndex`.  With world > 1 every rank must build its index from the SAME
    centroids, as for a `CentroidIndex`: stage-1 scores of different centroid sets do not compare."""

    WIDTH = DIM
    _ENCODE = "msim_cent_wide_encode_docs"
    _TABLE = "msim_cent_wide_table"


class ResidualWideCorpus(_ResidualRows):
    """One resident 320-wide shard in compressed form: `centroids` [K, 320] (bf16 / f16), `codes` uint16 [rows], `residuals` uint8
    [rows, 40 * bits], `cutoffs` fp32 [2^bits - 1], `weights` fp32 [2^bits], the pages' `offsets` (int32 [n + 1], device), `clamp0`
    (uint8 [n] or None), `lengths` (int64 [n], host), `id_base` and `bits`.  `.index` is a `CentroidWideIndex` over the SAME `codes`
    and `centroids` tensors (no copy): the stage 1 that goes with this stage 2.  `build`, `decompress`, `save` and `load` as
    `ResidualCorpus`; `width` is 320."""

    WIDTH = DIM
    _INDEX = CentroidWideIndex
    _ENCODE = "msim_res_wide_encode_docs"
    _DECODE = "msim_res_wide_decode_rows"
    _CANDIDATES = "msim_res_wide_candidates"
    _SCORES = "msim_res_wide_scores"
    _ALIGN = "msim_res_wide_align_candidates"
    _GATHER = "msim_res_wide_gather_pages"


def centroid_wide_scores(queries, index: CentroidWideIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Centroid-interaction scores of every 320-wide query against every page of the index (msim_cent_wide_table, then
    msim_cent_scores): fp32 [n_q, len(index)], column j = page index.id_base + j, with the forms, checks and guarantees of
    `centroid_scores` -- bf16 / f16, queries of up to 128 tokens; given a `PackedQueries` no host synchronisation, hipGraph-capturable."""
    if not isinstance(index, _CentroidCodes):
        raise ValueError("index must be a CentroidWideIndex")
    _require_kind(index, CentroidWideIndex, "centroid_wide_scores")
    return _scores(queries, index, out)


def residual_wide_rerank_scores(queries, rc: ResidualWideCorpus, candidates: torch.Tensor, *,
                                out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaxSim of listed candidates against the compressed 320-wide pages (include/maxsim.h: msim_res_wide_candidates): (scores fp32
    [n_q, m], ids int64 [n_q, m]) with the signature, the query forms and the checks of `rerank_scores`.  Entry (q, j) has the bits
    `rerank_scores(queries, rc.decompress(), candidates)` gives; an id of -1 or outside [id_base, id_base + len(rc)) comes back as
    (-inf, -1).  bfloat16 / float16, width 320, queries of at most 128 tokens (NotImplementedError otherwise).  Given a
    `PackedQueries` it never synchronises with the host and is hipGraph-capturable."""
    return _rerank_scores(queries, rc, candidates, out, ResidualWideCorpus)


def residual_wide_scores(queries, rc: ResidualWideCorpus, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxSim of every query against every page of the compressed 320-wide shard (include/maxsim.h: msim_res_wide_scores): fp32
    [n_q, len(rc)], `residual_scores` at width 320 and the counterpart of `maxsim_scores` over a `PackedCorpus`.  Entry (q, c) has the
    bits `residual_wide_rerank_scores` gives the query against page c, which are the bits of `maxsim_scores(queries, rc.decompress())`
    whenever that scan runs the flat kernel every ragged batch runs; a scan of ONE query length and at most four 32-token tiles runs
    another kernel, whose token sum is a butterfly, and agrees to the bound include/maxsim.h states, not bit for bit.  Every row of the
    shard is decoded, once per group of up to 8 queries (128 tokens), and never written to memory.  The query forms and checks of
    `residual_wide_rerank_scores`: a `PackedQueries`, a host list or a dense device box; RuntimeError on a dtype mismatch;
    NotImplementedError for fp32, a width other than 320, a query over 128 tokens or a `ResidualCorpus` (width 128:
    `residual_scores`).  `out`: fp32 [n_q, n] with unit inner stride on the corpus' device -- it may be a column slice of a wider
    matrix, whose other columns are not touched.  Given a `PackedQueries` it never synchronises with the host and is
    hipGraph-capturable."""
    return _scan_scores(queries, rc, out, ResidualWideCorpus)


def residual_wide_align(queries, rc: ResidualWideCorpus, ids: torch.Tensor, *, maps: bool = False, max_rows: Optional[int] = None):
    """`align` over the compressed 320-wide shard (include/maxsim.h: msim_res_wide_align_candidates): `residual_align` at width 320.
    The `Alignment` of every entry (q, j) of `ids` (int64 [n_q, m] GLOBAL ids on the shard's device, -1 = none), with the signature,
    the query forms and the checks of `align`.  best_sim, best_row, ids and sims have the bits
    `align(queries, rc.decompress(), ids, maps=, max_rows=)` gives: every listed page is decoded chunk by chunk in the registers of
    the kernel that multiplies it, and no decoded row is written to memory.  bfloat16 / float16, width 320, queries of at most 128
    tokens (NotImplementedError otherwise, and for a `ResidualCorpus` -- width 128: `residual_align`; RuntimeError when queries and
    shard differ in dtype; ValueError for ids of the wrong shape, dtype or device).  `max_rows` bounds the rows of a listed page
    (default: the shard's longest page, known on the host); a longer page comes back NaN / -1.  Asynchronous on torch's current
    stream; with a `PackedQueries` there is no host synchronisation and the call is hipGraph-capturable.  What can be refused
    without the device is refused before it is asked for: the formats and `max_rows` always, the token count and `ids` for queries
    that come packed."""
    return _align_rows(queries, rc, ids, maps, max_rows, ResidualWideCorpus, "residual_wide_align")


def residual_wide_gather_pages(rc: ResidualWideCorpus, ids: torch.Tensor, pad_to: Optional[int] = None,
                               out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`gather_pages` over the compressed 320-wide shard (include/maxsim.h: msim_res_wide_gather_pages): `residual_gather_pages` at
    width 320.  (box [*ids.shape, L_pad, 320] of the shard's dtype, lengths int32 [*ids.shape]) with the bytes
    `gather_pages(rc.decompress(), ids, pad_to)` gives -- the listed pages are decoded straight into the box, so
    `mine_hard_negatives(q, rc, ...)` -> `gather_pages(rc, neg_ids)` feeds the explicit-negative losses without a decoded shard.
    ids: int64 GLOBAL ids of any shape; L_pad = `pad_to`, or the shard's longest page.  Rows past a page's length, and the whole
    page for id -1 or an id outside the shard, are exactly zero and `lengths` is 0 for such a slot.  A page longer than `pad_to`:
    host ids raise ValueError, device ids TRUNCATE (`lengths` reports the truncated count), as `gather_pages`.  out: a contiguous
    [*ids.shape, L_pad, 320] tensor to write into (every byte of it is written).  NotImplementedError for a `ResidualCorpus` (width
    128: `residual_gather_pages`).  Asynchronous on torch's current stream; with device ids there is no host synchronisation and the
    call is hipGraph-capturable."""
    return _gather_rows(rc, ids, pad_to, out, ResidualWideCorpus, "residual_wide_gather_pages")
