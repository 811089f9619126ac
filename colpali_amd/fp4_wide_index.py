"""An FP4 index for 320-wide (ColQwen3) shards: a token-level first stage for two-stage search at 161 bytes per corpus row
instead of 640.

`Fp4WideIndex.build` keeps every row of a resident 320-wide `PackedCorpus` as 320 OCP e2m1 values (two per byte) and ONE
power-of-two scale byte.  `fp4_wide_scores` codes the query tokens the same way and scores every page by MaxSim on the
block-scaled MFMA (include/maxsim.h: msim_f4w_*, colpali_amd/csrc/fp4_wide_index.hip): a 320-wide row is 2 1/2 of the
instruction's 128-wide K blocks, so one 16 rows x 16 tokens product is three instructions chained through the accumulator; with
one scale per row every partial sum is exactly representable in fp32, so a score's bits are fixed.  Its top `n_candidates` are
reranked exactly -- `ShardedRetriever.search(prefilter=index, n_candidates=m)` -- so every returned score is the exact one.  The
index carries no trained parameter: stage-1 scores of different shards are comparable.

`fp4_wide_rerank_scores` is the LIST form (msim_f4w_candidates, colpali_amd/csrc/fp4_wide_candidates.hip): the FP4 score of the
pages a candidate list names and of no other, bit for bit what the scan gives for the same query and page.  It is the middle stage
of a three-stage search on a 320-wide shard -- a cheap stage 1 makes a long list, the 161-byte FP4 rows cut it, the exact rerank
orders the survivors: `ShardedRetriever.search(prefilter=pooled, n_candidates=m1, refine=index, n_refine=m2)`.

`fp6_wide_scores` / `fp6_wide_rerank_scores` score the same index with the query tokens coded as OCP e2m3 (FP6: 240 code bytes
and a scale byte per token, msim_f6w_encode_rows / msim_f4w_scores_q6 / msim_f4w_candidates_q6).  The pages stay FP4 and the index
is untouched: the instruction takes a format per operand, so the first stage loses most of the query side's quantisation error for
nothing stored.  They are the functions to hand to a retriever:
`ShardedRetriever(shard, fp4_wide_score_fn=fp6_wide_scores, fp4_wide_rerank_fn=fp6_wide_rerank_scores)`.

It is the sibling of `Fp4Index` (width 128), which keeps refusing width 320 as this class refuses width 128.
"""
from __future__ import annotations

from functools import partial
from typing import Optional, Tuple

import torch

from . import _fp4_family as _family
from ._fp4_family import MAX_RERANK_TOKENS         # the longest query of the list form (eight 16-token tiles in registers)

FAMILY = _family.WIDE
DIM = FAMILY.dim
ROW_BYTES = DIM // 2
Q6_ROW_BYTES = DIM * 6 // 8                       # an e2m3 query token: 320 6-bit fields
QUERY_CODES = FAMILY.query_codes                  # query_code -> code bytes per token

_check_format = partial(_family.check_format, FAMILY)   # (dtype, width, what, query_code="e2m1")


class Fp4WideIndex(_family.Index):
    """The FP4 rows of one resident 320-wide shard: `codes` uint8 [rows, 160] in the corpus's row order (dimension k is nibble
    k & 1 of byte k >> 1, the low nibble the even k; a nibble is sign << 3 | e2m1 code), `scales` uint8 [rows] (E8M0: the row's
    values are the decoded codes times 2^(scale - 127)), the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n]
    or None), copied; `lengths` (int64 [n], host) and `id_base` as the corpus's."""
    family = FAMILY


def fp4_wide_quantize_queries(queries, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token codes uint8 [T, 160] and scales uint8 [T] of `queries` (a `PackedQueries`, a host list of [len_i, 320] tensors or
    a [n_q, Lq, 320] tensor, packed into the flat layout first), in the packed token order: the page rows' code."""
    return _family.quantize_queries(FAMILY, queries, device, "e2m1")


def fp6_wide_quantize_queries(queries, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token e2m3 codes uint8 [T, 240] and scales uint8 [T] of `queries` (as `fp4_wide_quantize_queries` takes them), in the
    packed token order: dimension k is the 6-bit field (sign << 5 | code) at bit 6 k of the little-endian 240-byte row."""
    return _family.quantize_queries(FAMILY, queries, device, "e2m3")


def fp4_wide_scores_from_codes(q_codes: torch.Tensor, q_scales: torch.Tensor, q_offsets: torch.Tensor, max_q_tokens: int,
                               index: Fp4WideIndex, out: Optional[torch.Tensor] = None, *, query_code: str = "e2m1") -> torch.Tensor:
    """fp32 [n_q, len(index)] (msim_f4w_scores) from coded queries (`fp4_wide_quantize_queries`): codes uint8 [T, 160], scales
    uint8 [T], offsets int32 [n_q + 1] on the device and a host bound on every query's token count.  `query_code="e2m3"`: codes
    uint8 [T, 240] from `fp6_wide_quantize_queries` (msim_f4w_scores_q6)."""
    return _family.scores_from_codes(FAMILY, q_codes, q_scales, q_offsets, max_q_tokens, index, out, query_code)


def fp4_wide_scores(queries, index: Fp4WideIndex, out: Optional[torch.Tensor] = None, *, query_code: str = "e2m1") -> torch.Tensor:
    """Approximate MaxSim of every query against every page of the index: fp32 [n_q, len(index)], column j = page
    index.id_base + j.  A score's bits depend on its query and page only.  Asynchronous on torch's current stream.  Given a
    `PackedQueries` it never synchronises with the host and is hipGraph-capturable: its only allocations are torch tensors (the
    query codes and scales, and `out` when it is None), made on the current stream before the library calls.  `query_code`: how the
    query tokens are coded, "e2m1" (as the pages) or "e2m3" (`fp6_wide_scores`)."""
    return _family.scores(FAMILY, queries, index, out, query_code)


def fp6_wide_scores(queries, index: Fp4WideIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`fp4_wide_scores` with the query tokens coded as e2m3 (FP6) against the same FP4 pages: a first stage with less query-side
    quantisation error from the same index, bit for bit reproducible in the same way.  The stage-1 hook of a retriever on a
    320-wide shard: `ShardedRetriever(shard, fp4_wide_score_fn=fp6_wide_scores)`.  A 128-wide shard takes `fp6_scores`."""
    return fp4_wide_scores(queries, index, out, query_code="e2m3")


def fp4_wide_rerank_scores(queries, index: Fp4WideIndex, candidates: torch.Tensor, *, query_code: str = "e2m1",
                           out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The FP4 score of listed candidates at width 320 (include/maxsim.h: msim_f4w_candidates, msim_f4w_candidates_q6): (scores
    fp32 [n_q, m], ids int64 [n_q, m]).

    Entry (q, j) is scored against page candidates[q, j] (a GLOBAL id, int64 [n_q, m] on the index's device) of `index`; its bits
    are those of `fp4_wide_scores(queries, index, query_code=query_code)[q, candidates[q, j] - index.id_base]`, whatever else the
    list holds.  An id of -1 or outside [id_base, id_base + len(index)) comes back as (-inf, -1) and reads nothing; a page of 0
    rows scores -inf; an id listed twice is scored twice.  Only the listed pages are read: 161 bytes per row.  Lists are taken as
    `rerank_scores` takes them (a broadcast row is copied).  Queries are packed and coded as `fp4_wide_scores` does; more than 128
    tokens in a query, or an index that is not an `Fp4WideIndex` (an `Fp4Index` of a 128-wide shard goes to `fp4_rerank_scores` /
    `fp6_rerank_scores`), raises NotImplementedError.  `out`: the fp32 [n_q, m] score tensor.  Asynchronous on torch's current
    stream; given a `PackedQueries` it never synchronises with the host, never reads the list on the host, and is
    hipGraph-capturable (its allocations are torch tensors made before the library call; the list may be rewritten in place between
    replays).  It is the `fp4_wide_rerank_fn` hook of `ShardedRetriever` (`search(refine=)`)."""
    return _family.rerank_scores(FAMILY, queries, index, candidates, query_code, out)


def fp6_wide_rerank_scores(queries, index: Fp4WideIndex, candidates: torch.Tensor, *, out: Optional[torch.Tensor] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`fp4_wide_rerank_scores` with the query tokens coded as e2m3 (FP6): the bits of `fp6_wide_scores` at the listed pages.  The
    refine hook to hand to a retriever beside `fp4_wide_score_fn=fp6_wide_scores`:
    `ShardedRetriever(shard, fp4_wide_rerank_fn=fp6_wide_rerank_scores)`.  An `Fp4Index` of a 128-wide shard takes
    `fp6_rerank_scores`."""
    return fp4_wide_rerank_scores(queries, index, candidates, query_code="e2m3", out=out)
