"""An FP4 index: a token-level first stage for two-stage search at 65 bytes per corpus row, half of the int8 index.

`Fp4Index.build` keeps every row of a resident `PackedCorpus` as 128 OCP e2m1 values (two per byte) and one power-of-two scale
byte.  `fp4_scores` codes the query tokens the same way and scores every page by MaxSim on the block-scaled MFMA
(include/maxsim.h: msim_f4_*, colpali_amd/csrc/fp4_index.hip): one instruction per 16 rows x 16 tokens over all 128 dimensions;
every per-token maximum is exactly representable in fp32, so a score's bits are fixed.  Its top `n_candidates` are reranked
exactly -- `ShardedRetriever.search(prefilter=index, n_candidates=m)` -- so every returned score is the exact one.  The index
carries no trained parameter: stage-1 scores of different shards are comparable.

`fp6_scores` scores the same index with the query tokens coded as OCP e2m3 (FP6: 96 code bytes and a scale byte per token,
msim_f6_encode_rows / msim_f4_scores_q6).  The pages stay FP4 and the index is untouched; the instruction takes a format per
operand and FP6 runs at the FP4 rate, so the first stage loses the query side's quantisation error for nothing stored.  It is the
function to hand to a retriever: `ShardedRetriever(shard, fp4_score_fn=fp6_scores)`.

`fp4_rerank_scores` / `fp6_rerank_scores` are the LIST form of the two (msim_f4_candidates / msim_f4_candidates_q6,
colpali_amd/csrc/fp4_candidates.hip): the FP4 score of the pages a candidate list names and of no other, bit for bit what the scan
gives for the same query and page.  It is the middle stage of a three-stage search -- a cheap stage 1 makes a long list, the FP4
rows cut it, the exact rerank orders the survivors: `ShardedRetriever.search(prefilter=fde, n_candidates=m1, refine=index,
n_refine=m2)`.
"""
from __future__ import annotations

from functools import partial
from typing import Optional, Tuple

import torch

from . import _fp4_family as _family
from ._fp4_family import MAX_RERANK_TOKENS         # the longest query of the list form (eight 16-token tiles in registers)

FAMILY = _family.NARROW
DIM = FAMILY.dim
ROW_BYTES = DIM // 2
Q6_ROW_BYTES = DIM * 6 // 8                       # an e2m3 query token: 128 6-bit fields
QUERY_CODES = FAMILY.query_codes                  # query_code -> code bytes per token

_check_format = partial(_family.check_format, FAMILY)   # (dtype, width, what, query_code="e2m1")


class Fp4Index(_family.Index):
    """The FP4 rows of one resident shard: `codes` uint8 [rows, 64] in the corpus's row order (dimension k is nibble k & 1 of byte
    k >> 1, the low nibble the even k; a nibble is sign << 3 | e2m1 code), `scales` uint8 [rows] (E8M0: the row's values are the
    decoded codes times 2^(scale - 127)), the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n] or None),
    copied; `lengths` (int64 [n], host) and `id_base` as the corpus's."""
    family = FAMILY


def fp4_quantize_queries(queries, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token codes uint8 [T, 64] and scales uint8 [T] of `queries` (a `PackedQueries`, a host list of [len_i, 128] tensors or a
    [n_q, Lq, 128] tensor, packed into the flat layout first), in the packed token order: the page rows' code."""
    return _family.quantize_queries(FAMILY, queries, device, "e2m1")


def fp6_quantize_queries(queries, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token e2m3 codes uint8 [T, 96] and scales uint8 [T] of `queries` (as `fp4_quantize_queries` takes them), in the packed
    token order: dimension k is the 6-bit field (sign << 5 | code) at bit 6 (k mod 32) of the little-endian 24-byte group k // 32."""
    return _family.quantize_queries(FAMILY, queries, device, "e2m3")


def fp4_scores_from_codes(q_codes: torch.Tensor, q_scales: torch.Tensor, q_offsets: torch.Tensor, max_q_tokens: int,
                          index: Fp4Index, out: Optional[torch.Tensor] = None, *, query_code: str = "e2m1") -> torch.Tensor:
    """fp32 [n_q, len(index)] (msim_f4_scores) from coded queries (`fp4_quantize_queries`): codes uint8 [T, 64], scales uint8 [T],
    offsets int32 [n_q + 1] on the device and a host bound on every query's token count.  `query_code="e2m3"`: codes uint8 [T, 96]
    from `fp6_quantize_queries` (msim_f4_scores_q6)."""
    return _family.scores_from_codes(FAMILY, q_codes, q_scales, q_offsets, max_q_tokens, index, out, query_code)


def fp4_scores(queries, index: Fp4Index, out: Optional[torch.Tensor] = None, *, query_code: str = "e2m1") -> torch.Tensor:
    """Approximate MaxSim of every query against every page of the index: fp32 [n_q, len(index)], column j = page
    index.id_base + j.  A score's bits depend on its query and page only.  Asynchronous on torch's current stream.  Given a
    `PackedQueries` it never synchronises with the host and is hipGraph-capturable: its only allocations are torch tensors (the
    query codes and scales, and `out` when it is None), made on the current stream before the library calls.  `query_code`: how the
    query tokens are coded, "e2m1" (as the pages) or "e2m3" (`fp6_scores`)."""
    return _family.scores(FAMILY, queries, index, out, query_code)


def fp6_scores(queries, index: Fp4Index, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`fp4_scores` with the query tokens coded as e2m3 (FP6) against the same FP4 pages: a better first stage from the same index,
    bit for bit reproducible in the same way.  The stage-1 hook of a retriever: `ShardedRetriever(shard, fp4_score_fn=fp6_scores)`."""
    return fp4_scores(queries, index, out, query_code="e2m3")


def fp4_rerank_scores(queries, index: Fp4Index, candidates: torch.Tensor, *, query_code: str = "e2m1",
                      out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The FP4 score of listed candidates (include/maxsim.h: msim_f4_candidates, msim_f4_candidates_q6): (scores fp32 [n_q, m], ids
    int64 [n_q, m]).

    Entry (q, j) is scored against page candidates[q, j] (a GLOBAL id, int64 [n_q, m] on the index's device) of `index`; its bits
    are those of `fp4_scores(queries, index, query_code=query_code)[q, candidates[q, j] - index.id_base]`, whatever else the list
    holds.  An id of -1 or outside [id_base, id_base + len(index)) comes back as (-inf, -1) and reads nothing; a page of 0 rows
    scores -inf; an id listed twice is scored twice.  Only the listed pages are read: 65 bytes per row.  Lists are taken as
    `rerank_scores` takes them (a broadcast row is copied).  Queries are packed and coded as `fp4_scores` does; more than 128
    tokens in a query, or an index that is not an `Fp4Index`, raises NotImplementedError.  `out`: the fp32 [n_q, m] score tensor.
    Asynchronous on torch's current stream; given a `PackedQueries` it never synchronises with the host, never reads the list on
    the host, and is hipGraph-capturable (its allocations are torch tensors made before the library call; the list may be
    rewritten in place between replays).  It is the `fp4_rerank_fn` hook of `ShardedRetriever` (`search(refine=)`)."""
    return _family.rerank_scores(FAMILY, queries, index, candidates, query_code, out)


def fp6_rerank_scores(queries, index: Fp4Index, candidates: torch.Tensor, *, out: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`fp4_rerank_scores` with the query tokens coded as e2m3 (FP6): the bits of `fp6_scores` at the listed pages.  The refine hook
    to hand to a retriever beside `fp4_score_fn=fp6_scores`: `ShardedRetriever(shard, fp4_rerank_fn=fp6_rerank_scores)`."""
    return fp4_rerank_scores(queries, index, candidates, query_code="e2m3", out=out)
