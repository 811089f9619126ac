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

from typing import Optional, Tuple

import torch

from . import _lib
from .corpus import PackedCorpus, PackedQueries, _as_packed, _rerank_args
from .scoring import _require_gpu

DIM = 320
ROW_BYTES = DIM // 2
Q6_ROW_BYTES = DIM * 6 // 8                       # an e2m3 query token: 320 6-bit fields
QUERY_CODES = {"e2m1": ROW_BYTES, "e2m3": Q6_ROW_BYTES}   # query_code -> code bytes per token


def _check_format(dtype: torch.dtype, width: int, what: str, query_code: str = "e2m1") -> None:
    if dtype not in (torch.bfloat16, torch.float16) or width != DIM:
        narrow = "fp6_scores" if query_code == "e2m3" else "fp4_scores"
        hint = f"; a 128-wide corpus takes Fp4Index / {narrow}" if width == 128 else ""
        raise NotImplementedError(f"the wide fp4 index takes bfloat16 / float16 {what} of width {DIM} (got {dtype}, width {width})"
                                  f"{hint}")


def _check_query_code(query_code: str) -> int:
    """code bytes per token of a query code"""
    if query_code not in QUERY_CODES:
        raise ValueError(f"query_code must be 'e2m1' or 'e2m3' (got {query_code!r})")
    return QUERY_CODES[query_code]


def _encode_rows(rows_t: torch.Tensor, dev: torch.device, code: str = "e2m1") -> Tuple[torch.Tensor, torch.Tensor]:
    """codes uint8 [rows, 160] (e2m1) or [rows, 240] (e2m3) and scales uint8 [rows] of a [rows, 320] bf16 / f16 device tensor: one
    launch, asynchronous"""
    rows_t = rows_t if rows_t.is_contiguous() else rows_t.contiguous()
    rows = int(rows_t.shape[0])
    name = "msim_f6w_encode_rows" if code == "e2m3" else "msim_f4w_encode_rows"
    codes = torch.empty((rows, QUERY_CODES[code]), dtype=torch.uint8, device=dev)
    scales = torch.empty((rows,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), name)(_lib.dtype_code(rows_t.dtype), _lib.ptr(rows_t), rows, DIM, _lib.ptr(codes), _lib.ptr(scales),
                                       _lib.current_stream_handle(dev))
    _lib.check(rc, name)
    return codes, scales


class Fp4WideIndex:
    """The FP4 rows of one resident 320-wide shard: `codes` uint8 [rows, 160] in the corpus's row order (dimension k is nibble
    k & 1 of byte k >> 1, the low nibble the even k; a nibble is sign << 3 | e2m1 code), `scales` uint8 [rows] (E8M0: the row's
    values are the decoded codes times 2^(scale - 127)), the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n]
    or None), copied; `lengths` (int64 [n], host) and `id_base` as the corpus's."""

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor, offsets: torch.Tensor, clamp0: Optional[torch.Tensor],
                 lengths: torch.Tensor, id_base: int = 0):
        n = int(lengths.numel())
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != ROW_BYTES or not codes.is_contiguous():
            raise ValueError(f"codes must be a contiguous uint8 [rows, {ROW_BYTES}] tensor")
        if scales.dtype != torch.uint8 or scales.shape != (codes.shape[0],) or not scales.is_contiguous():
            raise ValueError(f"scales must be a contiguous uint8 [{int(codes.shape[0])}] tensor")
        if offsets.shape != (n + 1,) or offsets.dtype != torch.int32:
            raise ValueError(f"offsets must be int32 [{n + 1}]")
        if clamp0 is not None and (clamp0.dtype != torch.uint8 or clamp0.shape != (n,)):
            raise ValueError(f"clamp0 must be uint8 [{n}] or None")
        self.codes, self.scales, self.offsets, self.clamp0 = codes, scales, offsets, clamp0
        self.lengths, self.id_base = lengths, int(id_base)

    def __len__(self) -> int:
        return int(self.lengths.numel())

    @property
    def device(self) -> torch.device:
        return self.codes.device

    @property
    def nbytes(self) -> int:
        n = sum(t.numel() * t.element_size() for t in (self.codes, self.scales, self.offsets))
        return n + (self.clamp0.numel() if self.clamp0 is not None else 0)

    @classmethod
    def build(cls, corpus: PackedCorpus) -> "Fp4WideIndex":
        """The FP4 code of every row of `corpus` (bf16 / f16, width 320): one launch over the blob.  Asynchronous on torch's
        current stream."""
        if not isinstance(corpus, PackedCorpus):
            raise NotImplementedError(f"Fp4WideIndex.build takes a PackedCorpus (got {type(corpus).__name__})")
        _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
        dev = _require_gpu(corpus.device)
        codes, scales = _encode_rows(corpus.blob, dev)
        clamp0 = corpus.clamp0.clone() if corpus.clamp0 is not None else None
        return cls(codes, scales, corpus.offsets.clone(), clamp0, corpus.lengths.clone(), corpus.id_base)

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write this index to `path` (colpali_amd/persist.py: one flat file, every chunk carrying its msim_digest)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, *, verify: bool = True, pages=None) -> "Fp4WideIndex":
        """The index saved at `path`, on `device`, every chunk verified where it landed; `pages=(lo, hi)`: those pages only
        (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, pages=pages, expect=cls)


def fp4_wide_quantize_queries(queries, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token codes uint8 [T, 160] and scales uint8 [T] of `queries` (a `PackedQueries`, a host list of [len_i, 320] tensors or
    a [n_q, Lq, 320] tensor, packed into the flat layout first), in the packed token order: the page rows' code."""
    if not isinstance(queries, PackedQueries):
        if device is None:
            device = queries.device if isinstance(queries, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        queries = _as_packed(queries, device, layout="flat")
    return _quantize_packed(queries)


def fp6_wide_quantize_queries(queries, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token e2m3 codes uint8 [T, 240] and scales uint8 [T] of `queries` (as `fp4_wide_quantize_queries` takes them), in the
    packed token order: dimension k is the 6-bit field (sign << 5 | code) at bit 6 k of the little-endian 240-byte row."""
    if not isinstance(queries, PackedQueries):
        if device is None:
            device = queries.device if isinstance(queries, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        queries = _as_packed(queries, device, layout="flat")
    return _quantize_packed(queries, "e2m3")


def _quantize_packed(q: PackedQueries, code: str = "e2m1") -> Tuple[torch.Tensor, torch.Tensor]:
    dev = _require_gpu(q.device)
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries")
    return _encode_rows(q.tokens, dev, code)


def fp4_wide_scores_from_codes(q_codes: torch.Tensor, q_scales: torch.Tensor, q_offsets: torch.Tensor, max_q_tokens: int,
                               index: Fp4WideIndex, out: Optional[torch.Tensor] = None, *, query_code: str = "e2m1") -> torch.Tensor:
    """fp32 [n_q, len(index)] (msim_f4w_scores) from coded queries (`fp4_wide_quantize_queries`): codes uint8 [T, 160], scales
    uint8 [T], offsets int32 [n_q + 1] on the device and a host bound on every query's token count.  `query_code="e2m3"`: codes
    uint8 [T, 240] from `fp6_wide_quantize_queries` (msim_f4w_scores_q6)."""
    width = _check_query_code(query_code)
    if q_codes.dtype != torch.uint8 or q_codes.dim() != 2 or q_codes.shape[1] != width or not q_codes.is_contiguous():
        raise ValueError(f"{query_code} query codes must be a contiguous uint8 [tokens, {width}] tensor (got {q_codes.dtype} "
                         f"{list(q_codes.shape)})")
    name = "msim_f4w_scores_q6" if query_code == "e2m3" else "msim_f4w_scores"
    dev = _require_gpu(index.device)
    for t in (q_codes, q_scales, q_offsets):
        if t.device != dev:
            raise ValueError("queries and index live on different devices")
    n_q, n = int(q_offsets.numel()) - 1, len(index)
    if out is None:
        out = torch.empty((n_q, n), dtype=torch.float32, device=dev)
    elif out.shape != (n_q, n) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous fp32 [{n_q}, {n}] tensor on {dev}")
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), name)(_lib.ptr(q_codes), _lib.ptr(q_scales), _lib.ptr(q_offsets), n_q, int(q_codes.shape[0]),
                                       int(max_q_tokens), _lib.ptr(index.codes), _lib.ptr(index.scales), _lib.ptr(index.offsets),
                                       _lib.ptr(index.clamp0), n, int(index.codes.shape[0]), DIM, _lib.ptr(out), max(n, 1),
                                       _lib.current_stream_handle(dev))
    _lib.check(rc, name)
    return out


def fp4_wide_scores(queries, index: Fp4WideIndex, out: Optional[torch.Tensor] = None, *, query_code: str = "e2m1") -> torch.Tensor:
    """Approximate MaxSim of every query against every page of the index: fp32 [n_q, len(index)], column j = page
    index.id_base + j.  A score's bits depend on its query and page only.  Asynchronous on torch's current stream.  Given a
    `PackedQueries` it never synchronises with the host and is hipGraph-capturable: its only allocations are torch tensors (the
    query codes and scales, and `out` when it is None), made on the current stream before the library calls.  `query_code`: how the
    query tokens are coded, "e2m1" (as the pages) or "e2m3" (`fp6_wide_scores`)."""
    _check_query_code(query_code)
    if not isinstance(index, Fp4WideIndex):
        hint = "; an Fp4Index of a 128-wide shard takes fp6_scores" if type(index).__name__ == "Fp4Index" and query_code == "e2m3" else ""
        raise TypeError(f"fp4_wide_scores takes an Fp4WideIndex (got {type(index).__name__}){hint}")
    dev = index.device
    q = _as_packed(queries, dev, layout="flat")
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries", query_code)
    if q.device != dev:
        raise ValueError("queries and index live on different devices")
    lens = q.lengths
    max_q = int(lens.max()) if lens.numel() else 0
    codes, scales = _quantize_packed(q, query_code)
    return fp4_wide_scores_from_codes(codes, scales, q.offsets, max_q, index, out=out, query_code=query_code)


def fp6_wide_scores(queries, index: Fp4WideIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`fp4_wide_scores` with the query tokens coded as e2m3 (FP6) against the same FP4 pages: a first stage with less query-side
    quantisation error from the same index, bit for bit reproducible in the same way.  The stage-1 hook of a retriever on a
    320-wide shard: `ShardedRetriever(shard, fp4_wide_score_fn=fp6_wide_scores)`.  A 128-wide shard takes `fp6_scores`."""
    return fp4_wide_scores(queries, index, out, query_code="e2m3")


MAX_RERANK_TOKENS = 128                            # the longest query of the list form (eight 16-token tiles in registers)


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
    width = _check_query_code(query_code)
    if not isinstance(index, Fp4WideIndex):
        other = "fp6_rerank_scores" if query_code == "e2m3" else "fp4_rerank_scores"
        hint = f"; an Fp4Index of a 128-wide shard takes {other}" if type(index).__name__ == "Fp4Index" else ""
        raise NotImplementedError(f"the wide fp4 rerank takes an Fp4WideIndex of a 320-wide shard (got {type(index).__name__}){hint}")
    dev = _require_gpu(index.device)
    q = _as_packed(queries, dev, layout="flat")
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries", query_code)
    if q.device != dev:
        raise ValueError("queries and index live on different devices")
    lens = q.lengths
    max_q = int(lens.max()) if lens.numel() else 0
    if max_q > MAX_RERANK_TOKENS:
        raise NotImplementedError(f"the wide fp4 rerank takes queries of at most {MAX_RERANK_TOKENS} tokens (got {max_q})")
    n_q, n = len(q), len(index)
    codes, scales = _quantize_packed(q, query_code)
    assert int(codes.shape[1]) == width
    name = "msim_f4w_candidates_q6" if query_code == "e2m3" else "msim_f4w_candidates"
    with torch.cuda.device(dev):
        candidates, m, ld_cand, out, ids, _ = _rerank_args(n_q, dev, candidates, out, lambda m: 0)
        rc = getattr(_lib.lib(), name)(_lib.ptr(codes), _lib.ptr(scales), _lib.ptr(q.offsets), n_q, int(codes.shape[0]), max_q,
                                       _lib.ptr(index.codes), _lib.ptr(index.scales), _lib.ptr(index.offsets), _lib.ptr(index.clamp0),
                                       n, int(index.codes.shape[0]), DIM, _lib.ptr(candidates), m, ld_cand, int(index.id_base),
                                       _lib.ptr(out), max(m, 1), _lib.ptr(ids), _lib.current_stream_handle(dev))
    _lib.check(rc, name)
    return out, ids


def fp6_wide_rerank_scores(queries, index: Fp4WideIndex, candidates: torch.Tensor, *, out: Optional[torch.Tensor] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`fp4_wide_rerank_scores` with the query tokens coded as e2m3 (FP6): the bits of `fp6_wide_scores` at the listed pages.  The
    refine hook to hand to a retriever beside `fp4_wide_score_fn=fp6_wide_scores`:
    `ShardedRetriever(shard, fp4_wide_rerank_fn=fp6_wide_rerank_scores)`.  An `Fp4Index` of a 128-wide shard takes
    `fp6_rerank_scores`."""
    return fp4_wide_rerank_scores(queries, index, candidates, query_code="e2m3", out=out)
