"""An int8 token-level index: a first stage for two-stage search that keeps MaxSim's token structure.

`Int8Index.build` quantizes a resident `PackedCorpus` (full pages or pooled ones) once: one int8 row per corpus row, one fp32 scale
per page.  `int8_scores` quantizes the queries per token and scores every page on int8 MFMAs (include/maxsim.h: msim_i8_*,
colpali_amd/csrc/int8_index.hip): 128 B per row streamed instead of 256 B, at twice the bf16 matrix rate.  Its top `n_candidates`
are reranked exactly by `rerank` -- `ShardedRetriever.search(prefilter=index, n_candidates=m)` -- so every returned score is the
exact one.  The bf16 corpus stays as it is: the index is an extra, opt-in copy.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .corpus import PackedCorpus, PackedQueries, _as_packed
from .scoring import _require_gpu

DIM = 128


def _check_format(dtype: torch.dtype, width: int, what: str) -> None:
    if dtype not in (torch.bfloat16, torch.float16) or width != DIM:
        raise NotImplementedError(f"the int8 index takes bfloat16 / float16 {what} of width {DIM} (got {dtype}, width {width})")


class Int8Index:
    """The int8 copy of one resident shard: `codes` int8 [rows, 128] in the corpus's row order, `scales` fp32 [n] (one per page),
    the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n] or None), copied; `lengths` (int64 [n], host) and
    `id_base` as the corpus's."""

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor, offsets: torch.Tensor, clamp0: Optional[torch.Tensor],
                 lengths: torch.Tensor, id_base: int = 0):
        n = int(lengths.numel())
        if codes.dtype != torch.int8 or codes.dim() != 2 or codes.shape[1] != DIM or not codes.is_contiguous():
            raise ValueError(f"codes must be a contiguous int8 [rows, {DIM}] tensor")
        if scales.dtype != torch.float32 or scales.shape != (n,) or offsets.shape != (n + 1,) or offsets.dtype != torch.int32:
            raise ValueError(f"scales must be fp32 [{n}] and offsets int32 [{n + 1}]")
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
    def build(cls, corpus: PackedCorpus, chunk_docs: int = 65536) -> "Int8Index":
        """Quantize every page of `corpus` (bf16 / f16, width 128), `chunk_docs` pages per launch, straight into the index.
        Asynchronous on torch's current stream."""
        if chunk_docs < 1:
            raise ValueError("chunk_docs must be >= 1")
        dev = _require_gpu(corpus.device)
        _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
        n, rows = len(corpus), int(corpus.blob.shape[0])
        codes = torch.empty((rows, DIM), dtype=torch.int8, device=dev)
        scales = torch.empty((n,), dtype=torch.float32, device=dev)
        blob = corpus.blob if corpus.blob.is_contiguous() else corpus.blob.contiguous()
        L = _lib.lib()
        with torch.cuda.device(dev):
            for lo in range(0, n, chunk_docs):
                hi = min(n, lo + chunk_docs)
                rc = L.msim_i8_encode_docs(_lib.dtype_code(blob.dtype), _lib.ptr(blob), _lib.ptr(corpus.offsets[lo:]), hi - lo, rows,
                                           DIM, _lib.ptr(codes), _lib.ptr(scales[lo:]), _lib.current_stream_handle(dev))
                _lib.check(rc, "msim_i8_encode_docs")
        clamp0 = corpus.clamp0.clone() if corpus.clamp0 is not None else None
        return cls(codes, scales, corpus.offsets.clone(), clamp0, corpus.lengths.clone(), corpus.id_base)

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write this index to `path` (colpali_amd/persist.py: one flat file, every chunk carrying its msim_digest)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, *, verify: bool = True, pages=None) -> "Int8Index":
        """The index saved at `path`, on `device`, every chunk verified where it landed; `pages=(lo, hi)`: those pages only
        (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, pages=pages, expect=cls)


def quantize_queries(queries, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token codes int8 [T, 128] and scales fp32 [T] of `queries` (a `PackedQueries`, a host list of [len_i, 128] tensors or a
    [n_q, Lq, 128] tensor, packed into the flat layout first), in the packed token order."""
    if not isinstance(queries, PackedQueries):
        if device is None:
            device = queries.device if isinstance(queries, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        queries = _as_packed(queries, device, layout="flat")
    return _quantize_packed(queries)


def _quantize_packed(q: PackedQueries) -> Tuple[torch.Tensor, torch.Tensor]:
    dev = _require_gpu(q.device)
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries")
    tokens = q.tokens if q.tokens.is_contiguous() else q.tokens.contiguous()
    rows = int(tokens.shape[0])
    codes = torch.empty((rows, DIM), dtype=torch.int8, device=dev)
    scales = torch.empty((rows,), dtype=torch.float32, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.msim_i8_encode_queries(_lib.dtype_code(q.dtype), _lib.ptr(tokens), rows, DIM, _lib.ptr(codes), _lib.ptr(scales),
                                      _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_i8_encode_queries")
    return codes, scales


def scores_from_codes(q_codes: torch.Tensor, q_scales: torch.Tensor, q_offsets: torch.Tensor, max_q_tokens: int, index: Int8Index,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n_q, len(index)] (msim_i8_scores) from quantized queries: codes [T, 128], scales [T], offsets int32 [n_q + 1] on the
    device and a host bound on every query's token count."""
    dev = _require_gpu(index.device)
    for t in (q_codes, q_scales, q_offsets):
        if t.device != dev:
            raise ValueError("queries and index live on different devices")
    n_q, n = int(q_offsets.numel()) - 1, len(index)
    if out is None:
        out = torch.empty((n_q, n), dtype=torch.float32, device=dev)
    elif out.shape != (n_q, n) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous fp32 [{n_q}, {n}] tensor on {dev}")
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.msim_i8_scores(_lib.ptr(q_codes), _lib.ptr(q_scales), _lib.ptr(q_offsets), n_q, int(q_codes.shape[0]), int(max_q_tokens),
                              _lib.ptr(index.codes), _lib.ptr(index.scales), _lib.ptr(index.offsets), _lib.ptr(index.clamp0), n,
                              int(index.codes.shape[0]), DIM, _lib.ptr(out), max(n, 1), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_i8_scores")
    return out


def int8_scores(queries, index: Int8Index, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Approximate MaxSim of every query against every page of the index: fp32 [n_q, len(index)], column j = page
    index.id_base + j.  A score's bits depend on its query and page only.  Asynchronous on torch's current stream.  Given a
    `PackedQueries` it never synchronises with the host and is hipGraph-capturable: its only allocations are torch tensors (the
    query codes and scales, and `out` when it is None), made on the current stream before the library calls."""
    dev = index.device
    q = _as_packed(queries, dev, layout="flat")
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries")
    if q.device != dev:
        raise ValueError("queries and index live on different devices")
    lens = q.lengths
    max_q = int(lens.max()) if lens.numel() else 0
    codes, scales = _quantize_packed(q)
    return scores_from_codes(codes, scales, q.offsets, max_q, index, out=out)
