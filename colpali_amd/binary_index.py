"""A 1-bit sign index: a token-level first stage for two-stage search at 16 bytes per corpus row.

`BinaryIndex.build` keeps one sign bit per dimension of every row of a resident `PackedCorpus`: 1/16 of the bf16 shard.
`binary_scores` quantizes the queries per token to int8 (the int8 index's query side, unchanged) and scores every page by MaxSim
against the +-1 rows on int8 MFMAs (include/maxsim.h: msim_bin_*, colpali_amd/csrc/binary_index.hip); every per-token maximum is
an exact integer.  Its top `n_candidates` are reranked exactly -- `ShardedRetriever.search(prefilter=index, n_candidates=m)` -- so
every returned score is the exact one.  The index carries no trained parameter: stage-1 scores of different shards are comparable.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .corpus import PackedCorpus, _as_packed
from .int8_index import _quantize_packed
from .scoring import _require_gpu

DIM = 128
ROW_BYTES = DIM // 8


def _check_format(dtype: torch.dtype, width: int, what: str) -> None:
    if dtype not in (torch.bfloat16, torch.float16) or width != DIM:
        raise NotImplementedError(f"the binary index takes bfloat16 / float16 {what} of width {DIM} (got {dtype}, width {width})")


class BinaryIndex:
    """The sign bits of one resident shard: `codes` uint8 [rows, 16] in the corpus's row order (dimension k is bit k & 7 of byte
    k >> 3, set = +1), the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n] or None), copied; `lengths`
    (int64 [n], host) and `id_base` as the corpus's."""

    def __init__(self, codes: torch.Tensor, offsets: torch.Tensor, clamp0: Optional[torch.Tensor], lengths: torch.Tensor,
                 id_base: int = 0):
        n = int(lengths.numel())
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != ROW_BYTES or not codes.is_contiguous():
            raise ValueError(f"codes must be a contiguous uint8 [rows, {ROW_BYTES}] tensor")
        if offsets.shape != (n + 1,) or offsets.dtype != torch.int32:
            raise ValueError(f"offsets must be int32 [{n + 1}]")
        if clamp0 is not None and (clamp0.dtype != torch.uint8 or clamp0.shape != (n,)):
            raise ValueError(f"clamp0 must be uint8 [{n}] or None")
        self.codes, self.offsets, self.clamp0 = codes, offsets, clamp0
        self.lengths, self.id_base = lengths, int(id_base)

    def __len__(self) -> int:
        return int(self.lengths.numel())

    @property
    def device(self) -> torch.device:
        return self.codes.device

    @property
    def nbytes(self) -> int:
        n = sum(t.numel() * t.element_size() for t in (self.codes, self.offsets))
        return n + (self.clamp0.numel() if self.clamp0 is not None else 0)

    @classmethod
    def build(cls, corpus: PackedCorpus) -> "BinaryIndex":
        """The sign bits of every row of `corpus` (bf16 / f16, width 128): one launch over the blob.  Asynchronous on torch's
        current stream."""
        _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
        dev = _require_gpu(corpus.device)
        rows = int(corpus.blob.shape[0])
        codes = torch.empty((rows, ROW_BYTES), dtype=torch.uint8, device=dev)
        blob = corpus.blob if corpus.blob.is_contiguous() else corpus.blob.contiguous()
        with torch.cuda.device(dev):
            rc = _lib.lib().msim_bin_encode_rows(_lib.dtype_code(blob.dtype), _lib.ptr(blob), rows, DIM, _lib.ptr(codes),
                                                 _lib.current_stream_handle(dev))
        _lib.check(rc, "msim_bin_encode_rows")
        clamp0 = corpus.clamp0.clone() if corpus.clamp0 is not None else None
        return cls(codes, corpus.offsets.clone(), clamp0, corpus.lengths.clone(), corpus.id_base)

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write this index to `path` (colpali_amd/persist.py: one flat file, every chunk carrying its msim_digest)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, *, verify: bool = True, pages=None) -> "BinaryIndex":
        """The index saved at `path`, on `device`, every chunk verified where it landed; `pages=(lo, hi)`: those pages only
        (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, pages=pages, expect=cls)


def binary_scores_from_codes(q_codes: torch.Tensor, q_scales: torch.Tensor, q_offsets: torch.Tensor, max_q_tokens: int,
                             index: BinaryIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n_q, len(index)] (msim_bin_scores) from quantized queries (`quantize_queries`): codes int8 [T, 128], scales [T],
    offsets int32 [n_q + 1] on the device and a host bound on every query's token count."""
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
        rc = _lib.lib().msim_bin_scores(_lib.ptr(q_codes), _lib.ptr(q_scales), _lib.ptr(q_offsets), n_q, int(q_codes.shape[0]),
                                        int(max_q_tokens), _lib.ptr(index.codes), _lib.ptr(index.offsets), _lib.ptr(index.clamp0), n,
                                        int(index.codes.shape[0]), DIM, _lib.ptr(out), max(n, 1), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_bin_scores")
    return out


def binary_scores(queries, index: BinaryIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
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
    return binary_scores_from_codes(codes, scales, q.offsets, max_q, index, out=out)
