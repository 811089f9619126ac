"""Fixed dimensional encodings (colpali_amd/fde.py) of a 320-wide (ColQwen3) shard: a one-GEMM first stage for two-stage search.

`FdeWideIndex` is to `FdeIndex` what `Fp4WideIndex` is to `Fp4Index`: the same encoding with 128 replaced by 320 -- G [reps, ksim,
320] and S [reps, dproj, 320] from `FdeConfig.params(width=320)`, the bucket SUM for queries and MEAN for pages, fill-empty by
Hamming distance -- computed by an encoder of its own (include/maxsim.h: msim_fdew_*, colpali_amd/csrc/fde_wide.hip).  The
scorer depends on F alone: `fde_wide_scores` encodes the queries and runs the streamed MFMA GEMM of `fde_scores`
(msim_fde_scores).  `ShardedRetriever.search(prefilter=index, n_candidates=m)` reranks its top m exactly at width 320, and
`search(prefilter=index, n_candidates=m1, refine=<Fp4WideIndex>, n_refine=m2)` puts the FP4 rows between the two.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .corpus import PackedCorpus, PackedQueries, _as_packed, _dtype_width, check_query_list, max_flat_query_tokens
from .fde import WIDE_DIM as DIM
from .fde import FdeConfig, scores_from_encodings
from .scoring import _require_gpu


def _check_format(dtype: torch.dtype, width: int, what: str) -> None:
    if dtype not in (torch.bfloat16, torch.float16) or width != DIM:
        raise NotImplementedError(f"wide FDE {what} take bfloat16 / float16 embeddings of width {DIM} (got {dtype}, width {width})")


def _check_codes(codes: Optional[torch.Tensor], rows: int, reps: int, dev: torch.device) -> None:
    if codes is not None and (codes.shape != (rows, reps) or codes.dtype != torch.uint8 or not codes.is_contiguous()
                              or codes.device != dev):
        raise ValueError(f"codes must be a contiguous uint8 [{rows}, {reps}] tensor on {dev}")


def _out(out: Optional[torch.Tensor], n: int, F: int, dtype: torch.dtype, dev: torch.device) -> torch.Tensor:
    if out is None:
        return torch.empty((n, F), dtype=dtype, device=dev)
    if out.shape != (n, F) or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous {dtype} [{n}, {F}] tensor on {dev}")
    return out


def _pack_any_length(queries, dev: torch.device) -> PackedQueries:
    """The flat layout for queries of any length: up to `pack_queries`' cap (512 tokens at width 320, which belongs to the scan
    kernels, not to this encoder) its own packing; beyond it the tokens back to back as they stand."""
    dtype, width = _dtype_width(queries)
    _check_format(dtype, width, "queries")
    if isinstance(queries, torch.Tensor):
        if queries.dim() != 3:
            raise ValueError("a query tensor must be 3-D (n_queries, max_len, dim)")
        lens = [int(queries.shape[1])] * int(queries.shape[0])
    else:
        check_query_list(queries)
        lens = [int(q.shape[0]) for q in queries]
    if max(lens, default=0) <= max_flat_query_tokens(width):
        return _as_packed(queries, dev, layout="flat")
    if isinstance(queries, torch.Tensor):
        tokens = queries.to(dev, non_blocking=True).reshape(-1, width)
    else:
        tokens = torch.cat([q.to(dev, non_blocking=True) for q in queries])
    oh = torch.zeros(len(lens) + 1, dtype=torch.int32)
    torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0, out=oh[1:])
    return PackedQueries(tokens=tokens.contiguous(), offsets=oh.to(dev, non_blocking=True), offsets_host=oh)


def fde_wide_encode_corpus(corpus: PackedCorpus, config: FdeConfig, out: Optional[torch.Tensor] = None, *, lo: int = 0,
                           hi: Optional[int] = None, codes: Optional[torch.Tensor] = None,
                           params: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """Encodings of pages lo .. hi-1 of the 320-wide `corpus` into `out` [hi - lo, F] (the corpus dtype).  codes: optional uint8
    [rows, reps] of the whole blob, where the bucket of every row of those pages is written (a test hook; NULL in production)."""
    dev = _require_gpu(corpus.device)
    _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
    hi = len(corpus) if hi is None else hi
    if not 0 <= lo <= hi <= len(corpus):
        raise ValueError(f"page range {lo} .. {hi} outside the corpus of {len(corpus)}")
    out = _out(out, hi - lo, config.dim, corpus.blob.dtype, dev)
    rows = int(corpus.blob.shape[0])
    _check_codes(codes, rows, config.reps, dev)
    G, S = params if params is not None else tuple(p.to(dev) for p in config.params(DIM))
    off = corpus.offsets[lo:]
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.msim_fdew_encode_docs(_lib.dtype_code(corpus.blob.dtype), _lib.ptr(corpus.blob), _lib.ptr(off), hi - lo, rows, DIM,
                                     _lib.ptr(G), _lib.ptr(S), config.reps, config.ksim, config.dproj, int(config.fill_empty),
                                     _lib.ptr(out), _lib.ptr(codes), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_fdew_encode_docs")
    return out


class FdeWideIndex:
    """The encodings of one resident 320-wide shard: `Fd` [count, F] in the corpus dtype, for pages id_base .. id_base + count - 1."""

    def __init__(self, Fd: torch.Tensor, id_base: int, config: FdeConfig,
                 params: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        if Fd.dim() != 2 or Fd.shape[1] != config.dim or not Fd.is_contiguous():
            raise ValueError(f"Fd must be a contiguous [count, {config.dim}] tensor")
        self.Fd, self.id_base, self.config = Fd, int(id_base), config
        # (G, S) on the index's device: the query encoder reads them without a host copy inside a captured call
        self.params = tuple(params) if params is not None else tuple(p.to(Fd.device) for p in config.params(DIM))
        G, S = self.params
        if tuple(G.shape) != (config.reps, config.ksim, DIM) or tuple(S.shape) != (config.reps, config.dproj, DIM):
            raise ValueError(f"params must be G [{config.reps}, {config.ksim}, {DIM}] and S [{config.reps}, {config.dproj}, {DIM}]")

    width = DIM

    def __len__(self) -> int:
        return int(self.Fd.shape[0])

    @property
    def count(self) -> int:
        return len(self)

    @property
    def device(self) -> torch.device:
        return self.Fd.device

    @property
    def dtype(self) -> torch.dtype:
        return self.Fd.dtype

    @classmethod
    def build(cls, corpus: PackedCorpus, config: FdeConfig = FdeConfig(), chunk_docs: int = 65536) -> "FdeWideIndex":
        """Encode every page of the 320-wide `corpus`, `chunk_docs` pages per launch, straight into the index (no copy of the corpus,
        no staging).  A page's bits do not depend on `chunk_docs`.  Asynchronous on torch's current stream."""
        if chunk_docs < 1:
            raise ValueError("chunk_docs must be >= 1")
        dev = _require_gpu(corpus.device)
        _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
        n = len(corpus)
        Fd = torch.empty((n, config.dim), dtype=corpus.blob.dtype, device=dev)
        params = tuple(p.to(dev) for p in config.params(DIM))
        for lo in range(0, n, chunk_docs):
            hi = min(n, lo + chunk_docs)
            fde_wide_encode_corpus(corpus, config, Fd[lo:hi], lo=lo, hi=hi, params=params)
        return cls(Fd, corpus.id_base, config, params)

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write this index (its parameter tensors included) to `path` (colpali_amd/persist.py: one flat file, every chunk carrying its msim_digest)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, *, verify: bool = True, pages=None) -> "FdeWideIndex":
        """The index (its parameter tensors included) saved at `path`, on `device`, every chunk verified where it landed;
        `pages=(lo, hi)`: those pages only (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, pages=pages, expect=cls)


def fde_wide_encode_queries(queries, index: FdeWideIndex, out: Optional[torch.Tensor] = None, *,
                            codes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Encodings [n_q, F] of `queries` (a `PackedQueries`, a host list of [len_i, 320] tensors or a [n_q, Lq, 320] tensor; any
    length) under the index's configuration, in its dtype.  codes: optional uint8 [tokens, reps] of the packed tokens (a test
    hook).  With a `PackedQueries` the call is asynchronous and hipGraph-capturable."""
    dev = index.device
    config = index.config
    q = queries if isinstance(queries, PackedQueries) else _pack_any_length(queries, dev)
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries")
    if q.dtype != index.dtype:
        raise RuntimeError(f"expected queries and index of one dtype, got {q.dtype} and {index.dtype}")
    if q.device != dev:
        raise ValueError("queries and index live on different devices")
    n_q = len(q)
    out = _out(out, n_q, config.dim, q.dtype, dev)
    rows = int(q.tokens.shape[0])
    _check_codes(codes, rows, config.reps, dev)
    G, S = index.params
    tokens = q.tokens if q.tokens.is_contiguous() else q.tokens.contiguous()
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.msim_fdew_encode_queries(_lib.dtype_code(q.dtype), _lib.ptr(tokens), _lib.ptr(q.offsets), n_q, rows, DIM, _lib.ptr(G),
                                        _lib.ptr(S), config.reps, config.ksim, config.dproj, _lib.ptr(out), _lib.ptr(codes),
                                        _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_fdew_encode_queries")
    return out


def fde_wide_scores(queries, index: FdeWideIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Approximate MaxSim of every 320-wide query against every page of the index: fp32 [n_q, len(index)], column j = page
    index.id_base + j.  A query's scores have the same bits whatever other queries share the call."""
    return scores_from_encodings(fde_wide_encode_queries(queries, index), index.Fd, out=out)
