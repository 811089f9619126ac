"""Fixed dimensional encodings (FDE): a first stage for two-stage search whose cost is one dense GEMM.

Dhulipala et al., "MUVERA: Multi-Vector Retrieval via Fixed Dimensional Encodings" (NeurIPS 2024): every page and every query
becomes one vector of F = reps * 2^ksim * dproj values, and the inner product of a query's and a page's encodings approximates
their MaxSim (Chamfer similarity).  `FdeIndex.build` encodes a resident `PackedCorpus` once; `fde_scores` encodes the queries and
scores them against every page with one streamed MFMA GEMM (include/maxsim.h: msim_fde_*, colpali_amd/csrc/fde.hip); its top
`n_candidates` are then reranked exactly by `rerank` -- `ShardedRetriever.search(prefilter=index, n_candidates=m)`.

The reference's fast path, `get_topk_plaid` (processing_utils.py:189-244), delegates to FastPlaid, an approximate centroid index;
here `create_plaid_index` stays an exact scan and this module is the opt-in approximate first stage.  The MUVERA final
projection is not implemented.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from .corpus import PackedCorpus, _as_packed
from .scoring import _require_gpu

DIM = 128
WIDE_DIM = 320                    # colpali_amd/fde_wide.py
MAX_DIM = 65536


@dataclass(frozen=True)
class FdeConfig:
    """reps R, ksim (2^ksim buckets per rep), dproj (projected values per bucket), the seed of the random parameters, and whether a
    page's empty bucket takes its nearest row (fill_empty).  F = reps * 2^ksim * dproj must be a multiple of 256, at most 65536."""
    reps: int = 20
    ksim: int = 5
    dproj: int = 16
    seed: int = 0
    fill_empty: bool = True

    def __post_init__(self):
        for name in ("reps", "ksim", "dproj", "seed"):
            if not isinstance(getattr(self, name), int) or isinstance(getattr(self, name), bool):
                raise ValueError(f"FdeConfig.{name} must be an int, got {getattr(self, name)!r}")
        if not isinstance(self.fill_empty, bool):
            raise ValueError("FdeConfig.fill_empty must be a bool")
        if self.reps < 1:
            raise ValueError(f"FdeConfig.reps={self.reps}: at least 1")
        if not 1 <= self.ksim <= 6:
            raise ValueError(f"FdeConfig.ksim={self.ksim}: the kernels take 1 .. 6")
        if self.dproj not in (8, 16, 32, 64):
            raise ValueError(f"FdeConfig.dproj={self.dproj}: the kernels take 8, 16, 32 or 64")
        if self.dim % 256 or self.dim > MAX_DIM:
            raise ValueError(f"FdeConfig: F = reps x 2^ksim x dproj = {self.dim} must be a multiple of 256 and at most {MAX_DIM}")

    @property
    def buckets(self) -> int:
        return 1 << self.ksim

    @property
    def dim(self) -> int:
        """F, the length of one encoding."""
        return self.reps * self.buckets * self.dproj

    def params(self, width: int = DIM) -> Tuple[torch.Tensor, torch.Tensor]:
        """The random parameters, fp32 on the host, drawn in this fixed order from torch.Generator().manual_seed(seed):
        G [reps, ksim, width] standard normal (the bucket hyperplanes), S [reps, dproj, width] +-1 (the projections).
        width: 128 (the default: `FdeIndex`) or 320 (`FdeWideIndex`)."""
        if isinstance(width, bool) or width not in (DIM, WIDE_DIM):
            raise ValueError(f"FdeConfig.params(width={width!r}): the encoders take rows of width {DIM} or {WIDE_DIM}")
        g = torch.Generator().manual_seed(self.seed)
        G = torch.randn((self.reps, self.ksim, width), generator=g, dtype=torch.float32)
        S = torch.randint(0, 2, (self.reps, self.dproj, width), generator=g, dtype=torch.int64).to(torch.float32) * 2 - 1
        return G, S


def _check_format(dtype: torch.dtype, width: int, what: str) -> None:
    if dtype not in (torch.bfloat16, torch.float16) or width != DIM:
        raise NotImplementedError(f"FDE {what} take bfloat16 / float16 embeddings of width {DIM} (got {dtype}, width {width})")


def encode_corpus(corpus: PackedCorpus, config: FdeConfig, out: Optional[torch.Tensor] = None, *, lo: int = 0,
                  hi: Optional[int] = None, codes: Optional[torch.Tensor] = None,
                  params: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """Encodings of pages lo .. hi-1 of `corpus` into `out` [hi - lo, F] (the corpus dtype).  codes: optional uint8 [rows, reps] of the
    whole blob, where the bucket of every row of those pages is written (a test hook; NULL in production)."""
    dev = _require_gpu(corpus.device)
    _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
    hi = len(corpus) if hi is None else hi
    if not 0 <= lo <= hi <= len(corpus):
        raise ValueError(f"page range {lo} .. {hi} outside the corpus of {len(corpus)}")
    F = config.dim
    if out is None:
        out = torch.empty((hi - lo, F), dtype=corpus.blob.dtype, device=dev)
    elif out.shape != (hi - lo, F) or out.dtype != corpus.blob.dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous {corpus.blob.dtype} [{hi - lo}, {F}] tensor on {dev}")
    rows = int(corpus.blob.shape[0])
    if codes is not None and (codes.shape != (rows, config.reps) or codes.dtype != torch.uint8 or not codes.is_contiguous()
                              or codes.device != dev):
        raise ValueError(f"codes must be a contiguous uint8 [{rows}, {config.reps}] tensor on {dev}")
    G, S = params if params is not None else tuple(p.to(dev) for p in config.params())
    off = corpus.offsets[lo:]
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.msim_fde_encode_docs(_lib.dtype_code(corpus.blob.dtype), _lib.ptr(corpus.blob), _lib.ptr(off), hi - lo, rows, DIM,
                                    _lib.ptr(G), _lib.ptr(S), config.reps, config.ksim, config.dproj, int(config.fill_empty),
                                    _lib.ptr(out), _lib.ptr(codes), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_fde_encode_docs")
    return out


class FdeIndex:
    """The encodings of one resident shard: `Fd` [count, F] in the corpus dtype, for pages id_base .. id_base + count - 1."""

    def __init__(self, Fd: torch.Tensor, id_base: int, config: FdeConfig,
                 params: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        if Fd.dim() != 2 or Fd.shape[1] != config.dim or not Fd.is_contiguous():
            raise ValueError(f"Fd must be a contiguous [count, {config.dim}] tensor")
        self.Fd, self.id_base, self.config = Fd, int(id_base), config
        # (G, S) on the index's device: the query encoder reads them without a host copy inside a captured call
        self.params = params if params is not None else tuple(p.to(Fd.device) for p in config.params())

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
    def build(cls, corpus: PackedCorpus, config: FdeConfig = FdeConfig(), chunk_docs: int = 65536) -> "FdeIndex":
        """Encode every page of `corpus`, `chunk_docs` pages per launch, straight into the index (no copy of the corpus, no
        staging: the memory beyond `Fd` itself is the parameters' few KB).  Asynchronous on torch's current stream."""
        if chunk_docs < 1:
            raise ValueError("chunk_docs must be >= 1")
        dev = _require_gpu(corpus.device)
        _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
        n = len(corpus)
        Fd = torch.empty((n, config.dim), dtype=corpus.blob.dtype, device=dev)
        params = tuple(p.to(dev) for p in config.params())
        for lo in range(0, n, chunk_docs):
            hi = min(n, lo + chunk_docs)
            encode_corpus(corpus, config, Fd[lo:hi], lo=lo, hi=hi, params=params)
        return cls(Fd, corpus.id_base, config, params)

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write this index (its parameter tensors included) to `path` (colpali_amd/persist.py: one flat file, every chunk carrying its msim_digest)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, *, verify: bool = True, pages=None) -> "FdeIndex":
        """The index (its parameter tensors included) saved at `path`, on `device`, every chunk verified where it landed; `pages=(lo, hi)`: those pages only
        (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, pages=pages, expect=cls)


def encode_queries(queries, index: FdeIndex, out: Optional[torch.Tensor] = None, *,
                   codes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Encodings [n_q, F] of `queries` (a `PackedQueries`, a host list of [len_i, 128] tensors or a [n_q, Lq, 128] tensor) under
    the index's configuration, in its dtype.  codes: optional uint8 [tokens, reps] of the packed tokens (a test hook).
    With a `PackedQueries` the call is asynchronous and hipGraph-capturable."""
    dev = index.device
    config = index.config
    q = _as_packed(queries, dev, layout="flat")
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries")
    if q.dtype != index.dtype:
        raise RuntimeError(f"expected queries and index of one dtype, got {q.dtype} and {index.dtype}")
    if q.device != dev:
        raise ValueError("queries and index live on different devices")
    n_q = len(q)
    F = config.dim
    if out is None:
        out = torch.empty((n_q, F), dtype=q.dtype, device=dev)
    elif out.shape != (n_q, F) or out.dtype != q.dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous {q.dtype} [{n_q}, {F}] tensor on {dev}")
    rows = int(q.tokens.shape[0])
    if codes is not None and (codes.shape != (rows, config.reps) or codes.dtype != torch.uint8 or not codes.is_contiguous()
                              or codes.device != dev):
        raise ValueError(f"codes must be a contiguous uint8 [{rows}, {config.reps}] tensor on {dev}")
    G, S = index.params
    tokens = q.tokens if q.tokens.is_contiguous() else q.tokens.contiguous()
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.msim_fde_encode_queries(_lib.dtype_code(q.dtype), _lib.ptr(tokens), _lib.ptr(q.offsets), n_q, rows, DIM, _lib.ptr(G),
                                       _lib.ptr(S), config.reps, config.ksim, config.dproj, _lib.ptr(out), _lib.ptr(codes),
                                       _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_fde_encode_queries")
    return out


def scores_from_encodings(Fq: torch.Tensor, Fd: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n_q, n_d] = Fq [n_q, F] . Fd [n_d, F]^T (msim_fde_scores).  out: a contiguous fp32 [n_q, n_d] tensor, or None."""
    if Fq.dim() != 2 or Fd.dim() != 2 or Fq.shape[1] != Fd.shape[1] or Fq.dtype != Fd.dtype or Fq.device != Fd.device:
        raise ValueError("Fq [n_q, F] and Fd [n_d, F] must share F, dtype and device")
    if Fq.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"msim_fde_scores takes bfloat16 / float16 encodings (got {Fq.dtype})")
    dev = _require_gpu(Fd.device)
    Fq, Fd = Fq.contiguous(), Fd.contiguous()
    n_q, n_d = int(Fq.shape[0]), int(Fd.shape[0])
    if out is None:
        out = torch.empty((n_q, n_d), dtype=torch.float32, device=dev)
    elif out.shape != (n_q, n_d) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous fp32 [{n_q}, {n_d}] tensor on {dev}")
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.msim_fde_scores(_lib.dtype_code(Fq.dtype), _lib.ptr(Fq), n_q, _lib.ptr(Fd), n_d, int(Fq.shape[1]), _lib.ptr(out),
                               max(n_d, 1), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_fde_scores")
    return out


def fde_scores(queries, index: FdeIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Approximate MaxSim of every query against every page of the index: fp32 [n_q, len(index)], column j = page
    index.id_base + j.  A query's scores have the same bits whatever other queries share the call."""
    return scores_from_encodings(encode_queries(queries, index), index.Fd, out=out)
