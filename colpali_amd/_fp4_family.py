"""The host layer of the FP4 index family, once for both widths: `Fp4Index` (128, colpali_amd/fp4_index.py) and `Fp4WideIndex` (320,
colpali_amd/fp4_wide_index.py) are this module's `Index` bound to a `Family`, and their functions are this module's, given that
family.  A family is data -- the width, the ABI symbols, the words of its messages, and the two checks only the wide side makes --
so what the two widths do differently is read in one place.  The kernels stay apart, a body per width and query code (DESIGN.md
section 3.32); nothing here chooses between them but the symbol names."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .corpus import PackedCorpus, PackedQueries, _as_packed, _rerank_args
from .scoring import _require_gpu

MAX_RERANK_TOKENS = 128                            # the longest query of the list form (eight 16-token tiles in registers)


@dataclass(eq=False)
class Family:
    dim: int
    encode: Dict[str, str]                         # query_code -> ABI symbol; the pages' code is "e2m1"
    scan: Dict[str, str]
    candidates: Dict[str, str]
    words: str                                     # "<words> index takes ...", "<words> rerank takes ..."
    scores_name: str                               # the scan function, as its TypeError names it
    build_checks_corpus: bool                      # `build` refuses what is not a PackedCorpus (else: an AttributeError further on)
    scores_checks_index: bool                      # the scan function refuses what is not the family's class
    sibling_dim: int                               # a caller of that width, or with the sibling's class, is told where to go:
    sibling_cls: str
    hints: Dict[Tuple[str, str], str] = field(default_factory=dict)   # (check, query_code) -> what the message ends with
    cls: Optional[type] = None                     # the index class, set when it is defined

    def __post_init__(self):
        self.row_bytes = self.dim // 2                                           # a row of e2m1 nibbles
        self.query_codes = {"e2m1": self.row_bytes, "e2m3": self.dim * 6 // 8}   # query_code -> code bytes per token


NARROW = Family(128, encode={"e2m1": "msim_f4_encode_rows", "e2m3": "msim_f6_encode_rows"},
                scan={"e2m1": "msim_f4_scores", "e2m3": "msim_f4_scores_q6"},
                candidates={"e2m1": "msim_f4_candidates", "e2m3": "msim_f4_candidates_q6"}, words="the fp4", scores_name="fp4_scores",
                build_checks_corpus=False, scores_checks_index=False, sibling_dim=320, sibling_cls="Fp4WideIndex")
WIDE = Family(320, encode={"e2m1": "msim_f4w_encode_rows", "e2m3": "msim_f6w_encode_rows"},
              scan={"e2m1": "msim_f4w_scores", "e2m3": "msim_f4w_scores_q6"},
              candidates={"e2m1": "msim_f4w_candidates", "e2m3": "msim_f4w_candidates_q6"}, words="the wide fp4",
              scores_name="fp4_wide_scores", build_checks_corpus=True, scores_checks_index=True, sibling_dim=128, sibling_cls="Fp4Index",
              hints={("format", "e2m1"): "; a 128-wide corpus takes Fp4Index / fp4_scores",
                     ("format", "e2m3"): "; a 128-wide corpus takes Fp4Index / fp6_scores",
                     ("scores", "e2m3"): "; an Fp4Index of a 128-wide shard takes fp6_scores",
                     ("rerank", "e2m1"): "; an Fp4Index of a 128-wide shard takes fp4_rerank_scores",
                     ("rerank", "e2m3"): "; an Fp4Index of a 128-wide shard takes fp6_rerank_scores"})
FAMILIES = {f.dim: f for f in (NARROW, WIDE)}      # by row width


def check_format(fam: Family, dtype: torch.dtype, width: int, what: str, query_code: str = "e2m1") -> None:
    if dtype not in (torch.bfloat16, torch.float16) or width != fam.dim:
        hint = fam.hints.get(("format", query_code), "") if width == fam.sibling_dim else ""
        raise NotImplementedError(f"{fam.words} index takes bfloat16 / float16 {what} of width {fam.dim} (got {dtype}, width {width})"
                                  f"{hint}")


def check_query_code(fam: Family, query_code: str) -> int:
    """code bytes per token of a query code"""
    if query_code not in fam.query_codes:
        raise ValueError(f"query_code must be 'e2m1' or 'e2m3' (got {query_code!r})")
    return fam.query_codes[query_code]


def _sibling_hint(fam: Family, check: str, index, query_code: str) -> str:
    return fam.hints.get((check, query_code), "") if type(index).__name__ == fam.sibling_cls else ""


def encode_rows(fam: Family, rows_t: torch.Tensor, dev: torch.device, code: str = "e2m1") -> Tuple[torch.Tensor, torch.Tensor]:
    """codes uint8 [rows, dim / 2] (e2m1) or [rows, dim * 3 / 4] (e2m3) and scales uint8 [rows] of a [rows, dim] bf16 / f16 device
    tensor: one launch, asynchronous"""
    rows_t = rows_t if rows_t.is_contiguous() else rows_t.contiguous()
    rows = int(rows_t.shape[0])
    name = fam.encode[code]
    codes = torch.empty((rows, fam.query_codes[code]), dtype=torch.uint8, device=dev)
    scales = torch.empty((rows,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), name)(_lib.dtype_code(rows_t.dtype), _lib.ptr(rows_t), rows, fam.dim, _lib.ptr(codes), _lib.ptr(scales),
                                       _lib.current_stream_handle(dev))
    _lib.check(rc, name)
    return codes, scales


class Index:
    """What `Fp4Index` and `Fp4WideIndex` share; a subclass names its `family`."""
    family: Family

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls.family.cls = cls

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor, offsets: torch.Tensor, clamp0: Optional[torch.Tensor],
                 lengths: torch.Tensor, id_base: int = 0):
        n, row_bytes = int(lengths.numel()), self.family.row_bytes
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != row_bytes or not codes.is_contiguous():
            raise ValueError(f"codes must be a contiguous uint8 [rows, {row_bytes}] tensor")
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
    def build(cls, corpus: PackedCorpus):
        """The FP4 code of every row of `corpus` (bf16 / f16, of the class's width): one launch over the blob.  Asynchronous on
        torch's current stream."""
        fam = cls.family
        if fam.build_checks_corpus and not isinstance(corpus, PackedCorpus):
            raise NotImplementedError(f"{cls.__name__}.build takes a PackedCorpus (got {type(corpus).__name__})")
        check_format(fam, corpus.blob.dtype, int(corpus.blob.shape[1]), "pages")
        dev = _require_gpu(corpus.device)
        codes, scales = encode_rows(fam, corpus.blob, dev)
        clamp0 = corpus.clamp0.clone() if corpus.clamp0 is not None else None
        return cls(codes, scales, corpus.offsets.clone(), clamp0, corpus.lengths.clone(), corpus.id_base)

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write this index to `path` (colpali_amd/persist.py: one flat file, every chunk carrying its msim_digest)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, *, verify: bool = True, pages=None):
        """The index saved at `path`, on `device`, every chunk verified where it landed; `pages=(lo, hi)`: those pages only
        (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, pages=pages, expect=cls)


def quantize_packed(fam: Family, q: PackedQueries, code: str = "e2m1") -> Tuple[torch.Tensor, torch.Tensor]:
    dev = _require_gpu(q.device)
    check_format(fam, q.dtype, int(q.tokens.shape[1]), "queries")
    return encode_rows(fam, q.tokens, dev, code)


def quantize_queries(fam: Family, queries, device: Optional[torch.device], code: str) -> Tuple[torch.Tensor, torch.Tensor]:
    if not isinstance(queries, PackedQueries):
        if device is None:
            device = queries.device if isinstance(queries, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        queries = _as_packed(queries, device, layout="flat")
    return quantize_packed(fam, queries, code)


def scores_from_codes(fam: Family, q_codes: torch.Tensor, q_scales: torch.Tensor, q_offsets: torch.Tensor, max_q_tokens: int, index,
                      out: Optional[torch.Tensor], query_code: str) -> torch.Tensor:
    width = check_query_code(fam, query_code)
    if q_codes.dtype != torch.uint8 or q_codes.dim() != 2 or q_codes.shape[1] != width or not q_codes.is_contiguous():
        raise ValueError(f"{query_code} query codes must be a contiguous uint8 [tokens, {width}] tensor (got {q_codes.dtype} "
                         f"{list(q_codes.shape)})")
    name = fam.scan[query_code]
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
                                       _lib.ptr(index.clamp0), n, int(index.codes.shape[0]), fam.dim, _lib.ptr(out), max(n, 1),
                                       _lib.current_stream_handle(dev))
    _lib.check(rc, name)
    return out


def _packed_for(fam: Family, queries, dev: torch.device, query_code: str) -> Tuple[PackedQueries, int]:
    """the flat queries of a scoring call, checked, and the host bound on their token counts"""
    q = _as_packed(queries, dev, layout="flat")
    check_format(fam, q.dtype, int(q.tokens.shape[1]), "queries", query_code)
    if q.device != dev:
        raise ValueError("queries and index live on different devices")
    lens = q.lengths
    return q, int(lens.max()) if lens.numel() else 0


def scores(fam: Family, queries, index, out: Optional[torch.Tensor], query_code: str) -> torch.Tensor:
    check_query_code(fam, query_code)
    if fam.scores_checks_index and not isinstance(index, fam.cls):
        raise TypeError(f"{fam.scores_name} takes an {fam.cls.__name__} (got {type(index).__name__})"
                        f"{_sibling_hint(fam, 'scores', index, query_code)}")
    q, max_q = _packed_for(fam, queries, index.device, query_code)
    codes, scales = quantize_packed(fam, q, query_code)
    return scores_from_codes(fam, codes, scales, q.offsets, max_q, index, out, query_code)


def rerank_scores(fam: Family, queries, index, candidates: torch.Tensor, query_code: str, out: Optional[torch.Tensor]
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    width = check_query_code(fam, query_code)
    if not isinstance(index, fam.cls):
        raise NotImplementedError(f"{fam.words} rerank takes an {fam.cls.__name__} of a {fam.dim}-wide shard (got {type(index).__name__})"
                                  f"{_sibling_hint(fam, 'rerank', index, query_code)}")
    dev = _require_gpu(index.device)
    q, max_q = _packed_for(fam, queries, dev, query_code)
    if max_q > MAX_RERANK_TOKENS:
        raise NotImplementedError(f"{fam.words} rerank takes queries of at most {MAX_RERANK_TOKENS} tokens (got {max_q})")
    n_q, n = len(q), len(index)
    codes, scales = quantize_packed(fam, q, query_code)
    assert int(codes.shape[1]) == width
    name = fam.candidates[query_code]
    with torch.cuda.device(dev):
        candidates, m, ld_cand, out, ids, _ = _rerank_args(n_q, dev, candidates, out, lambda m: 0)
        rc = getattr(_lib.lib(), name)(_lib.ptr(codes), _lib.ptr(scales), _lib.ptr(q.offsets), n_q, int(codes.shape[0]), max_q,
                                       _lib.ptr(index.codes), _lib.ptr(index.scales), _lib.ptr(index.offsets), _lib.ptr(index.clamp0),
                                       n, int(index.codes.shape[0]), fam.dim, _lib.ptr(candidates), m, ld_cand, int(index.id_base),
                                       _lib.ptr(out), max(m, 1), _lib.ptr(ids), _lib.current_stream_handle(dev))
    _lib.check(rc, name)
    return out, ids
