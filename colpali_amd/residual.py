"""A residual-compressed corpus (PLAID's second half): a resident shard that keeps no full-precision embedding.

`ResidualCorpus.build` stores every row of a `PackedCorpus` as its `CentroidIndex` code (2 bytes) plus `bits` (2 or 4) of residual
per dimension -- 34 or 66 bytes per row instead of 256 -- and the caller may then free the bf16 corpus.  The codec (include/maxsim.h:
msim_res_*, colpali_amd/csrc/residual_codec.hip):

    encode   e_k = fl32(float(x_k) - float(C[c]_k));  bucket b_k = #{cutoffs t : t <= e_k}
    pack     dimension k = bits [k * bits, k * bits + bits) of the row's 16 * bits bytes, a little-endian bit string
    decode   xhat_k = round_to_dtype(float(C[c]_k) + weights[b_k])   -- one rounding, NO renormalisation (ColBERTv2's Python path
             renormalises the decoded row; PLAID's kernels do not, and neither does this)

`residual_rerank_scores` reranks candidate lists straight from the compressed rows (each 32-row slab of a page is decoded in
registers into LDS and never written to memory); every score has the bits `rerank_scores` gives the same query against
`rc.decompress()`.  Stage 1 is `rc.index`, the `CentroidIndex` view over the same codes:
`ShardedRetriever(rc).search(q, k, prefilter=rc.index, n_candidates=m)`.

`residual_scores` is the full scan of such a shard (a page is decoded once per group of up to 8 queries, never written to memory):
the `[n_q, len(rc)]` matrix with the bits of `maxsim_scores(queries, rc.decompress())`.  It decodes every row of the shard, so the
retriever only scans on request: `ShardedRetriever(rc, score_fn=residual_scores)` opens the full scan, `filter=`, `group_by=` and
`mine`.

`residual_align` and `residual_gather_pages` are the two operations that return rows -- `align` and `gather_pages` -- with the
listed pages decoded inside the kernel that consumes them (colpali_amd/csrc/residual_align.hip): the bits of the same call over
`rc.decompress()`, no decoded copy in memory, no host read of the list.  `align(queries, rc, ids)` and `gather_pages(rc, ids)`
dispatch to them; `ShardedRetriever(rc, align_fn=residual_align)` opens the retriever's `align`.

The container, the build, `decompress` and the rerank are one host layer for both row widths (`_ResidualRows`: a public class binds
the width, its centroid-index class and the library entries that read rows of that width).  `ResidualCorpus` is width 128;
`ResidualWideCorpus` (colpali_amd/residual_wide.py) is width 320 -- a sibling, not a subclass, so the scan above (its own is
`residual_wide_scores`, over the same host body: `_scan_scores`) and `residual_align` / `residual_gather_pages` (its own are
`residual_wide_align` / `residual_wide_gather_pages`, over the same host bodies: `_align_rows`, `_gather_rows`) refuse it by its type.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .centroid import CentroidIndex, _CentroidCodes
from .corpus import PackedCorpus, PackedQueries, _as_packed, _dtype_width, _id_list, _rerank_args
from .scoring import _require_gpu

DIM = 128
WIDE_DIM = 320
BITS = (2, 4)


def _check_bits(bits) -> int:
    if isinstance(bits, bool) or not isinstance(bits, int) or bits not in BITS:
        raise ValueError(f"bits must be 2 or 4 (got {bits!r})")
    return bits


def _check_codec(cutoffs: torch.Tensor, weights: torch.Tensor, bits: int) -> None:
    nb = 1 << bits
    if cutoffs.dtype != torch.float32 or cutoffs.shape != (nb - 1,) or not cutoffs.is_contiguous():
        raise ValueError(f"cutoffs must be a contiguous fp32 [{nb - 1}] tensor")
    if weights.dtype != torch.float32 or weights.shape != (nb,) or not weights.is_contiguous():
        raise ValueError(f"weights must be a contiguous fp32 [{nb}] tensor")


def train_residual_codec(residual_sample: torch.Tensor, bits: int = 2, *, width: int = DIM) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cutoffs fp32 [2^bits - 1], weights fp32 [2^bits]) from sampled residuals fp32 [s, 128] (any device; plain torch: this is
    build time, like `train_centroids`).  `width=320` takes the [s, 320] samples of a `ResidualWideCorpus` instead: the sample's
    width must be the one named, 128 unless said otherwise.  Cutoff j (1 .. 2^bits - 1) is the j / 2^bits quantile of ALL sampled values: element
    floor(j * N / 2^bits) of the N sorted values.  Weight b is the mean of the values falling in bucket b (the number of cutoffs
    <= value); an empty bucket takes the midpoint of its cutoffs (an outer one, which has a single cutoff, that cutoff)."""
    bits = _check_bits(bits)
    if width not in (DIM, WIDE_DIM):
        raise ValueError(f"width must be {DIM} or {WIDE_DIM} (got {width!r})")
    if residual_sample.dim() != 2 or residual_sample.shape[1] != width or residual_sample.dtype != torch.float32:
        raise ValueError(f"residual_sample must be fp32 [s, {width}]")
    if residual_sample.shape[0] < 1:
        raise ValueError("residual_sample is empty")
    nb = 1 << bits
    vals = residual_sample.reshape(-1)
    srt = torch.sort(vals).values
    n = int(srt.numel())
    pick = torch.tensor([min(j * n // nb, n - 1) for j in range(1, nb)], dtype=torch.int64, device=srt.device)
    cutoffs = srt[pick].contiguous()
    # bucket b (the number of cutoffs <= value) is a contiguous run of the sorted values: it starts at the first value >= cutoff b - 1.
    # Sums from one float64 prefix sum, not from 2^bits-way atomics over every value
    zero = torch.zeros((1,), dtype=torch.int64, device=srt.device)
    edges = torch.cat([zero, torch.searchsorted(srt, cutoffs), zero + n])
    prefix = torch.cat([torch.zeros((1,), dtype=torch.float64, device=srt.device), torch.cumsum(srt.double(), 0)])
    sums = prefix[edges[1:]] - prefix[edges[:-1]]
    counts = edges[1:] - edges[:-1]
    lo = torch.cat([cutoffs[:1], cutoffs])                                # bucket b spans [lo[b], hi[b]]; the outer ones end at their cutoff
    hi = torch.cat([cutoffs, cutoffs[-1:]])
    mid = (lo.double() + hi.double()) / 2
    mean = sums / counts.clamp(min=1)
    weights = torch.where(counts > 0, mean, mid).float()
    inf = torch.full((1,), float("inf"), dtype=torch.float32, device=vals.device)
    weights = torch.maximum(torch.minimum(weights, torch.cat([cutoffs, inf])), torch.cat([-inf, cutoffs]))    # the fp32 rounding of a mean
    return cutoffs, weights.contiguous()


class _ResidualRows:
    """What the compressed shards of both widths are: `centroids` [K, WIDTH] (bf16 / f16), `codes` uint16 [rows], `residuals` uint8
    [rows, WIDTH / 8 * bits], `cutoffs` fp32 [2^bits - 1], `weights` fp32 [2^bits], the pages' `offsets` (int32 [n + 1], device),
    `clamp0` (uint8 [n] or None), `lengths` (int64 [n], host), `id_base` and `bits`.  `.index` is the centroid index of the same
    width over the SAME `codes` and `centroids` tensors (no copy).  A subclass sets WIDTH, its index class and the names of the
    library entries that read rows of that width."""

    WIDTH: int = 0
    _INDEX = None
    _ENCODE: str = ""
    _DECODE: str = ""
    _CANDIDATES: str = ""
    _SCORES: str = ""
    _ALIGN: str = ""
    _GATHER: str = ""

    def __init__(self, centroids: torch.Tensor, codes: torch.Tensor, residuals: torch.Tensor, cutoffs: torch.Tensor,
                 weights: torch.Tensor, offsets: torch.Tensor, clamp0: Optional[torch.Tensor], lengths: torch.Tensor,
                 id_base: int = 0, bits: int = 2):
        bits = _check_bits(bits)
        self.index = self._INDEX(centroids, codes, offsets, clamp0, lengths, id_base)         # validates what the two share
        _check_codec(cutoffs, weights, bits)
        row_bytes = self.WIDTH // 8 * bits
        if (residuals.dtype != torch.uint8 or residuals.dim() != 2 or residuals.shape != (codes.shape[0], row_bytes)
                or not residuals.is_contiguous()):
            raise ValueError(f"residuals must be a contiguous uint8 [{codes.shape[0]}, {row_bytes}] tensor")
        for name, t in (("centroids", centroids), ("residuals", residuals), ("cutoffs", cutoffs), ("weights", weights),
                        ("offsets", offsets)):
            if t.device != codes.device:
                raise ValueError(f"{name} live on {t.device}, the codes on {codes.device}")
        self.centroids, self.codes, self.residuals = centroids, codes, residuals
        self.cutoffs, self.weights = cutoffs, weights
        self.offsets, self.clamp0, self.lengths = offsets, clamp0, lengths
        self.id_base, self.bits = int(id_base), bits

    def __len__(self) -> int:
        return int(self.lengths.numel())

    @property
    def device(self) -> torch.device:
        return self.codes.device

    @property
    def dtype(self) -> torch.dtype:
        return self.centroids.dtype

    @property
    def width(self) -> int:
        return self.WIDTH

    @property
    def n_centroids(self) -> int:
        return int(self.centroids.shape[0])

    @property
    def nbytes(self) -> int:
        n = sum(t.numel() * t.element_size() for t in (self.centroids, self.codes, self.residuals, self.cutoffs, self.weights,
                                                       self.offsets))
        return n + (self.clamp0.numel() if self.clamp0 is not None else 0)

    @classmethod
    def build(cls, corpus: PackedCorpus, index: Optional[_CentroidCodes] = None, bits: int = 2,
              cutoffs: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None, sample_rows: int = 1 << 18,
              seed: int = 0, **centroid_kwargs):
        """Compress `corpus` (bf16 / f16, the class's width: 128 for `ResidualCorpus`, 320 for `ResidualWideCorpus`).  `index=None`
        builds the centroid index of that width first (`CentroidIndex` / `CentroidWideIndex`; `**centroid_kwargs` go to its
        `build`); a given one must be of that class and cover the corpus's pages and rows.  With given `cutoffs` and `weights` the build is
        bit-reproducible; otherwise they are trained (`train_residual_codec`) on the residuals of a seeded sample of `sample_rows`
        rows.  The corpus is not kept: the caller may free it.  Asynchronous on torch's current stream (training reads a few
        numbers back)."""
        bits = _check_bits(bits)
        dev = _require_gpu(corpus.device)
        W, kind = cls.WIDTH, cls._INDEX
        if corpus.blob.dtype not in (torch.bfloat16, torch.float16) or int(corpus.blob.shape[1]) != W:
            raise NotImplementedError(f"the residual codec takes bfloat16 / float16 pages of width {W} (got {corpus.blob.dtype}, "
                                      f"width {int(corpus.blob.shape[1])})")
        if (cutoffs is None) != (weights is None):
            raise ValueError("pass both cutoffs and weights, or neither")
        if sample_rows < 1:
            raise ValueError("sample_rows must be >= 1")
        if index is None:
            index = kind.build(corpus, **centroid_kwargs)
        elif centroid_kwargs:
            raise ValueError(f"{sorted(centroid_kwargs)} go to {kind.__name__}.build: they do not go with index=")
        rows = int(corpus.blob.shape[0])
        if (not isinstance(index, kind) or len(index) != len(corpus) or index.id_base != corpus.id_base or int(index.codes.shape[0]) != rows
                or index.device != dev or index.centroids.dtype != corpus.blob.dtype):
            raise ValueError(f"index must be a {kind.__name__} of this corpus (same pages, rows, id_base, dtype and device)")
        blob = corpus.blob if corpus.blob.is_contiguous() else corpus.blob.contiguous()
        if cutoffs is None:
            g = torch.Generator().manual_seed(int(seed))
            n_s = min(int(sample_rows), rows)
            pick = (torch.randperm(rows, generator=g)[:n_s] if rows <= 1 << 24 else torch.randint(0, rows, (n_s,), generator=g)).to(dev)
            c_of = (index.codes.view(torch.int16)[pick].to(torch.int64) & 0xFFFF).clamp(max=index.n_centroids - 1)
            sample = blob.index_select(0, pick).float() - index.centroids.index_select(0, c_of).float()
            cutoffs, weights = train_residual_codec(sample, bits, width=W)
        cutoffs, weights = cutoffs.to(dev), weights.to(dev)
        _check_codec(cutoffs, weights, bits)
        residuals = torch.empty((rows, W // 8 * bits), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = getattr(_lib.lib(), cls._ENCODE)(_lib.dtype_code(blob.dtype), _lib.ptr(blob), rows, W, _lib.ptr(index.codes),
                                                  _lib.ptr(index.centroids), index.n_centroids, _lib.ptr(cutoffs), bits,
                                                  _lib.ptr(residuals), _lib.current_stream_handle(dev))
        _lib.check(rc, cls._ENCODE)
        return cls(index.centroids, index.codes, residuals, cutoffs, weights, index.offsets, index.clamp0, index.lengths,
                   index.id_base, bits)

    def _decode(self, row0: int, row1: int, out: torch.Tensor) -> None:
        dev = self.device
        with torch.cuda.device(dev):
            rc = getattr(_lib.lib(), self._DECODE)(_lib.dtype_code(self.dtype), _lib.ptr(self.codes), _lib.ptr(self.residuals),
                                                   int(self.codes.shape[0]), row0, row1, _lib.ptr(self.centroids), self.n_centroids,
                                                   _lib.ptr(self.weights), self.bits, self.WIDTH, out.data_ptr(),
                                                   _lib.current_stream_handle(dev))
        _lib.check(rc, self._DECODE)

    def decompress(self, ids: Union[None, Sequence[int], torch.Tensor] = None) -> PackedCorpus:
        """The decoded pages as a `PackedCorpus` (msim_res_decode_rows / msim_res_wide_decode_rows): all of them (same offsets, clamp0 and id_base), or the
        listed LOCAL pages in the order given (id_base 0; only their rows are read)."""
        dev = _require_gpu(self.device)
        if ids is None:
            rows = int(self.lengths.sum()) if len(self) else 0
            blob = torch.zeros((max(rows, 1), self.WIDTH), dtype=self.dtype, device=dev)
            self._decode(0, rows, blob)
            clamp0 = self.clamp0.clone() if self.clamp0 is not None else None
            return PackedCorpus(blob=blob, offsets=self.offsets.clone(), clamp0=clamp0, lengths=self.lengths.clone(),
                                id_base=self.id_base)
        pages = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else list(ids), dtype=np.int64).reshape(-1)
        n = len(self)
        if pages.size and (pages.min() < 0 or pages.max() >= n):
            raise ValueError(f"decompress takes local page indices in 0 .. {n - 1}")
        ln = self.lengths.numpy().astype(np.int64, copy=False)
        start = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(ln, out=start[1:])
        sel = ln[pages]
        off = np.zeros(pages.size + 1, dtype=np.int64)
        np.cumsum(sel, out=off[1:])
        blob = torch.zeros((max(int(off[-1]), 1), self.WIDTH), dtype=self.dtype, device=dev)
        for i, p in enumerate(pages):
            if sel[i]:
                self._decode(int(start[p]), int(start[p + 1]), blob[int(off[i]):])
        clamp0 = self.clamp0[torch.from_numpy(pages).to(dev)] if self.clamp0 is not None else None
        return PackedCorpus(blob=blob, offsets=torch.from_numpy(off.astype(np.int32)).to(dev), clamp0=clamp0,
                            lengths=torch.from_numpy(sel.copy()), id_base=0)

    def save(self, path, *, chunk_bytes: int = 64 << 20) -> None:
        """Write this compressed corpus to `path` (colpali_amd/persist.py: one flat file, every chunk carrying its msim_digest)."""
        from . import persist

        persist.save(self, path, chunk_bytes=chunk_bytes)

    @classmethod
    def load(cls, path, device, *, verify: bool = True, pages=None):
        """The compressed corpus saved at `path`, on `device`, every chunk verified where it landed; `pages=(lo, hi)`: those pages only
        (`persist.load`)."""
        from . import persist

        return persist.load(path, device, verify=verify, pages=pages, expect=cls)


class ResidualCorpus(_ResidualRows):
    """One resident shard in compressed form: `centroids` [K, 128] (bf16 / f16), `codes` uint16 [rows], `residuals` uint8
    [rows, 16 * bits], `cutoffs` fp32 [2^bits - 1], `weights` fp32 [2^bits], the pages' `offsets` (int32 [n + 1], device), `clamp0`
    (uint8 [n] or None), `lengths` (int64 [n], host), `id_base` and `bits`.  `.index` is a `CentroidIndex` over the SAME `codes` and
    `centroids` tensors (no copy): the stage 1 that goes with this stage 2."""

    WIDTH = DIM
    _INDEX = CentroidIndex
    _ENCODE = "msim_res_encode_docs"
    _DECODE = "msim_res_decode_rows"
    _CANDIDATES = "msim_res_candidates"
    _SCORES = "msim_res_scores"
    _ALIGN = "msim_res_align_candidates"
    _GATHER = "msim_res_gather_pages"


def _check_query_format(queries, rc: _ResidualRows, what: str) -> None:
    """the formats the residual kernels take, in whatever form the queries came (no device work)"""
    q_dtype, dim = _dtype_width(queries)
    if q_dtype != rc.dtype:
        raise RuntimeError(f"expected queries and passages of one dtype, got {q_dtype} and {rc.dtype}")
    if q_dtype not in (torch.bfloat16, torch.float16) or dim != rc.WIDTH:
        raise NotImplementedError(f"the residual {what} takes bfloat16 / float16 embeddings of width {rc.WIDTH} (got {q_dtype}, width "
                                  f"{dim})")


def _require_kind(rc, kind, who: str) -> None:
    """the sibling classes refuse each other by type, naming the width: no kernel of one width ever sees rows of the other"""
    if isinstance(rc, _ResidualRows) and not isinstance(rc, kind):
        raise NotImplementedError(f"{who} of a {kind.__name__} exists at width {kind.WIDTH} only (got a {type(rc).__name__} of width "
                                  f"{rc.WIDTH})")
    if not isinstance(rc, kind):
        raise ValueError(f"rc must be a {kind.__name__}")


def _flat_queries(queries, rc, what: str, kind=None) -> Tuple[torch.device, PackedQueries]:
    """the query forms and checks the residual kernels share: a `PackedQueries`, a host list, or a dense device box.  `kind`: the
    class the caller's kernels take (the siblings refuse each other by type)"""
    kind = kind or ResidualCorpus
    _require_kind(rc, kind, f"the residual {what}")
    dev = _require_gpu(rc.device)
    _check_query_format(queries, rc, what)
    queries = _as_packed(queries, dev, layout="flat")
    if queries.device != dev:
        raise ValueError("queries and corpus live on different devices")
    return dev, queries


def residual_scores(queries, rc: ResidualCorpus, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxSim of every query against every page of the compressed shard (include/maxsim.h: msim_res_scores): fp32 [n_q, len(rc)],
    the counterpart of `maxsim_scores` over a `PackedCorpus`.  Entry (q, c) has the bits `maxsim_scores(queries, rc.decompress())`
    gives; every row of the shard is decoded, once per group of up to 8 queries (128 tokens).  The query forms and checks of
    `residual_rerank_scores`: a `PackedQueries`, a host list or a dense device box; RuntimeError on a dtype mismatch;
    NotImplementedError for fp32, a width other than 128 or a query over 128 tokens.  `out`: fp32 [n_q, n] with unit inner stride on
    the corpus' device -- it may be a column slice of a wider matrix, whose other columns are not touched.  Given a `PackedQueries`
    it never synchronises with the host and is hipGraph-capturable."""
    return _scan_scores(queries, rc, out, ResidualCorpus)


def _scan_scores(queries, rc, out: Optional[torch.Tensor], kind) -> torch.Tensor:
    """the full scan of both widths: the entry of `kind` over a shard of that class"""
    dev, queries = _flat_queries(queries, rc, "scan", kind)
    n_q, n = len(queries), len(rc)
    if out is None:
        out = torch.empty((n_q, n), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.shape != (n_q, n) or out.dtype != torch.float32 or out.device != dev
          or (n > 1 and out.stride(1) != 1) or (n_q > 1 and out.stride(0) < n)):
        raise ValueError(f"out must be an fp32 [n_q={n_q}, n={n}] tensor with unit inner stride on the corpus' device")
    ld = out.stride(0) if n_q > 1 else max(n, 1)
    L = _lib.lib()
    entry, ws_bytes = getattr(L, kind._SCORES), getattr(L, kind._SCORES + "_workspace_bytes")
    tokens = queries.tokens if queries.tokens.is_contiguous() else queries.tokens.contiguous()
    with torch.cuda.device(dev):
        ws = _lib.workspace(int(ws_bytes(n_q, n)), dev)
        rcode = entry(_lib.dtype_code(rc.dtype), _lib.ptr(tokens), _lib.ptr(queries.offsets), queries.offsets_host.data_ptr(), n_q,
                      _lib.ptr(rc.codes), _lib.ptr(rc.residuals), _lib.ptr(rc.centroids), rc.n_centroids, _lib.ptr(rc.weights), rc.bits,
                      _lib.ptr(rc.offsets), _lib.ptr(rc.clamp0), n, int(rc.codes.shape[0]), kind.WIDTH, _lib.ptr(out), max(ld, 1),
                      _lib.ptr(ws), _lib.current_stream_handle(dev))
    _lib.check(rcode, kind._SCORES)
    return out


def residual_rerank_scores(queries, rc: ResidualCorpus, candidates: torch.Tensor, *,
                           out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaxSim of listed candidates against the compressed pages (include/maxsim.h: msim_res_candidates): (scores fp32 [n_q, m], ids
    int64 [n_q, m]) with the signature, the query forms and the checks of `rerank_scores`.  Entry (q, j) has the bits
    `rerank_scores(queries, rc.decompress(), candidates)` gives; an id of -1 or outside [id_base, id_base + len(rc)) comes back as
    (-inf, -1).  bfloat16 / float16, width 128, queries of at most 128 tokens (NotImplementedError otherwise).  Given a
    `PackedQueries` it never synchronises with the host and is hipGraph-capturable."""
    return _rerank_scores(queries, rc, candidates, out, ResidualCorpus)


def _rerank_scores(queries, rc, candidates: torch.Tensor, out: Optional[torch.Tensor], kind) -> Tuple[torch.Tensor, torch.Tensor]:
    """the candidate rerank of both widths: the entry of `kind` over a shard of that class"""
    dev, queries = _flat_queries(queries, rc, "rerank", kind)
    n_q, n = len(queries), len(rc)
    L = _lib.lib()
    entry, ws_bytes = getattr(L, kind._CANDIDATES), getattr(L, kind._CANDIDATES + "_workspace_bytes")
    tokens = queries.tokens if queries.tokens.is_contiguous() else queries.tokens.contiguous()
    with torch.cuda.device(dev):
        candidates, m, ld_cand, out, ids, ws = _rerank_args(n_q, dev, candidates, out, lambda m: ws_bytes(n_q, m, n))
        rcode = entry(_lib.dtype_code(rc.dtype), _lib.ptr(tokens), _lib.ptr(queries.offsets), queries.offsets_host.data_ptr(), n_q,
                      _lib.ptr(rc.codes), _lib.ptr(rc.residuals), _lib.ptr(rc.centroids), rc.n_centroids, _lib.ptr(rc.weights), rc.bits,
                      _lib.ptr(rc.offsets), _lib.ptr(rc.clamp0), n, int(rc.codes.shape[0]), kind.WIDTH, _lib.ptr(candidates), m, ld_cand,
                      int(rc.id_base), _lib.ptr(out), max(m, 1), _lib.ptr(ids), _lib.ptr(ws), _lib.current_stream_handle(dev))
    _lib.check(rcode, kind._CANDIDATES)
    return out, ids


def residual_align(queries, rc: ResidualCorpus, ids: torch.Tensor, *, maps: bool = False, max_rows: Optional[int] = None):
    """`align` over the compressed shard (include/maxsim.h: msim_res_align_candidates): the `Alignment` of every entry (q, j) of `ids`
    (int64 [n_q, m] GLOBAL ids on the shard's device, -1 = none), with the signature, the query forms and the checks of `align`.
    best_sim, best_row, ids and sims have the bits `align(queries, rc.decompress(), ids, maps=, max_rows=)` gives: every listed page
    is decoded chunk by chunk in the registers of the kernel that multiplies it, and no decoded row is written to memory.
    bfloat16 / float16, width 128, queries of at most 128 tokens (NotImplementedError otherwise; RuntimeError when queries and
    shard differ in dtype; ValueError for ids of the wrong shape, dtype or device).  `max_rows` bounds the rows of a listed page
    (default: the shard's longest page, known on the host); a longer page comes back NaN / -1.  Asynchronous on torch's current
    stream; with a `PackedQueries` there is no host synchronisation and the call is hipGraph-capturable.
    What can be refused without the device is refused before it is asked for: the formats and `max_rows` always, the token count
    and `ids` for queries that come packed."""
    return _align_rows(queries, rc, ids, maps, max_rows, ResidualCorpus, "residual_align")


def _align_rows(queries, rc, ids: torch.Tensor, maps: bool, max_rows: Optional[int], kind, who: str):
    """`align` over the compressed shard of both widths: the entry of `kind` over a shard of that class"""
    from .align import MAX_QUERY_TOKENS, Alignment, resolve_ids          # align dispatches here

    _require_kind(rc, kind, who)
    _check_query_format(queries, rc, "align")
    n = len(rc)
    if max_rows is None:
        max_rows = int(rc.lengths.max()) if n else 0
    max_rows = int(max_rows)
    if max_rows < 0:
        raise ValueError(f"max_rows={max_rows} is negative")
    if not isinstance(queries, PackedQueries):                           # packing is device work
        queries = _as_packed(queries, _require_gpu(rc.device), layout="flat")
    if queries.device != rc.device:
        raise ValueError("queries and corpus live on different devices")
    n_q = len(queries)
    ids, m, ld = _id_list(ids, n_q, rc.device, "ids")
    q_lens = queries.lengths.to(torch.int64)
    T = int(q_lens.max()) if n_q else 0
    if T > MAX_QUERY_TOKENS:
        raise NotImplementedError(f"align takes queries of at most {MAX_QUERY_TOKENS} tokens (got one of {T})")
    dev = _require_gpu(rc.device)
    best_sim = torch.empty((n_q, m, T), dtype=torch.float32, device=dev)
    best_row = torch.empty((n_q, m, T), dtype=torch.int32, device=dev)
    sims = torch.empty((n_q, m, T, max_rows), dtype=torch.float32, device=dev) if maps else None
    tokens = queries.tokens if queries.tokens.is_contiguous() else queries.tokens.contiguous()
    with torch.cuda.device(dev):
        rcode = getattr(_lib.lib(), kind._ALIGN)(
            _lib.dtype_code(rc.dtype), _lib.ptr(tokens), _lib.ptr(queries.offsets), n_q, int(tokens.shape[0]), T, _lib.ptr(rc.codes),
            _lib.ptr(rc.residuals), _lib.ptr(rc.centroids), rc.n_centroids, _lib.ptr(rc.weights), rc.bits, _lib.ptr(rc.offsets),
            _lib.ptr(rc.clamp0), n, int(rc.codes.shape[0]), kind.WIDTH, _lib.ptr(ids), m, ld, int(rc.id_base), _lib.ptr(best_sim),
            _lib.ptr(best_row), _lib.ptr(sims), max_rows, _lib.current_stream_handle(dev))
    _lib.check(rcode, kind._ALIGN)
    return Alignment(best_sim, best_row, resolve_ids(ids, int(rc.id_base), n), sims, q_lens, page_lengths=rc.lengths,
                     id_base=int(rc.id_base))


def residual_gather_pages(rc: ResidualCorpus, ids: torch.Tensor, pad_to: Optional[int] = None,
                          out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`gather_pages` over the compressed shard (include/maxsim.h: msim_res_gather_pages): (box [*ids.shape, L_pad, 128] of the
    shard's dtype, lengths int32 [*ids.shape]) with the bytes `gather_pages(rc.decompress(), ids, pad_to)` gives -- the listed pages
    are decoded straight into the box, so `mine_hard_negatives(q, rc, ...)` -> `gather_pages(rc, neg_ids)` feeds the
    explicit-negative losses without a decoded shard.  ids: int64 GLOBAL ids of any shape; L_pad = `pad_to`, or the shard's longest
    page.  Rows past a page's length, and the whole page for id -1 or an id outside the shard, are exactly zero and `lengths` is 0
    for such a slot.  A page longer than `pad_to`: host ids raise ValueError, device ids TRUNCATE (`lengths` reports the truncated
    count), as `gather_pages`.  out: a contiguous [*ids.shape, L_pad, 128] tensor to write into (every byte of it is written).
    Asynchronous on torch's current stream; with device ids there is no host synchronisation and the call is hipGraph-capturable."""
    return _gather_rows(rc, ids, pad_to, out, ResidualCorpus, "residual_gather_pages")


def _gather_rows(rc, ids: torch.Tensor, pad_to: Optional[int], out: Optional[torch.Tensor], kind,
                 who: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """`gather_pages` over the compressed shard of both widths: the entry of `kind` over a shard of that class"""
    _require_kind(rc, kind, who)
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
        raise ValueError("ids must be an int64 tensor")
    n = len(rc)
    if pad_to is None:
        pad_to = int(rc.lengths.max()) if n else 0
    pad_to = int(pad_to)
    if pad_to < 0:
        raise ValueError(f"pad_to={pad_to} is negative")
    if ids.device.type == "cpu":
        idx = ids.reshape(-1).numpy() - int(rc.id_base)
        inside = idx[(ids.reshape(-1).numpy() >= 0) & (idx >= 0) & (idx < n)]
        lens = rc.lengths.numpy()[inside]
        if lens.size and int(lens.max()) > pad_to:
            bad = int(inside[int(np.argmax(lens))]) + int(rc.id_base)
            raise ValueError(f"page {bad} has {int(lens.max())} rows, pad_to={pad_to}")
    elif ids.device != rc.device:
        raise ValueError("ids and corpus live on different devices")
    dev = _require_gpu(rc.device)
    flat = ids.to(dev).reshape(-1).contiguous()
    shape = tuple(ids.shape) + (pad_to, kind.WIDTH)
    if out is None:
        out = torch.empty(shape, dtype=rc.dtype, device=dev)
    elif out.shape != shape or out.dtype != rc.dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {rc.dtype} tensor of shape {shape} on {dev}")
    lengths = torch.empty(tuple(ids.shape), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rcode = getattr(_lib.lib(), kind._GATHER)(_lib.dtype_code(rc.dtype), _lib.ptr(rc.codes), _lib.ptr(rc.residuals),
                                                  _lib.ptr(rc.centroids), rc.n_centroids, _lib.ptr(rc.weights), rc.bits, kind.WIDTH,
                                                  int(rc.codes.shape[0]), _lib.ptr(rc.offsets), n, int(rc.id_base), _lib.ptr(flat),
                                                  flat.numel(), pad_to, _lib.ptr(out), _lib.ptr(lengths),
                                                  _lib.current_stream_handle(dev))
    _lib.check(rcode, kind._GATHER)
    return out, lengths
