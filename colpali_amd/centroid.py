"""A centroid-code index (PLAID's first stage): a first stage for two-stage search that reads 2 bytes per corpus row.

`CentroidIndex.build` stores every row of a resident `PackedCorpus` as the uint16 id of its nearest of K centroids (trained by
`train_centroids`, spherical k-means on a sample, or handed in).  `centroid_scores` computes the query-centroid similarities
S = Q . C^T once per query as an fp16 table and scores every page as sum_i max_j S[i, code_j] by table lookups from LDS
(include/maxsim.h: msim_cent_*, colpali_amd/csrc/centroid_index.hip): no corpus row is read, no MFMA runs over the corpus.  Its top
`n_candidates` are reranked exactly by `rerank` -- `ShardedRetriever.search(prefilter=index, n_candidates=m)` -- so every returned
score is the exact one.  The bf16 corpus stays as it is: the index is an extra, opt-in copy of 1/128 of its size.

The host layer is one for both row widths: `_CentroidCodes` holds everything that does not depend on the width, and a public class
binds the width and the two entries that read rows of it (encode and table; the scan reads the table and the codes alone and is the
same call for both).  `CentroidIndex` is width 128; `CentroidWideIndex` (colpali_amd/residual_wide.py) is width 320.  The two are
siblings, not parent and child: a function that takes one refuses the other by its type.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .corpus import PackedCorpus, PackedQueries, _as_packed
from .scoring import _require_gpu

DIM = 128
MIN_CENTROIDS, MAX_CENTROIDS = 256, 2048
MAX_Q_TOKENS = 128


def _check_format(dtype: torch.dtype, width: int, what: str, dim: int = DIM) -> None:
    if dtype not in (torch.bfloat16, torch.float16) or width != dim:
        raise NotImplementedError(f"the centroid index takes bfloat16 / float16 {what} of width {dim} (got {dtype}, width {width})")


def _check_k(k: int) -> int:
    k = int(k)
    if k < MIN_CENTROIDS or k > MAX_CENTROIDS or k % 256:
        raise ValueError(f"n_centroids must be a multiple of 256 from {MIN_CENTROIDS} to {MAX_CENTROIDS} (got {k})")
    return k


def _check_centroids(centroids: torch.Tensor, dim: int = DIM) -> None:
    if centroids.dim() != 2 or not centroids.is_contiguous():
        raise ValueError(f"centroids must be a contiguous [K, {dim}] tensor")
    _check_format(centroids.dtype, int(centroids.shape[1]), "centroids", dim)
    _check_k(centroids.shape[0])


class _CentroidCodes:
    """What the centroid-code indexes of both widths are: `centroids` [K, WIDTH] (bf16 / f16, K a multiple of 256 in 256 .. 2048),
    `codes` uint16 [rows] in the corpus's row order, the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n] or
    None), copied; `lengths` (int64 [n], host) and `id_base` as the corpus's.  A subclass sets WIDTH and the names of the two
    library entries that read rows of that width."""

    WIDTH: int = 0
    _ENCODE: str = ""
    _TABLE: str = ""

    def __init__(self, centroids: torch.Tensor, codes: torch.Tensor, offsets: torch.Tensor, clamp0: Optional[torch.Tensor],
                 lengths: torch.Tensor, id_base: int = 0):
        n = int(lengths.numel())
        _check_centroids(centroids, self.WIDTH)
        if codes.dtype != torch.uint16 or codes.dim() != 1 or not codes.is_contiguous():
            raise ValueError("codes must be a contiguous uint16 [rows] tensor")
        if offsets.shape != (n + 1,) or offsets.dtype != torch.int32:
            raise ValueError(f"offsets must be int32 [{n + 1}]")
        if clamp0 is not None and (clamp0.dtype != torch.uint8 or clamp0.shape != (n,)):
            raise ValueError(f"clamp0 must be uint8 [{n}] or None")
        self.centroids, self.codes, self.offsets, self.clamp0 = centroids, codes, offsets, clamp0
        self.lengths, self.id_base = lengths, int(id_base)

    def __len__(self) -> int:
        return int(self.lengths.numel())

    @property
    def n_centroids(self) -> int:
        return int(self.centroids.shape[0])

    @property
    def device(self) -> torch.device:
        return self.codes.device

    @property
    def nbytes(self) -> int:
        n = sum(t.numel() * t.element_size() for t in (self.centroids, self.codes, self.offsets))
        return n + (self.clamp0.numel() if self.clamp0 is not None else 0)

    @classmethod
    def build(cls, corpus: PackedCorpus, centroids: Optional[torch.Tensor] = None, n_centroids: int = 1024, iters: int = 8,
              sample_rows: int = 1 << 18, seed: int = 0, chunk_docs: int = 65536):
        """Encode every page of `corpus` (bf16 / f16, the class's width), `chunk_docs` pages per launch, straight into the index.
        `centroids=None` trains them first (spherical k-means with the index's own encode kernel: `n_centroids`, `iters`,
        `sample_rows`, `seed`); given centroids (in the corpus dtype) the build is bit-reproducible.  Asynchronous on torch's current
        stream."""
        if chunk_docs < 1:
            raise ValueError("chunk_docs must be >= 1")
        dev = _require_gpu(corpus.device)
        _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages", cls.WIDTH)
        if centroids is None:
            centroids = _train(cls, corpus, n_centroids, iters, sample_rows, seed)
        _check_centroids(centroids, cls.WIDTH)
        if centroids.dtype != corpus.blob.dtype or centroids.device != dev:
            raise ValueError(f"centroids must be {corpus.blob.dtype} on {dev}")
        codes = _encode_rows(cls, corpus.blob, corpus.offsets, corpus.lengths, centroids, chunk_docs)
        clamp0 = corpus.clamp0.clone() if corpus.clamp0 is not None else None
        return cls(centroids, codes, corpus.offsets.clone(), clamp0, corpus.lengths.clone(), corpus.id_base)

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


class CentroidIndex(_CentroidCodes):
    """The centroid-code copy of one resident shard: `centroids` [K, 128] (bf16 / f16, K a multiple of 256 in 256 .. 2048), `codes`
    uint16 [rows] in the corpus's row order, the corpus's page `offsets` (int32 [n + 1], device) and `clamp0` (uint8 [n] or None),
    copied; `lengths` (int64 [n], host) and `id_base` as the corpus's."""

    WIDTH = DIM
    _ENCODE = "msim_cent_encode_docs"
    _TABLE = "msim_cent_table"


def _encode_rows(kind, blob: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, centroids: torch.Tensor,
                 chunk_docs: int = 65536) -> torch.Tensor:
    """uint16 [rows]: the nearest centroid (the encode entry of `kind`) of every row of the pages `offsets` cuts out of `blob`"""
    dev = _require_gpu(blob.device)
    n, rows = int(lengths.numel()), int(blob.shape[0])
    codes = torch.zeros((rows,), dtype=torch.int16, device=dev).view(torch.uint16)      # (uint16 has few device kernels of its own)
    blob = blob if blob.is_contiguous() else blob.contiguous()
    entry = getattr(_lib.lib(), kind._ENCODE)
    with torch.cuda.device(dev):
        for lo in range(0, n, chunk_docs):
            hi = min(n, lo + chunk_docs)
            longest = int(lengths[lo:hi].max())
            rc = entry(_lib.dtype_code(blob.dtype), _lib.ptr(blob), _lib.ptr(offsets[lo:]), hi - lo, rows, kind.WIDTH, longest,
                       _lib.ptr(centroids), int(centroids.shape[0]), _lib.ptr(codes), None, _lib.current_stream_handle(dev))
            _lib.check(rc, kind._ENCODE)
    return codes


def encode_rows(blob: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, centroids: torch.Tensor,
                chunk_docs: int = 65536) -> torch.Tensor:
    """uint16 [rows]: the nearest centroid (msim_cent_encode_docs) of every row of the pages `offsets` (int32 [n + 1], device)
    cuts out of `blob` [rows, 128]; `lengths`: their row counts on the host (int64 [n])."""
    return _encode_rows(CentroidIndex, blob, offsets, lengths, centroids, chunk_docs)


def _train(kind, corpus: PackedCorpus, n_centroids: int, iters: int, sample_rows: int, seed: int) -> torch.Tensor:
    k = _check_k(n_centroids)
    if iters < 0 or sample_rows < 1:
        raise ValueError("iters must be >= 0 and sample_rows >= 1")
    dev = _require_gpu(corpus.device)
    _check_format(corpus.blob.dtype, int(corpus.blob.shape[1]), "pages", kind.WIDTH)
    rows = int(corpus.blob.shape[0])
    if rows < k:
        raise ValueError(f"{rows} corpus rows cannot seed {k} centroids")
    g = torch.Generator().manual_seed(int(seed))
    n_s = max(min(int(sample_rows), rows), k)
    if rows <= 1 << 24:
        pick = torch.randperm(rows, generator=g)[:n_s]                  # the first k of the sample are the initial centroids
    else:                                                               # a permutation of a big shard costs seconds: draw with replacement
        pick = torch.randint(0, rows, (n_s,), generator=g)
    sample = corpus.blob.index_select(0, pick.to(dev)).contiguous()
    centroids = sample[:k].clone()
    one_page = torch.tensor([0, n_s], dtype=torch.int32, device=dev)
    one_len = torch.tensor([n_s], dtype=torch.int64)
    rows32 = sample.float()
    for _ in range(int(iters)):
        codes = _encode_rows(kind, sample, one_page, one_len, centroids).view(torch.int16).to(torch.int64) & 0xFFFF
        sums = torch.zeros((k, kind.WIDTH), dtype=torch.float32, device=dev).index_add_(0, codes, rows32)
        counts = torch.bincount(codes, minlength=k)
        mean = torch.nn.functional.normalize(sums / counts.clamp(min=1).unsqueeze(1), dim=-1)
        keep = (counts == 0) | (sums.norm(dim=-1) == 0)
        centroids = torch.where(keep.unsqueeze(1), centroids, mean.to(centroids.dtype))
    return centroids.contiguous()


def train_centroids(corpus: PackedCorpus, n_centroids: int = 1024, iters: int = 8, sample_rows: int = 1 << 18,
                    seed: int = 0) -> torch.Tensor:
    """Spherical k-means on a seeded sample of the corpus's rows: [n_centroids, 128] unit rows in the corpus dtype.  The initial
    centroids are sampled rows (`iters=0` returns them); every iteration assigns the sample with the index's own encode kernel and
    replaces each centroid by the fp32 mean of its cluster, L2-normalised and cast to the corpus dtype (an empty cluster keeps its
    centroid).  The update is plain torch: this is build time, not the scoring path."""
    return _train(CentroidIndex, corpus, n_centroids, iters, sample_rows, seed)


def _prepare(queries, index: _CentroidCodes) -> Tuple[PackedQueries, int]:
    dev = _require_gpu(index.device)
    dim = index.WIDTH
    if isinstance(queries, torch.Tensor):
        _check_format(queries.dtype, int(queries.shape[-1]), "queries", dim)
    elif not isinstance(queries, PackedQueries):
        for x in queries:
            _check_format(x.dtype, int(x.shape[-1]), "queries", dim)
    q = _as_packed(queries, dev, layout="flat")
    _check_format(q.dtype, int(q.tokens.shape[1]), "queries", dim)
    if q.device != dev:
        raise ValueError("queries and index live on different devices")
    if q.dtype != index.centroids.dtype:
        raise ValueError(f"queries are {q.dtype}, the index's centroids {index.centroids.dtype}")
    lens = q.lengths
    max_q = int(lens.max()) if lens.numel() else 0
    if max_q > MAX_Q_TOKENS:
        raise NotImplementedError(f"the centroid index scores queries of up to {MAX_Q_TOKENS} tokens (got {max_q})")
    return q, max_q


def _require_kind(index, kind, who: str) -> None:
    """the sibling classes refuse each other by type: no kernel of one width ever sees rows of the other"""
    if isinstance(index, _CentroidCodes) and not isinstance(index, kind):
        raise NotImplementedError(f"{who} takes a {kind.__name__} (width {kind.WIDTH}); got a {type(index).__name__} of width "
                                  f"{index.WIDTH}")


def scores_plan(queries, index: CentroidIndex) -> Tuple[int, int, int, int]:
    """The launch plan `centroid_scores` uses for these queries (msim_cent_scores_plan): (32-token blocks per query, pages per wave,
    waves per workgroup, workgroups)."""
    import ctypes

    q, max_q = _prepare(queries, index)
    plan = (ctypes.c_int32 * 4)()
    with torch.cuda.device(index.device):
        rc = _lib.lib().msim_cent_scores_plan(int(q.offsets.numel()) - 1, max_q, index.n_centroids, len(index), int(index.codes.shape[0]),
                                              plan)
    _lib.check(rc, "msim_cent_scores_plan")
    return tuple(int(x) for x in plan)


def _scores(queries, index: _CentroidCodes, out: Optional[torch.Tensor]) -> torch.Tensor:
    q, max_q = _prepare(queries, index)
    dev = index.device
    n_q, n, k = int(q.offsets.numel()) - 1, len(index), index.n_centroids
    if out is None:
        out = torch.empty((n_q, n), dtype=torch.float32, device=dev)
    elif out.shape != (n_q, n) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous fp32 [{n_q}, {n}] tensor on {dev}")
    tokens = q.tokens if q.tokens.is_contiguous() else q.tokens.contiguous()
    L = _lib.lib()
    table = torch.empty((max(int(L.msim_cent_table_bytes(n_q, max_q, k)), 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = _lib.current_stream_handle(dev)
        rc = getattr(L, index._TABLE)(_lib.dtype_code(q.dtype), _lib.ptr(tokens), _lib.ptr(q.offsets), n_q, int(tokens.shape[0]), max_q,
                                      index.WIDTH, _lib.ptr(index.centroids), k, _lib.ptr(table), st)
        _lib.check(rc, index._TABLE)
        rc = L.msim_cent_scores(_lib.ptr(table), _lib.ptr(q.offsets), n_q, int(tokens.shape[0]), max_q, k, _lib.ptr(index.codes),
                                _lib.ptr(index.offsets), _lib.ptr(index.clamp0), n, int(index.codes.shape[0]), _lib.ptr(out), max(n, 1),
                                st)
        _lib.check(rc, "msim_cent_scores")
    return out


def centroid_scores(queries, index: CentroidIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Centroid-interaction scores of every query against every page of the index: fp32 [n_q, len(index)], column j = page
    index.id_base + j.  A score's bits depend on its query, the centroids and the page's codes only.  Asynchronous on torch's current
    stream.  Given a `PackedQueries` it never synchronises with the host and is hipGraph-capturable: its only allocations are torch
    tensors (the fp16 table, n_q * ceil(longest query / 32) * K * 64 bytes, and `out` when it is None), made on the current stream
    before the library calls."""
    _require_kind(index, CentroidIndex, "centroid_scores")
    return _scores(queries, index, out)
