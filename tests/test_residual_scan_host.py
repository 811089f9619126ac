"""The full scan of a residual-compressed shard without a GPU: the refusals of msim_res_scores before any device work, the header
and the binding, and the retriever's routing over a host `ResidualCorpus` with injected stand-ins for the kernels -- the default
retriever keeps refusing, `score_fn=` opens the full scan, `filter=`, `group_by=` and `mine`, `align` raises either way."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_filter_host import _filter
from tests.test_group_host import Hooks as GroupHooks
from tests.test_mine_host import _bounds_fn, _mask_fn, _page, _score_fn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CPU = torch.device("cpu")
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _scan_call(L, dtype=0, qt=FAKE, q_off=FAKE, q_off_host=None, n_q=2, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, d_off=FAKE,
               n_d=10, d_rows=100, dim=128, out=FAKE, ld=10, ws=FAKE):
    oh = np.array([0, 3, 7], dtype=np.int32) if q_off_host is None else np.asarray(q_off_host, dtype=np.int32)
    return L.msim_res_scores(dtype, qt, q_off, oh.ctypes.data, n_q, codes, res, C, K, w, bits, d_off, None, n_d, d_rows, dim, out, ld, ws, None)


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    ws = L.msim_res_scores_workspace_bytes
    assert ws(0, 10) == 0 and ws(-1, 10) == 0 and ws(3, 0) == 0 and ws(3, -5) == 0
    for n_q in (1, 2, 7, 1000):
        assert ws(n_q, 10) > 0 and ws(n_q, 10) % 16 == 0
        assert ws(n_q, 10) == ws(n_q, 125000) == ws(n_q, 2**31 - 1)             # a function of n_q alone: there is no row count to pass
    assert _scan_call(L, n_q=0) == 0 and _scan_call(L, n_d=0) == 0              # nothing to do: no pointer is looked at
    assert _scan_call(L, n_q=0, qt=None, out=None, ws=None, K=100, bits=3) == 0
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(d_rows=-1), dict(qt=None), dict(q_off=None), dict(d_off=None), dict(out=None),
               dict(ws=None), dict(codes=None), dict(res=None), dict(C=None), dict(w=None), dict(qt=FAKE + 8), dict(res=FAKE + 8),
               dict(C=FAKE + 2), dict(ws=FAKE + 4), dict(codes=FAKE + 1), dict(w=FAKE + 2), dict(q_off=FAKE + 2), dict(d_off=FAKE + 2),
               dict(out=FAKE + 2), dict(ld=9), dict(q_off_host=[1, 3, 7]), dict(q_off_host=[0, 5, 3]), dict(K=100), dict(K=4096)):
        assert _scan_call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=320), dict(dim=64), dict(bits=1), dict(bits=3), dict(bits=8),
               dict(q_off_host=[0, 3, 3 + 129]), dict(d_rows=1 << 31)):
        assert _scan_call(L, **kw) == EUNSUPPORTED, kw


def test_header_and_binding():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"\bsize_t\s+msim_res_scores_workspace_bytes\s*\(\s*int n_q,\s*int n_d\s*\)\s*;", header)
    assert re.search(r"\bint\s+msim_res_scores\s*\(", header)
    text = " ".join(header.split())
    for phrase in ("exactly the bits msim_fwd_ragged (flags 0) gives the same query against the page decoded by msim_res_decode_rows",
                   "the bits do not depend on which queries share a wave", "a function of n_q alone"):
        assert phrase in text.replace(" * ", " "), phrase
    L = colpali_amd._lib.lib()
    assert L.msim_res_scores.argtypes is not None and len(L.msim_res_scores.argtypes) == 20
    assert L.msim_res_scores_workspace_bytes.restype is not None
    assert L.msim_abi_version() == 22 == colpali_amd._lib.ABI_VERSION
    assert callable(colpali_amd.residual_scores) and "residual_scores" in colpali_amd.__all__


# ------------------------------------------------------------------------------------------------------------------ routing
def _shards(seed=0, n=23, n_q=4, id_base=100):
    """a host PackedCorpus and a host ResidualCorpus over the same pages (same count, lengths and id_base; the codes are never read)"""
    import colpali_amd as amd

    g = torch.Generator().manual_seed(seed)
    pages = [_page(g, int(k)) for k in torch.randint(1, 9, (n,), generator=g)]
    pages[7] = pages[3].clone()                                          # an exact tie
    pages[5] = pages[5][:0]                                              # a page of 0 rows
    packed = amd.pack_passages(pages, CPU, batch_size=None, id_base=id_base)
    rows = int(packed.lengths.sum())
    rc = amd.ResidualCorpus(centroids=torch.zeros(256, 128, dtype=torch.bfloat16), codes=torch.zeros(rows, dtype=torch.int16).view(torch.uint16),
                            residuals=torch.zeros(rows, 32, dtype=torch.uint8), cutoffs=torch.zeros(3), weights=torch.zeros(4),
                            offsets=packed.offsets.clone(), clamp0=None, lengths=packed.lengths.clone(), id_base=id_base, bits=2)
    q = torch.stack([_page(g, 6) for _ in range(n_q)])
    labels = torch.randint(0, 6, (n,), generator=g) * 3 + 2
    return amd, g, packed, rc, q, labels


class Stubs(GroupHooks):
    """the filter and group stand-ins, plus a scorer and a rerank that answer for the residual shard with the packed pages' scores"""

    def __init__(self, packed, rc):
        super().__init__()
        self.packed, self.rc = packed, rc
        self.scored = 0

    def score(self, queries, shard):
        assert shard is self.rc or shard is self.packed
        self.scored += shard is self.rc
        return _score_fn(queries, self.packed)

    def rerank_rc(self, queries, shard, candidates):
        assert shard is self.rc or shard is self.packed
        return self.rerank(queries, self.packed, candidates)

    def kw(self):
        return dict(super().kw(), score_fn=self.score, rerank_fn=self.rerank_rc, mine_bounds_fn=_bounds_fn, mine_mask_fn=_mask_fn)


def _same(got, want, what):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg=what)


def test_the_default_retriever_keeps_refusing():
    amd, g, packed, rc, q, labels = _shards()
    r = amd.ShardedRetriever(rc)
    groups = amd.PageGroups.from_labels(labels, 100)
    pos = torch.tensor([100, 101, -1, 103])
    cand = torch.zeros((len(q), 2), dtype=torch.int64)
    for call in (lambda: r.search(q, k=2), lambda: r.search(q, k=2, filter=object()), lambda: r.search(q, k=2, group_by=groups),
                 lambda: r.search(q, k=2, candidates=cand, filter=object()), lambda: r.search(q, k=2, prefilter=rc.index, n_candidates=2, group_by=groups),
                 lambda: r.align(q, cand), lambda: r.mine(q, pos, 2)):
        with pytest.raises(NotImplementedError, match="ResidualCorpus") as e:
            call()
        assert "score_fn=residual_scores" in str(e.value)               # the message names the opt-in


def test_an_injected_scorer_opens_the_routes_that_need_the_score_matrix():
    amd, g, packed, rc, q, labels = _shards()
    n, n_q = len(rc), len(q)
    h = Stubs(packed, rc)
    r, ref = amd.ShardedRetriever(rc, **h.kw()), amd.ShardedRetriever(packed, **h.kw())
    for k in (1, 4, n + 3):
        _same(r.search(q, k), ref.search(q, k), f"scan k={k}")
    assert h.scored == 3
    rng = np.random.default_rng(3)
    shared = rng.random(n) < 0.4
    shared[[3, 5, 7]] = True
    per = rng.random((n_q, n)) < 0.4
    per[1] = False
    lab = (rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 4, n_q).astype(np.int32))
    groups = amd.PageGroups.from_labels(labels, 100)
    cand = torch.stack([torch.randperm(n + 6, generator=g)[:12] + 97 for _ in range(n_q)])
    for spec in (("shared", shared), ("per_query", per), ("labels", *lab)):
        for route in ("mask", "list", "auto"):
            _same(r.search(q, 5, filter=_filter(amd, spec, 100), filter_route=route),
                  ref.search(q, 5, filter=_filter(amd, spec, 100), filter_route=route), f"{spec[0]} {route}")
            _same(r.search(q, 5, filter=_filter(amd, spec, 100), filter_route=route, group_by=groups),
                  ref.search(q, 5, filter=_filter(amd, spec, 100), filter_route=route, group_by=groups), f"{spec[0]} {route} grouped")
        _same(r.search(q, 5, filter=_filter(amd, spec, 100), candidates=cand), ref.search(q, 5, filter=_filter(amd, spec, 100), candidates=cand),
              f"{spec[0]} candidates")
    assert h.calls["mask"] >= 3 and h.calls["list"] >= 3 and h.calls["ids"] >= 3
    # the list route asks the shard for its format: a residual shard is its centroids' dtype at width 128
    assert (rc.dtype, rc.width) == (torch.bfloat16, 128) and r._list_formats_fit(q) and not r._list_formats_fit(q.float())
    with pytest.raises(NotImplementedError, match="bfloat16 of width 128"):
        r.search(q.float(), 5, filter=_filter(amd, ("shared", shared), 100), filter_route="list")
    _same(r.search(q, 4, group_by=groups), ref.search(q, 4, group_by=groups), "grouped scan")
    _same(r.search(q, 4, candidates=cand, group_by=groups), ref.search(q, 4, candidates=cand, group_by=groups), "grouped candidates")
    pos = torch.tensor([[100, 103], [101, -1], [-1, -1], [107, 122]])
    for kw in (dict(), dict(max_ratio=0.95), dict(skip_top=2)):
        _same(r.mine(q, pos, 3, **kw), ref.mine(q, pos, 3, **kw), f"mine {kw}")
    with pytest.raises(NotImplementedError, match="ResidualCorpus"):        # align returns rows: it raises either way
        r.align(q, cand)
    # the retriever packs for residual_scores as it packs for its own scan (a host list of CPU tensors: the packer refuses, no GPU here)
    assert amd.ShardedRetriever(rc, score_fn=amd.residual_scores)._score is amd.residual_scores
    with pytest.raises(RuntimeError):
        amd.residual_scores(q, rc)
    with pytest.raises(ValueError):
        amd.residual_scores(q, rc.index)
