"""The full scan of a residual-compressed 320-wide shard without a GPU: the refusals of msim_res_wide_scores before any device work,
the header and the binding, and the retriever's routing over a host `ResidualWideCorpus` with injected stand-ins for the kernels --
the default retriever keeps refusing and names the opt-in, `score_fn=` opens the full scan, `filter=`, `group_by=` and `mine`,
`align` raises either way, and the sibling classes refuse each other's scan by type."""
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
W = 320
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _scan_call(L, dtype=0, qt=FAKE, q_off=FAKE, q_off_host=None, n_q=2, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, d_off=FAKE,
               n_d=10, d_rows=100, dim=W, out=FAKE, ld=10, ws=FAKE):
    oh = np.array([0, 3, 7], dtype=np.int32) if q_off_host is None else np.asarray(q_off_host, dtype=np.int32)
    return L.msim_res_wide_scores(dtype, qt, q_off, oh.ctypes.data, n_q, codes, res, C, K, w, bits, d_off, None, n_d, d_rows, dim, out, ld, ws,
                                  None)


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    ws = L.msim_res_wide_scores_workspace_bytes
    assert ws(0, 10) == 0 and ws(-1, 10) == 0 and ws(3, 0) == 0 and ws(3, -5) == 0
    for n_q in (1, 2, 7, 1000):
        assert ws(n_q, 10) == (16 + 16 * n_q + 15) // 16 * 16
        assert ws(n_q, 10) == ws(n_q, 125000) == ws(n_q, 2**31 - 1)             # a function of n_q alone: there is no row count to pass
        assert ws(n_q, 10) == L.msim_res_scores_workspace_bytes(n_q, 10)        # the group table does not depend on the row width

    def refused(code, words, **kw):
        assert _scan_call(L, **kw) == code, kw
        msg = L.msim_last_error().decode()
        assert "msim_res_wide_scores" in msg and words in msg, (kw, msg)

    assert _scan_call(L, n_q=0) == OK and _scan_call(L, n_d=0) == OK            # nothing to do: no pointer is looked at
    assert _scan_call(L, n_q=0, qt=None, out=None, ws=None, K=100, bits=3, dim=128) == OK
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(d_rows=-1)):
        refused(EINVAL, "negative size", **kw)
    assert _scan_call(L, n_q=-1, dim=128, K=100) == EINVAL                      # a negative size comes before the format
    for kw in (dict(dim=128), dict(dim=64), dict(dim=0)):
        refused(EUNSUPPORTED, "width", **kw)
    for kw in (dict(dtype=2), dict(dtype=7)):
        refused(EUNSUPPORTED, "bfloat16 / float16", **kw)
    for kw in (dict(K=100), dict(K=0), dict(K=2304), dict(K=4096)):
        refused(EINVAL, "multiple of 256", **kw)
    for kw in (dict(bits=1), dict(bits=3), dict(bits=8)):
        refused(EUNSUPPORTED, "residual bits", **kw)
    assert _scan_call(L, dim=128, qt=None) == EUNSUPPORTED                      # the format comes before the pointers
    for kw in (dict(qt=None), dict(q_off=None), dict(d_off=None), dict(out=None), dict(ws=None), dict(codes=None), dict(res=None),
               dict(C=None), dict(w=None)):
        refused(EINVAL, "null pointer", **kw)
    refused(EINVAL, "ld_scores", codes=None, res=None, d_rows=0, ld=9)          # (a shard without rows has no rows to point at)
    for kw in (dict(qt=FAKE + 8), dict(res=FAKE + 8), dict(C=FAKE + 2), dict(ws=FAKE + 4), dict(codes=FAKE + 1), dict(w=FAKE + 2),
               dict(q_off=FAKE + 2), dict(d_off=FAKE + 2), dict(out=FAKE + 2)):
        refused(EINVAL, "aligned", **kw)
    refused(EINVAL, "ld_scores=9 < n_d=10", ld=9)
    refused(EUNSUPPORTED, "32-bit page offsets", d_rows=1 << 31)
    refused(EINVAL, "q_off[0] must be 0", q_off_host=[1, 3, 7])
    refused(EINVAL, "non-decreasing", q_off_host=[0, 5, 3])
    assert _scan_call(L, q_off_host=[0, 3, 3 + 129]) == EUNSUPPORTED
    assert "129 tokens" in L.msim_last_error().decode() and "at most 128" in L.msim_last_error().decode()
    assert _scan_call(L, q_off_host=[0, 3, 3 + 129], ld=9) == EINVAL            # ld_scores comes before the offsets
    # msim_res_scores keeps refusing the wide rows
    assert L.msim_res_scores(0, FAKE, FAKE, np.array([0, 3, 7], dtype=np.int32).ctypes.data, 2, FAKE, FAKE, FAKE, 256, FAKE, 2, FAKE, None, 10,
                             100, W, FAKE, 10, FAKE, None) == EUNSUPPORTED


def test_header_and_binding():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"\bsize_t\s+msim_res_wide_scores_workspace_bytes\s*\(\s*int n_q,\s*int n_d\s*\)\s*;", header)
    m = re.search(r"\bint\s+msim_res_wide_scores\s*\(([^;]*)\)\s*;", header)
    narrow = re.search(r"\bint\s+msim_res_scores\s*\(([^;]*)\)\s*;", header)
    assert m and narrow and " ".join(m.group(1).split()) == " ".join(narrow.group(1).split())      # the 20 arguments, in that order
    assert len(m.group(1).split(",")) == 20
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    text = " ".join(header.split()).replace(" * ", " ")
    for phrase in ("exactly the bits msim_res_wide_candidates gives the same query against page c",
                   "the bits do not depend on which queries share a wave", "a function of n_q alone", "K1sP", "K1bPF",
                   "|delta| <= 2 gamma(L - 1) sum_i |M_i|"):
        assert phrase in text, phrase
    L = colpali_amd._lib.lib()
    assert L.msim_res_wide_scores.argtypes is not None and len(L.msim_res_wide_scores.argtypes) == 20
    assert list(L.msim_res_wide_scores.argtypes) == list(L.msim_res_scores.argtypes)
    assert L.msim_res_wide_scores_workspace_bytes.restype is not None and len(L.msim_res_wide_scores_workspace_bytes.argtypes) == 2
    assert L.msim_abi_version() == 22 == colpali_amd._lib.ABI_VERSION
    assert callable(colpali_amd.residual_wide_scores) and "residual_wide_scores" in colpali_amd.__all__
    assert "residual_wide_scores" in colpali_amd.__doc__ and "residual_wide_scores" in colpali_amd.residual_wide.__doc__
    assert colpali_amd.ResidualWideCorpus._SCORES == "msim_res_wide_scores" and colpali_amd.ResidualCorpus._SCORES == "msim_res_scores"
    assert colpali_amd.residual_wide_scores in colpali_amd.retrieval._KERNELS


# ------------------------------------------------------------------------------------------------------------------ routing
def _shards(seed=0, n=23, n_q=4, id_base=100):
    """a host PackedCorpus and a host ResidualWideCorpus over the same pages (same count, lengths and id_base; the codes are never read)"""
    import colpali_amd as amd

    g = torch.Generator().manual_seed(seed)
    pages = [_page(g, int(k), W) for k in torch.randint(1, 9, (n,), generator=g)]
    pages[7] = pages[3].clone()                                          # an exact tie
    pages[5] = pages[5][:0]                                              # a page of 0 rows
    packed = amd.pack_passages(pages, CPU, batch_size=None, id_base=id_base)
    rows = int(packed.lengths.sum())
    rc = amd.ResidualWideCorpus(centroids=torch.zeros(256, W, dtype=torch.bfloat16), codes=torch.zeros(rows, dtype=torch.int16).view(torch.uint16),
                                residuals=torch.zeros(rows, 80, dtype=torch.uint8), cutoffs=torch.zeros(3), weights=torch.zeros(4),
                                offsets=packed.offsets.clone(), clamp0=None, lengths=packed.lengths.clone(), id_base=id_base, bits=2)
    q = torch.stack([_page(g, 6, W) for _ in range(n_q)])
    labels = torch.randint(0, 6, (n,), generator=g) * 3 + 2
    return amd, g, packed, rc, q, labels


class Stubs(GroupHooks):
    """the filter and group stand-ins, plus a scorer and a rerank that answer for the residual shard with the packed pages' scores"""

    def __init__(self, packed, rc, q):
        super().__init__()
        self.packed, self.rc, self.q = packed, rc, q
        self.scored = 0

    def score(self, queries, shard):
        assert shard is self.rc or shard is self.packed
        assert queries is self.q                                         # an injected scorer receives the caller's queries untouched
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


def test_the_default_retriever_keeps_refusing_and_names_the_hook():
    amd, g, packed, rc, q, labels = _shards()
    r = amd.ShardedRetriever(rc)
    groups = amd.PageGroups.from_labels(labels, 100)
    pos = torch.tensor([100, 101, -1, 103])
    cand = torch.zeros((len(q), 2), dtype=torch.int64)
    for call in (lambda: r.search(q, k=2), lambda: r.search(q, k=2, filter=object()), lambda: r.search(q, k=2, group_by=groups),
                 lambda: r.search(q, k=2, candidates=cand, filter=object()), lambda: r.search(q, k=2, prefilter=rc.index, n_candidates=2, group_by=groups),
                 lambda: r.align(q, cand), lambda: r.mine(q, pos, 2)):
        with pytest.raises(NotImplementedError, match="ResidualWideCorpus.*width 128 only") as e:
            call()
        assert "score_fn=residual_wide_scores" in str(e.value)          # the message names the opt-in
        assert "align_fn=residual_align" not in str(e.value)            # ... and no hook that does not exist at this width


def test_an_injected_scorer_opens_the_routes_that_need_the_score_matrix():
    amd, g, packed, rc, q, labels = _shards()
    n, n_q = len(rc), len(q)
    h = Stubs(packed, rc, q)
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
    # the list route asks the shard for its format: a wide residual shard is its centroids' dtype at width 320
    assert (rc.dtype, rc.width) == (torch.bfloat16, W) and r._list_formats_fit(q) and not r._list_formats_fit(q.float())
    _same(r.search(q, 4, group_by=groups), ref.search(q, 4, group_by=groups), "grouped scan")
    _same(r.search(q, 4, candidates=cand, group_by=groups), ref.search(q, 4, candidates=cand, group_by=groups), "grouped candidates")
    pos = torch.tensor([[100, 103], [101, -1], [-1, -1], [107, 122]])
    scored = h.scored
    for kw in (dict(), dict(max_ratio=0.95), dict(skip_top=2)):
        _same(r.mine(q, pos, 3, **kw), ref.mine(q, pos, 3, **kw), f"mine {kw}")
    assert h.scored == scored + 3
    with pytest.raises(NotImplementedError, match="ResidualWideCorpus.*width 128 only"):      # align returns rows: it raises either way
        r.align(q, cand)


def test_the_kernel_hook_and_the_sibling_refusals():
    amd, g, packed, rc, q, labels = _shards()
    assert amd.residual_wide_scores in amd.retrieval._KERNELS and amd.residual_scores in amd.retrieval._KERNELS
    r = amd.ShardedRetriever(rc, score_fn=amd.residual_wide_scores)
    assert r._score is amd.residual_wide_scores and not r._res_refuses
    # the retriever packs for residual_wide_scores as it packs for its own scan (a host list of CPU tensors: the packer refuses, no GPU here)
    with pytest.raises(RuntimeError):
        r.search(list(q), k=2)
    with pytest.raises(RuntimeError):
        amd.residual_wide_scores(q, rc)
    with pytest.raises(ValueError):
        amd.residual_wide_scores(q, rc.index)
    with pytest.raises(RuntimeError):                                        # mine_hard_negatives dispatches on the class: a CPU shard is refused
        amd.mine_hard_negatives(q, rc, torch.tensor([100, 101, -1, 103]), 2)
    # the siblings refuse each other by type, naming the width, in both directions and before any kernel
    rows = 8
    narrow = amd.ResidualCorpus(centroids=torch.zeros(256, 128, dtype=torch.bfloat16), codes=torch.zeros(rows, dtype=torch.int16).view(torch.uint16),
                                residuals=torch.zeros(rows, 32, dtype=torch.uint8), cutoffs=torch.zeros(3), weights=torch.zeros(4),
                                offsets=torch.tensor([0, 3, 8], dtype=torch.int32), clamp0=None, lengths=torch.tensor([3, 5]), id_base=0, bits=2)
    q128 = torch.zeros(2, 4, 128, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="ResidualWideCorpus exists at width 320 only"):
        amd.residual_wide_scores(q128, narrow)
    with pytest.raises(NotImplementedError, match="ResidualCorpus exists at width 128 only"):
        amd.residual_scores(q, rc)
    with pytest.raises(NotImplementedError, match="width 128"):
        amd.ShardedRetriever(rc, score_fn=amd.residual_scores).search(q, k=2)
    with pytest.raises(NotImplementedError, match="width 320"):
        amd.ShardedRetriever(narrow, score_fn=amd.residual_wide_scores).search(q128, k=2)
