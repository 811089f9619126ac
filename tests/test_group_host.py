"""Document-level search without a GPU: the numpy restatement (tests/group_truth.py) against a brute-force loop, `PageGroups`'
argument errors, the C ABI's refusals (before any device work), and the host logic of `ShardedRetriever.search(group_by=)` /
`LiveCorpus.search(group_by=)` with the restatement injected for the kernels: every route against the truth, the routing rule of
"auto" with the 4096 cap, and gloo worlds of 2 and 3 against the single-shard answer."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import filter_truth as ft
from tests import group_truth as gt
from tests.test_filter_host import Hooks as FilterHooks
from tests.test_filter_host import _filter, _free_port, _pack_fn, _page, _score_fn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")
NINF = -np.inf


# ------------------------------------------------------------------------------------------------------------ the restatement
def _grid_scores(r, n_q, n):
    s = r.integers(-6, 7, size=(n_q, n)).astype(np.float32) / 4          # a coarse grid: many exact ties
    s[r.random((n_q, n)) < 0.15] = -np.inf
    s[(s == 0) & (r.random((n_q, n)) < 0.5)] = -0.0
    return s


def _key(s):
    return -float(s)                                                     # -0.0 and +0.0 give keys that compare equal


@pytest.mark.parametrize("seed,n_q,n,n_docs,k,id_base", [(0, 4, 23, 5, 3, 0), (1, 3, 70, 70, 80, 1000), (2, 5, 33, 1, 1, 7), (3, 2, 40, 9, 9, 5)])
def test_truth_equals_a_brute_force_loop(seed, n_q, n, n_docs, k, id_base):
    r = np.random.default_rng(seed)
    s = _grid_scores(r, n_q, n)
    labels = r.integers(0, n_docs, n).astype(np.int64) * 3 + 2           # sparse document ids, pages interleaved
    ok = r.random((n_q, n)) < 0.7
    assert np.signbit(s[s == 0]).any() or n_docs == 1
    gids, gs, gp = gt.reduce_truth(s, labels, id_base)
    assert gids.tolist() == sorted(set(labels.tolist()))
    for q in range(n_q):
        for g, d in enumerate(gids):
            cand = sorted((_key(s[q, c]), c) for c in range(n) if labels[c] == d and s[q, c] != NINF)
            if not cand:
                assert gs[q, g] == NINF and gp[q, g] == -1
            else:
                c = cand[0][1]
                assert gp[q, g] == c + id_base and gs[q, g].tobytes() == s[q, c].tobytes()       # the winner's own bits
    for allowed in (None, ok):
        ws, wg, wp = gt.search_truth(s, labels, k, id_base, allowed)
        for q in range(n_q):
            docs = []
            for d in set(labels.tolist()):
                cand = sorted((_key(s[q, c]), c) for c in range(n)
                              if labels[c] == d and s[q, c] != NINF and (allowed is None or allowed[q, c]))
                if cand:
                    docs.append((cand[0][0], d, cand[0][1] + id_base))
            docs = sorted(docs)[:k]
            pad = k - len(docs)
            assert wg[q].tolist() == [d for _, d, _ in docs] + [-1] * pad
            assert wp[q].tolist() == [p for _, _, p in docs] + [-1] * pad
            assert ws[q].tolist() == [-a for a, _, _ in docs] + [NINF] * pad
            assert not np.signbit(ws[q][ws[q] == 0]).any()               # as the top-k returns a zero: +0.0
    # select: random rows of triples, ids -1 and -inf scores mixed in
    m = 2 * n
    cs = _grid_scores(r, n_q, m)
    cg = r.integers(-1, n_docs, (n_q, m)).astype(np.int64)
    cp = np.stack([r.permutation(m) for _ in range(n_q)]).astype(np.int64) + id_base
    ws, wg, wp = gt.select_truth(cs, cg, cp, k)
    for q in range(n_q):
        docs = []
        for d in set(cg[q][cg[q] >= 0].tolist()):
            cand = sorted((_key(cs[q, j]), cp[q, j]) for j in range(m) if cg[q, j] == d and cs[q, j] != NINF)
            if cand:
                docs.append((cand[0][0], d, cand[0][1]))
        docs = sorted(docs)[:k]
        pad = k - len(docs)
        assert wg[q].tolist() == [d for _, d, _ in docs] + [-1] * pad and wp[q].tolist() == [p for _, _, p in docs] + [-1] * pad
        assert ws[q].tolist() == [-a for a, _, _ in docs] + [NINF] * pad


def test_truth_hand_written_case():
    #                 page  10    11    12     13    14    15
    s = np.asarray([[3.0, 5.0, 5.0, NINF, 1.0, 5.0], [-0.0, 0.0, NINF, NINF, -2.0, NINF]], dtype=np.float32)
    labels = np.asarray([7, 4, 7, 9, 4, 4])                              # document 9 holds only a page that scores -inf
    gids, gs, gp = gt.reduce_truth(s, labels, 10)
    assert gids.tolist() == [4, 7, 9]
    assert gs[0].tolist() == [5.0, 5.0, NINF] and gp[0].tolist() == [11, 12, -1]          # 11 beats 15 inside document 4
    assert gp[1].tolist() == [11, 10, -1] and np.signbit(gs[1, 1]) and not np.signbit(gs[1, 0])     # -0.0 keeps its bits
    ws, wg, wp = gt.search_truth(s, labels, 3, 10)
    assert wg.tolist() == [[4, 7, -1], [4, 7, -1]] and wp.tolist() == [[11, 12, -1], [11, 10, -1]]   # 0.0 == -0.0: document 4 first
    assert ws[0].tolist() == [5.0, 5.0, NINF] and not np.signbit(ws[1, :2]).any()
    ok = np.ones((2, 6), dtype=bool)
    ok[:, 1] = False                                                     # without page 11 document 4 is scored by page 15, then 14
    ws, wg, wp = gt.search_truth(s, labels, 2, 10, ok)
    assert wg.tolist() == [[4, 7], [7, 4]] and wp.tolist() == [[15, 12], [10, 14]] and ws[1].tolist() == [0.0, -2.0]
    ws, wg, wp = gt.select_truth(s, [[1, 1, 2, 2, -1, 3]] * 2, [[9, 8, 7, 6, 5, 4]] * 2, 4)
    assert wg.tolist() == [[1, 2, 3, -1], [1, -1, -1, -1]] and wp.tolist() == [[8, 7, 4, -1], [8, -1, -1, -1]]


# ------------------------------------------------------------------------------------------------------------------- the ABI
def _header_constant(name):
    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))


def test_the_header_declares_the_entries_and_the_package_exports_the_names():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    L = colpali_amd._lib.lib()
    for name in ("msim_group_reduce", "msim_group_select"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and hasattr(L, name)
    assert L.msim_abi_version() == colpali_amd._lib.ABI_VERSION
    for name in ("PageGroups", "group_reduce", "group_select"):
        assert name in colpali_amd.__all__
    assert colpali_amd.PageGroups is colpali_amd.group.PageGroups
    assert 1 <= _header_constant("MSIM_GROUP_THREAD_MAX") < _header_constant("MSIM_GROUP_WAVE_MAX")
    assert _header_constant("MSIM_GROUP_SELECT_MAX_M") == colpali_amd.group.SELECT_MAX_M == 4096
    assert _header_constant("MSIM_GROUP_SELECT_MAX_K") == colpali_amd.group.SELECT_MAX_K == 1024


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def reduce(scores=FAKE, ld=100, n_q=3, n=100, offsets=FAKE, pages=FAKE, n_groups=7, out_s=FAKE, out_p=FAKE, ld_out=7):
        return L.msim_group_reduce(scores, ld, n_q, n, offsets, pages, n_groups, 0, out_s, out_p, ld_out, None)

    def select(scores=FAKE, gids=FAKE, pages=FAKE, n_q=3, m=100, ld=100, k=10, out_s=FAKE, out_g=FAKE, out_p=FAKE):
        return L.msim_group_select(scores, gids, pages, n_q, m, ld, k, out_s, out_g, out_p, None)

    nothing = dict(scores=None, offsets=None, pages=None, out_s=None, out_p=None)
    assert reduce(n_q=0, **nothing) == 0 and reduce(n_groups=0, **nothing) == 0          # 0 before a pointer is looked at
    nothing = dict(scores=None, gids=None, pages=None, out_s=None, out_g=None, out_p=None)
    assert select(n_q=0, **nothing) == 0 and select(m=0, **nothing) == 0
    for kw in (dict(n_q=-1), dict(n=-1), dict(n_groups=-1), dict(scores=None), dict(offsets=None), dict(pages=None), dict(out_s=None),
               dict(out_p=None), dict(scores=FAKE + 2), dict(offsets=FAKE + 2), dict(pages=FAKE + 1), dict(out_s=FAKE + 2),
               dict(out_p=FAKE + 4), dict(ld=99), dict(ld_out=6)):
        assert reduce(**kw) == EINVAL, kw
        assert L.msim_last_error()
    assert reduce(n=1 << 31, ld=1 << 31) == EUNSUPPORTED
    for kw in (dict(n_q=-1), dict(m=-1), dict(k=0), dict(k=-3), dict(scores=None), dict(gids=None), dict(pages=None), dict(out_s=None),
               dict(out_g=None), dict(out_p=None), dict(scores=FAKE + 2), dict(gids=FAKE + 4), dict(pages=FAKE + 4), dict(out_s=FAKE + 1),
               dict(out_g=FAKE + 4), dict(out_p=FAKE + 4), dict(ld=99)):
        assert select(**kw) == EINVAL, kw
        assert L.msim_last_error()
    assert select(m=4097, ld=4097) == EUNSUPPORTED and select(k=1025) == EUNSUPPORTED
    assert b"4096" in L.msim_last_error() or b"1024" in L.msim_last_error()


# ----------------------------------------------------------------------------------------------------------------- PageGroups
def test_page_groups_forms_and_errors(monkeypatch):
    import colpali_amd as amd

    PG = amd.PageGroups
    labels = torch.tensor([40, 7, 40, 40, 9, 7], dtype=torch.int64)
    g = PG.from_labels(labels, 100)
    assert len(g) == 6 and g.id_base == 100 and g.device == CPU and g.n_groups is None
    assert g.prepare() is g and g.prepare().n_groups == 3 and g.max_group == 3
    assert g.group_ids.tolist() == [7, 9, 40] and g.group_ids.dtype == torch.int64
    assert g.page_group.tolist() == [2, 0, 2, 2, 1, 0] and g.page_group.dtype == torch.int32
    assert g.offsets.tolist() == [0, 2, 3, 6] and g.offsets.dtype == torch.int32
    assert g.pages.tolist() == [1, 5, 4, 0, 2, 3] and g.pages.dtype == torch.int32          # ascending inside every document
    ids = torch.tensor([[100, 105, 99, -1], [106, 104, 103, 101]])
    assert g.doc_ids(ids).tolist() == [[40, 7, -1, -1], [-1, 9, 40, 7]]                     # -1 and ids off the shard: -1
    assert PG.from_labels(labels).id_base == 0
    one = PG.from_labels(torch.zeros(5, dtype=torch.int64)).prepare()
    assert one.n_groups == 1 and one.max_group == 5 and one.offsets.tolist() == [0, 5]
    empty = PG.from_labels(torch.zeros(0, dtype=torch.int64)).prepare()
    assert empty.n_groups == 0 and empty.max_group == 0 and empty.offsets.tolist() == [0]
    for bad in (labels.to(torch.int32), labels.float(), labels[None], torch.tensor(3), labels.tolist()):
        with pytest.raises(ValueError):
            PG.from_labels(bad)
    neg = PG.from_labels(torch.tensor([3, -1, 2], dtype=torch.int64))
    with pytest.raises(ValueError, match="negative"):
        neg.prepare()
    fresh = PG.from_labels(labels)
    monkeypatch.setattr(type(fresh), "device", property(lambda self: torch.device("cuda:0")))    # stands in for device labels
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before the capture"):
        fresh.prepare()
    monkeypatch.undo()
    for fn, args in ((amd.group_reduce, (torch.zeros(3, 6), g)), (amd.group_select, (torch.zeros(3, 4), ids[:1].repeat(3, 1), ids[:1].repeat(3, 1), 2))):
        with pytest.raises(ValueError):                                  # the kernels have no CPU fallback
            fn(*args)
    with pytest.raises(ValueError):
        amd.group_reduce(torch.zeros(3, 6), labels)


# ------------------------------------------------------------------------------------------ injected stand-ins for the kernels
class Hooks(FilterHooks):
    """the restatement behind the filter hooks and the two group hooks, counting the calls"""

    def __init__(self):
        super().__init__()
        self.calls.update(reduce=0, select=0)
        self.selected = []

    def reduce(self, scores, groups):
        self.calls["reduce"] += 1
        gids, gs, gp = gt.reduce_truth(scores.numpy(), groups.labels.numpy(), groups.id_base)
        assert gids.tolist() == groups.group_ids.tolist()
        return torch.from_numpy(gs), torch.from_numpy(gp)

    def select(self, scores, gids, pages, k):
        self.calls["select"] += 1
        self.selected.append(int(scores.shape[1]))
        return tuple(torch.from_numpy(x) for x in gt.select_truth(scores.numpy(), gids.numpy(), pages.numpy(), k))

    def kw(self):
        return dict(super().kw(), group_reduce_fn=self.reduce, group_select_fn=self.select)


def _case(seed=0, n=41, n_q=5, id_base=100, n_docs=9):
    import colpali_amd as amd

    g = torch.Generator().manual_seed(seed)
    pages = [_page(g, int(k)) for k in torch.randint(1, 12, (n,), generator=g)]
    pages[7] = pages[3].clone()                                          # exact ties: inside a document ...
    pages[20] = pages[11].clone()                                        # ... and between two
    pages[5] = pages[5][:0]                                              # a page of 0 rows
    pages[30] = pages[30][:0]
    labels = torch.randint(0, n_docs, (n,), generator=g) * 5 + 1
    labels[3] = labels[7] = 11
    labels[11], labels[20] = 6, 16
    labels[30] = 1000                                                    # a document whose only page has 0 rows
    corpus = amd.pack_passages(pages, CPU, batch_size=None, id_base=id_base)
    q = torch.stack([_page(g, 6) for _ in range(n_q)])
    return amd, g, pages, labels, corpus, q


def _check(got, want, msg=""):
    assert len(got) == 3
    for a, b, what in zip(got, want, ("scores", "group_ids", "page_ids")):
        np.testing.assert_array_equal(a.numpy(), b, err_msg=f"{msg}: {what}")


@pytest.mark.parametrize("k", [4, 50])
def test_every_route_equals_the_truth(k):
    amd, g, pages, labels, corpus, q = _case()
    n, n_q = len(corpus), len(q)
    s = _score_fn(q, corpus).numpy()
    assert np.isneginf(s[:, [5, 30]]).all() and (s[:, 3] == s[:, 7]).all() and (s[:, 11] == s[:, 20]).all()
    h = Hooks()
    r = amd.ShardedRetriever(corpus, **h.kw())
    groups = amd.PageGroups.from_labels(labels, 100)
    want = gt.search_truth(s, labels.numpy(), k, 100)
    assert 1000 not in want[1] and (want[1][np.isneginf(want[0])] == -1).all() and (want[2][np.isneginf(want[0])] == -1).all()
    _check(r.search(q, k, group_by=groups), want, "scan")
    assert h.calls["reduce"] == 1 and h.calls["select"] == 0 and groups.n_groups is not None
    plain = r.search(q, k)
    assert isinstance(plain, tuple) and len(plain) == 2                  # without group_by: the 2-tuple, as before
    # candidates=: the listed pages only
    cand = torch.stack([torch.randperm(n + 10, generator=g)[:25] + 95 for _ in range(n_q)])
    cand[0, :3] = -1
    listed = np.zeros((n_q, n), dtype=bool)
    for q_, row in enumerate(cand.numpy()):
        listed[q_, row[(row >= 100) & (row < 100 + n)] - 100] = True
    _check(r.search(q, k, candidates=cand, group_by=groups), gt.search_truth(s, labels.numpy(), k, 100, listed), "candidates")
    assert h.selected[-1] == 25
    # prefilter=: n_candidates counts pages
    pooled = amd.pack_passages([p[:2] for p in pages], CPU, batch_size=None, id_base=100)
    _, kept = ft.search_truth(_score_fn(q, pooled).numpy(), np.ones((n_q, n), dtype=bool), 12, 100)
    listed = np.zeros((n_q, n), dtype=bool)
    for q_, row in enumerate(kept):
        listed[q_, row[row >= 0] - 100] = True
    _check(r.search(q, k, prefilter=pooled, n_candidates=12, group_by=groups), gt.search_truth(s, labels.numpy(), k, 100, listed), "prefilter")
    assert h.selected[-1] == 12
    # filter=: both routes, equal to each other and to the truth
    r_ = np.random.default_rng(5)
    shared = r_.random(n) < 0.3
    shared[[3, 5, 7, 11, 20]] = True
    per = r_.random((n_q, n)) < 0.3
    per[1] = False
    lab = (r_.integers(0, 4, n).astype(np.int32), r_.integers(0, 4, n_q).astype(np.int32))
    for spec in (("shared", shared), ("per_query", per), ("labels", *lab)):
        ok = ft.allowed(spec, n_q, n)
        want = gt.search_truth(s, labels.numpy(), k, 100, ok)
        got = {}
        for route in ("mask", "list", "auto"):
            got[route] = r.search(q, k, filter=_filter(amd, spec, 100), filter_route=route, group_by=groups)
            _check(got[route], want, f"{spec[0]} {route}")
        for a, b in zip(got["mask"], got["list"]):
            assert torch.equal(a, b)
        _check(r.search(q, k, prefilter=pooled, n_candidates=n, filter=_filter(amd, spec, 100), group_by=groups), want, f"{spec[0]} two-stage")
    assert h.calls["mask"] >= 3 and h.calls["list"] >= 3


def test_routing_rule_of_auto_with_the_cap_and_argument_errors():
    import colpali_amd as amd

    g = torch.Generator().manual_seed(3)
    n = 5 * 4097 + 5                                                     # max_allowed = 4097 is still below n / 5
    page = _page(g, 1)
    offsets = torch.arange(n + 1, dtype=torch.int32)
    corpus = amd.PackedCorpus(blob=page.expand(n, 128), offsets=offsets, clamp0=None, lengths=torch.ones(n, dtype=torch.int64), id_base=0)
    q = torch.stack([_page(g, 2) for _ in range(2)])
    labels = torch.arange(n, dtype=torch.int64) // 3
    groups = amd.PageGroups.from_labels(labels)

    def fake_scores(queries, c):
        return torch.zeros((len(queries), len(c)), dtype=torch.float32)

    def fake_rerank(queries, c, cand):
        return torch.zeros(cand.shape, dtype=torch.float32), cand

    def route_taken(count, **kw):
        h = Hooks()
        mask = torch.zeros(n, dtype=torch.bool)
        mask[:count] = True
        hooks = dict(h.kw(), score_fn=fake_scores, rerank_fn=fake_rerank,
                     group_reduce_fn=lambda s, gr: (h.calls.__setitem__("reduce", h.calls["reduce"] + 1),
                                                    (torch.zeros(len(s), gr.n_groups), torch.zeros(len(s), gr.n_groups, dtype=torch.int64)))[1],
                     group_select_fn=lambda s, gi, p, k: (h.calls.__setitem__("select", h.calls["select"] + 1),
                                                          (s[:, :k], gi[:, :k], p[:, :k]))[1])
        amd.ShardedRetriever(corpus, **hooks).search(q, 3, filter=amd.PageFilter.from_mask(mask, 0, pack_fn=_pack_fn), **kw)
        return {key: h.calls[key] for key in ("mask", "list", "reduce", "select")}

    assert 4097 <= n * amd.filter.LIST_ROUTE_MAX_FRACTION
    assert route_taken(4096, group_by=groups) == {"mask": 0, "list": 1, "reduce": 0, "select": 1}
    assert route_taken(4097, group_by=groups) == {"mask": 1, "list": 0, "reduce": 1, "select": 0}        # the cap, not the fraction
    assert route_taken(4097) == {"mask": 0, "list": 1, "reduce": 0, "select": 0}                        # without group_by: as before
    assert route_taken(4096, group_by=groups, filter_route="mask")["reduce"] == 1
    with pytest.raises(NotImplementedError, match="4096"):
        route_taken(4097, group_by=groups, filter_route="list")
    r = amd.ShardedRetriever(corpus, **dict(Hooks().kw(), score_fn=fake_scores, rerank_fn=fake_rerank))
    with pytest.raises(NotImplementedError, match="4096"):
        r.search(q, 3, candidates=torch.zeros((2, 4097), dtype=torch.int64), group_by=groups)
    with pytest.raises(NotImplementedError, match="4096"):
        r.search(q, 3, prefilter=corpus, n_candidates=4097, group_by=groups)
    for bad in (labels, amd.PageGroups.from_labels(labels[:-1]), amd.PageGroups.from_labels(labels, 1)):
        for kw in (dict(), dict(candidates=torch.zeros((2, 4), dtype=torch.int64)), dict(prefilter=corpus, n_candidates=3)):
            with pytest.raises(ValueError):
                r.search(q, 3, group_by=bad, **kw)
    other = amd.PageGroups.from_labels(labels)
    other.labels = other.labels.to("meta")                               # groups on another device than the shard
    with pytest.raises(ValueError, match="live on"):
        r.search(q, 3, group_by=other)
    forced = amd.ShardedRetriever(corpus, force_collective=True, **dict(Hooks().kw(), score_fn=fake_scores))
    with pytest.raises(ValueError, match="4096"):
        forced.search(q, 4097, group_by=groups)
    with pytest.raises(ValueError, match="4096"):
        amd.ShardedRetriever(corpus, world=5, rank=0, dist=dist, **Hooks().kw()).search(q, 820, group_by=groups)


# ------------------------------------------------------------------------------------------------- the message of the collective
class RecordingDist:
    """a one-rank stand-in for torch.distributed: records every message, and the gathered buffer is the rank's own"""

    def __init__(self):
        self.messages = []

    def all_gather_into_tensor(self, out, mine, group=None):
        assert mine.dtype == torch.uint8 and mine.dim() == 1 and out.dtype == torch.uint8 and out.numel() == mine.numel()
        self.messages.append(int(mine.numel()))
        out.copy_(mine)


def test_one_all_gather_per_merge_and_the_size_of_its_message():
    from oracle import topk_oracle

    n_q, k = 3, 1                                                        # 12 bytes of scores: the padding to 8 is not zero
    amd, g, pages, labels, corpus, q = _case(n_q=n_q)
    pad8 = (4 * n_q * k + 7) // 8 * 8
    assert pad8 == 16
    s = _score_fn(q, corpus)
    fake = RecordingDist()
    got = amd.shard_topk(s, k, 100, 1, fake, None, topk_oracle.torch_select, force_collective=True)
    assert fake.messages == [pad8 + 8 * n_q * k]                         # ONE all-gather: [scores | pad | ids]
    for a, b in zip(got, amd.shard_topk(s, k, 100, select=topk_oracle.torch_select)):
        assert torch.equal(a, b)
    groups = amd.PageGroups.from_labels(labels, 100)
    cand = torch.stack([torch.randperm(len(corpus) + 10, generator=g)[:25] + 95 for _ in range(n_q)])
    alone = amd.ShardedRetriever(corpus, **Hooks().kw())
    for kw in (dict(), dict(candidates=cand)):
        fake = RecordingDist()
        forced = amd.ShardedRetriever(corpus, dist=fake, force_collective=True, **Hooks().kw())
        got = forced.search(q, k, group_by=groups, **kw)
        assert fake.messages == [pad8 + 16 * n_q * k], kw                # ONE all-gather: [scores | pad | document ids | page ids]
        _check(got, [x.numpy() for x in alone.search(q, k, group_by=groups, **kw)], f"forced {sorted(kw)}")


# --------------------------------------------------------------------------------------------- LiveCorpus.search(group_by=), host logic
def test_live_corpus_scores_documents_by_their_surviving_pages():
    import colpali_amd as amd
    from tests import live_truth

    g = torch.Generator().manual_seed(5)
    pages = [_page(g, int(k)) for k in torch.randint(1, 9, (30,), generator=g)]
    h = Hooks()
    live = amd.LiveCorpus(300, 32, CPU, id_base=50, mask_fn=lambda s, a: torch.from_numpy(live_truth.mask(s.numpy(), a.numpy())), **h.kw())
    live.add(pages[:20])
    live.add(pages[20:])
    labels = torch.arange(30, dtype=torch.int64) % 7 + 3
    labels[[0, 9, 21]] = 77                                              # a document that will lose every page
    groups = amd.PageGroups.from_labels(labels, 50)                      # built after the last add, over all slots
    q = torch.stack([_page(g, 6) for _ in range(4)])
    s = _score_fn(q, live.view()).numpy()
    best_of_5 = int(np.argmax(np.where(labels.numpy() == 5, s[0], -np.inf)))
    deleted = sorted({0, 9, 21, best_of_5, 4, 13})
    live.delete([50 + d for d in deleted])
    alive = np.ones((4, 30), dtype=bool)
    alive[:, deleted] = False
    want = gt.search_truth(s, labels.numpy(), 8, 50, alive)
    assert 77 not in want[1] and 5 in want[1][0] and 50 + best_of_5 not in want[2]
    _check(live.search(q, 8, group_by=groups), want, "scan")
    cand = torch.arange(45, 85, dtype=torch.int64).repeat(4, 1)
    _check(live.search(q, 8, candidates=cand, group_by=groups), want, "candidates")
    spec = ("shared", np.arange(30) % 2 == 0)
    ok = ft.allowed(spec, 4, 30) & alive
    for route in ("mask", "list"):
        _check(live.search(q, 8, filter=_filter(amd, spec, 50), filter_route=route, group_by=groups),
               gt.search_truth(s, labels.numpy(), 8, 50, ok), route)
    assert len(live.search(q, 8)) == 2
    with pytest.raises(ValueError):
        live.search(q, 8, group_by=amd.PageGroups.from_labels(torch.zeros(32, dtype=torch.int64), 50))      # the slots, not the capacity


# --------------------------------------------------------------------------------------------------------- sharded, over gloo
def _world_case(n_docs, world):
    import colpali_amd as amd

    g = torch.Generator().manual_seed(21)
    pages = [_page(g, n) for n in torch.randint(1, 20, (n_docs,), generator=g).tolist()]
    pages[4] = pages[n_docs - 3].clone()                                 # an exact tie across shards, in two documents
    pages[6] = pages[6][:0]
    q = torch.stack([_page(g, 8) for _ in range(5)])
    labels = torch.randint(0, 6, (n_docs,), generator=g) * 2 + 10
    labels[4], labels[n_docs - 3] = 3, 5
    for rank in range(1, world):                                         # a document straddling every shard boundary
        lo = amd.shard_range(n_docs, world, rank)[0]
        labels[lo - 2:lo + 2] = 100 + rank
    # document 200: most pages on the first shard, its best page for query 0 on the last
    first_hi = amd.shard_range(n_docs, world, 0)[1]
    labels[[0, 1, 2]] = 200
    assert first_hi > 5
    labels[n_docs - 1] = 200
    pages[n_docs - 1] = q[0].clone()                                     # query 0 against itself: its highest score anywhere
    return pages, q, labels


def _worker(rank, world, port, n_docs, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import colpali_amd as amd

    pages, q, labels = _world_case(n_docs, world)
    lo, hi = amd.shard_range(n_docs, world, rank)
    shard = amd.pack_passages(pages[lo:hi], CPU, batch_size=None, id_base=lo)
    pooled = amd.pack_passages([d[:2] for d in pages[lo:hi]], CPU, batch_size=None, id_base=lo)
    groups = amd.PageGroups.from_labels(labels[lo:hi].clone(), lo)
    r = amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, **Hooks().kw())
    mask = np.arange(n_docs) % 3 != 1
    out = {}
    runs = {"scan": dict(), "two": dict(prefilter=pooled, n_candidates=9),
            "mask": dict(filter=_filter(amd, ("shared", mask[lo:hi]), lo), filter_route="mask"),
            "list": dict(filter=_filter(amd, ("shared", mask[lo:hi]), lo), filter_route="list")}
    for name, kw in runs.items():
        for k in (4, 40):
            s, gi, p = r.search(q, k, group_by=groups, **kw)
            out[f"{name}{k}_s"], out[f"{name}{k}_g"], out[f"{name}{k}_p"] = s.numpy(), gi.numpy(), p.numpy()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs", [(2, 23), (3, 31)])
def test_sharded_grouped_search_equals_the_single_shard_truth(tmp_path, world, n_docs):
    import colpali_amd as amd

    mp.spawn(_worker, args=(world, _free_port(), n_docs, str(tmp_path)), nprocs=world, join=True)
    pages, q, labels = _world_case(n_docs, world)
    labels = labels.numpy()
    exact = _score_fn(q, amd.pack_passages(pages, CPU, batch_size=None)).numpy()
    coarse = _score_fn(q, amd.pack_passages([d[:2] for d in pages], CPU, batch_size=None)).numpy()
    all_ok = np.ones_like(exact, dtype=bool)
    ok = np.broadcast_to(np.arange(n_docs) % 3 != 1, exact.shape)
    _, kept = ft.search_truth(coarse, all_ok, 9)
    listed = np.zeros_like(all_ok)
    for q_, row in enumerate(kept):
        listed[q_, row[row >= 0]] = True
    # the document whose best page sits on the other rank from most of its pages wins query 0, through that page
    top = gt.search_truth(exact, labels, 4)
    assert top[1][0, 0] == 200 and top[2][0, 0] == n_docs - 1
    for rank in range(1, world):
        assert (labels == 100 + rank).sum() == 4                         # the straddling documents are intact
    # world 1 with the same hooks is the same answer
    single = amd.ShardedRetriever(amd.pack_passages(pages, CPU, batch_size=None), **Hooks().kw())
    groups = amd.PageGroups.from_labels(torch.from_numpy(labels))
    for k in (4, 40):
        want = {"scan": gt.search_truth(exact, labels, k), "two": gt.search_truth(exact, labels, k, 0, listed),
                "mask": gt.search_truth(exact, labels, k, 0, ok)}
        want["list"] = want["mask"]
        _check(single.search(q, k, group_by=groups), want["scan"], "world 1")
        for rank in range(world):
            got = np.load(tmp_path / f"rank{rank}.npz")
            for name, w in want.items():
                for a, what in zip(w, "sgp"):
                    np.testing.assert_array_equal(got[f"{name}{k}_{what}"], a, err_msg=f"rank {rank}: {name} k={k} {what}")
