"""Filtered search without a GPU: the numpy restatement (tests/filter_truth.py) against a brute-force loop, `PageFilter`'s argument
errors, the C ABI's refusals (before any device work), and the host logic of `ShardedRetriever.search(filter=)` /
`LiveCorpus.search(filter=)` with the restatement injected for the kernels: both routes against the truth, the routing rules of
"auto", two-stage search under a filter, and gloo worlds of 2 and 3 against the single-shard answer."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import filter_truth as ft

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("seed,n_q,n,k,id_base", [(0, 4, 23, 5, 0), (1, 3, 70, 80, 1000), (2, 5, 33, 1, 7)])
def test_truth_equals_a_brute_force_loop(seed, n_q, n, k, id_base):
    r = np.random.default_rng(seed)
    s = r.integers(-6, 7, size=(n_q, n)).astype(np.float32) / 4          # a coarse grid: many exact ties
    s[r.random((n_q, n)) < 0.1] = -np.inf                                # pages of 0 rows
    specs = [("shared", r.random(n) < 0.5), ("per_query", r.random((n_q, n)) < 0.3),
             ("labels", r.integers(0, 3, n).astype(np.int32), r.integers(0, 4, n_q).astype(np.int32))]
    for spec in specs:
        ok = ft.allowed(spec, n_q, n)
        for q in range(n_q):                                             # `allowed`, one entry at a time
            for c in range(n):
                want = (bool(spec[1][c]) if spec[0] == "shared" else bool(spec[1][q, c]) if spec[0] == "per_query"
                        else spec[1][c] == spec[2][q])
                assert ok[q, c] == want
        got_s, got_i = ft.search_truth(s, ok, k, id_base)
        for q in range(n_q):
            rows = sorted((-float(s[q, c]), c + id_base) for c in range(n) if ok[q, c] and s[q, c] != -np.inf)[:k]
            assert got_i[q].tolist() == [i for _, i in rows] + [-1] * (k - len(rows))
            assert got_s[q].tolist() == [-a for a, _ in rows] + [-np.inf] * (k - len(rows))
        m = ft.masked(s, ok)
        assert np.isneginf(m[~ok]).all() and (m[ok] == s[ok]).all()
        for m_cap in (int(ok.sum(1).max()), int(ok.sum(1).max()) + 3, max(int(ok.sum(1).max()) - 1, 0)):
            cand, counts, status = ft.list_truth(ok, m_cap, id_base)
            for q in range(n_q):
                ids = [c + id_base for c in range(n) if ok[q, c]]
                assert counts[q] == len(ids) and cand[q].tolist() == (ids + [-1] * m_cap)[:m_cap]
            assert status == int(any(ok[q].sum() > m_cap for q in range(n_q)))
        ids = r.integers(id_base - 3, id_base + n + 3, size=(n_q, 9))
        ids[:, 0] = -1
        out = ft.ids_truth(ids, ok, id_base)
        for q in range(n_q):
            for j in range(9):
                c = ids[q, j] - id_base
                inside = ids[q, j] >= 0 and 0 <= c < n
                assert out[q, j] == (-1 if inside and not ok[q, c] else ids[q, j])
    words = ft.pack(specs[1][1])
    assert words.dtype == np.uint32 and words.shape == (n_q, (n + 31) // 32)
    for c in range(32 * words.shape[1]):
        bit = (words[:, c // 32] >> np.uint32(c % 32)) & 1
        assert (bit == (specs[1][1][:, c] if c < n else 0)).all()
    assert (ft.with_alive(ft.allowed(specs[0], n_q, n), np.zeros(n, np.uint8)) == 0).all()


def test_truth_hand_written_case():
    s = np.asarray([[3.0, 5.0, 5.0, -np.inf, 1.0], [2.0, 2.0, 2.0, 2.0, 2.0]], dtype=np.float32)
    ok = ft.allowed(("shared", [1, 0, 1, 1, 1]), 2, 5)
    gs, gi = ft.search_truth(s, ok, 4, id_base=10)
    assert gi.tolist() == [[12, 10, 14, -1], [10, 12, 13, 14]]           # the allowed 0-row page 13 is (-inf, -1), ties by id
    assert gs[0].tolist() == [5.0, 3.0, 1.0, -np.inf]
    ts, ti = ft.two_stage_truth(s, -s, ok, 2, 3, id_base=10)             # stage 1 keeps {12, 10}; stage 2 orders them by -s
    assert ti.tolist() == [[10, 12, -1], [10, 12, -1]] and ts[0].tolist() == [-3.0, -5.0, -np.inf]


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_entries_and_the_package_exports_the_names():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    L = colpali_amd._lib.lib()
    for name in ("msim_filter_pack", "msim_filter_mask", "msim_filter_list", "msim_filter_ids"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and hasattr(L, name)
    assert re.search(r"\bsize_t\s+msim_filter_list_workspace_bytes\s*\(", header)
    assert L.msim_abi_version() == 22 and colpali_amd._lib.ABI_VERSION == 22
    assert "PageFilter" in colpali_amd.__all__ and colpali_amd.PageFilter is colpali_amd.filter.PageFilter
    assert 0 < colpali_amd.filter.LIST_ROUTE_MAX_FRACTION <= 1 / 5
    assert f"S = {8192}" in header and L.msim_filter_list_workspace_bytes(4, 100) >= 4


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def pack(mask=FAKE, ld_mask=100, rows=3, n=100, words=FAKE, ld_words=4):
        return L.msim_filter_pack(mask, ld_mask, rows, n, words, ld_words, None)

    def mask(scores=FAKE, ld=100, n_q=3, n=100, bits=FAKE, ld_words=0, pl=None, ql=None, alive=None):
        return L.msim_filter_mask(scores, ld, n_q, n, bits, ld_words, pl, ql, alive, None)

    def lst(bits=FAKE, ld_words=0, pl=None, ql=None, alive=None, n_q=3, n=100, cand=FAKE, ld_cand=10, m_cap=10, counts=FAKE, ws=FAKE):
        return L.msim_filter_list(bits, ld_words, pl, ql, alive, n_q, n, 0, cand, ld_cand, m_cap, counts, ws, None)

    def ids(ids=FAKE, ld=10, n_q=3, m=10, n=100, bits=FAKE, ld_words=0, pl=None, ql=None, alive=None):
        return L.msim_filter_ids(ids, ld, n_q, m, n, 0, bits, ld_words, pl, ql, alive, None)

    # nothing to do: 0 before a pointer is looked at
    assert pack(rows=0, mask=None, words=None) == 0 and pack(n=0, mask=None, words=None) == 0
    assert mask(n_q=0, scores=None, bits=None) == 0 and mask(n=0, scores=None, bits=None) == 0
    assert lst(n_q=0, bits=None, cand=None, counts=None, ws=None) == 0 and lst(n=0, bits=None, cand=None, counts=None, ws=None) == 0
    assert ids(n_q=0, ids=None, bits=None) == 0 and ids(n=0, ids=None, bits=None) == 0
    for kw in (dict(rows=-1), dict(n=-1), dict(mask=None), dict(words=None), dict(words=FAKE + 2), dict(ld_mask=99), dict(ld_words=3)):
        assert pack(**kw) == EINVAL, kw
        assert L.msim_last_error()
    both, neither = dict(pl=FAKE, ql=FAKE), dict(bits=None)
    half = (dict(bits=None, pl=FAKE), dict(bits=None, ql=FAKE))
    shared_bad = (dict(n_q=-1), dict(n=-1), dict(ld_words=-1), both, neither, *half, dict(bits=FAKE + 2), dict(bits=None, pl=FAKE + 2, ql=FAKE),
                  dict(bits=None, pl=FAKE, ql=FAKE + 1), dict(ld_words=3))
    for kw in (*shared_bad, dict(scores=None), dict(scores=FAKE + 2), dict(ld=99)):
        assert mask(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (*shared_bad, dict(m_cap=-1), dict(cand=None), dict(counts=None), dict(ws=None), dict(cand=FAKE + 4), dict(counts=FAKE + 2),
               dict(ws=FAKE + 8), dict(ld_cand=9)):
        assert lst(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (*shared_bad, dict(m=-1), dict(ids=None), dict(ids=FAKE + 4), dict(ld=9)):
        assert ids(**kw) == EINVAL, kw
        assert L.msim_last_error()
    assert mask(n=1 << 31, ld=1 << 31) == EUNSUPPORTED and lst(n=1 << 31) == EUNSUPPORTED


# ------------------------------------------------------------------------------------------ injected stand-ins for the kernels
def _page(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _score_fn(queries, corpus):
    from oracle import maxsim_oracle as mo

    s = mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None)
    s[:, np.diff(corpus.offsets.numpy()) == 0] = -np.inf                # a page of 0 rows, as the scan kernels score it
    return torch.from_numpy(s)


def _rerank_fn(queries, corpus, candidates):
    full = _score_fn(queries, corpus)
    n = full.shape[1]
    d = candidates - corpus.id_base
    ok = (candidates >= 0) & (d >= 0) & (d < n)
    got = torch.gather(full, 1, d.clamp(0, n - 1))
    return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))


def _pack_fn(m2):
    return torch.from_numpy(ft.pack(m2.numpy()).view(np.int32))


def _ok(flt, n_q, alive):
    return ft.with_alive(ft.allowed(ft.spec_of(flt, n_q), n_q, len(flt)), None if alive is None else alive.numpy())


class Hooks:
    """the restatement behind the three filter hooks, counting the calls"""

    def __init__(self):
        self.calls = {"mask": 0, "list": 0, "ids": 0}
        self.reranked = []

    def mask(self, scores, flt, alive):
        self.calls["mask"] += 1
        return torch.from_numpy(ft.masked(scores.numpy(), _ok(flt, scores.shape[0], alive)))

    def list(self, flt, n_q, m_cap, alive):
        self.calls["list"] += 1
        cand, counts, status = ft.list_truth(_ok(flt, n_q, alive), m_cap, flt.id_base)
        assert status == 0
        return torch.from_numpy(cand), torch.from_numpy(counts), torch.tensor([status], dtype=torch.int32)

    def ids(self, ids, flt, alive):
        self.calls["ids"] += 1
        return torch.from_numpy(ft.ids_truth(ids.numpy(), _ok(flt, ids.shape[0], alive), flt.id_base))

    def rerank(self, queries, corpus, candidates):
        self.reranked.append(candidates.clone())
        return _rerank_fn(queries, corpus, candidates)

    def kw(self):
        from oracle import topk_oracle

        return dict(score_fn=_score_fn, rerank_fn=self.rerank, select=topk_oracle.torch_select, filter_mask_fn=self.mask,
                    filter_list_fn=self.list, filter_ids_fn=self.ids)


def _case(seed=0, n=41, n_q=5, id_base=100, dtype=torch.bfloat16):
    import colpali_amd as amd

    g = torch.Generator().manual_seed(seed)
    pages = [_page(g, int(k), dtype=dtype) for k in torch.randint(1, 12, (n,), generator=g)]
    pages[7] = pages[3].clone()                                          # an exact tie
    pages[5] = pages[5][:0]                                              # a page of 0 rows
    corpus = amd.pack_passages(pages, CPU, batch_size=None, id_base=id_base)
    q = torch.stack([_page(g, 6, dtype=dtype) for _ in range(n_q)])
    return amd, g, pages, corpus, q


def _specs(g, n_q, n):
    r = np.random.default_rng(int(torch.randint(0, 1 << 30, (1,), generator=g)))
    shared = r.random(n) < 0.15
    shared[[3, 5, 7]] = True                                             # the tie and the 0-row page are allowed
    per = r.random((n_q, n)) < 0.15
    per[1] = False                                                       # a query with no allowed page
    per[2, :] = False
    per[2, [5, 9]] = True                                                # k larger than the allowed count, one of them a 0-row page
    labels = (r.integers(0, 8, n).astype(np.int32), r.integers(0, 8, n_q).astype(np.int32))
    labels[1][0] = 99                                                    # a label no page carries
    return [("shared", shared), ("per_query", per), ("labels", *labels)]


def _filter(amd, spec, id_base):
    if spec[0] == "labels":
        return amd.PageFilter.from_labels(torch.from_numpy(spec[1]), torch.from_numpy(spec[2]), id_base)
    return amd.PageFilter.from_mask(torch.from_numpy(np.asarray(spec[1])), id_base, pack_fn=_pack_fn)


# ----------------------------------------------------------------------------------------------------------------- PageFilter
def test_page_filter_forms_errors_and_max_allowed():
    import colpali_amd as amd

    PF = amd.PageFilter
    m = torch.zeros((3, 70), dtype=torch.bool)
    m[0, :5] = True
    m[2, 10:40] = True
    f = PF.from_mask(m, 9, pack_fn=_pack_fn)
    assert len(f) == 70 and f.id_base == 9 and f.rows == 3 and not f.shared and f.words.shape == (3, 3) and f.max_allowed is None
    assert f.prepare() is f and f.max_allowed == 30 and f.prepare().max_allowed == 30
    s = PF.from_mask(m[2].to(torch.uint8) * 7, pack_fn=_pack_fn)         # uint8: non-zero is allowed
    assert s.shared and s.rows is None and s.prepare().max_allowed == 30 and s.id_base == 0
    strided = torch.zeros((3, 100), dtype=torch.bool)
    strided[:, :70] = m
    assert torch.equal(PF.from_mask(strided[:, :70], pack_fn=_pack_fn).words, f.words)       # any row stride
    full = PF.from_mask(torch.ones(64, dtype=torch.bool), pack_fn=_pack_fn).prepare()
    assert full.max_allowed == 64 and full.words.view(-1).tolist() == [-1, -1]               # all 32 bits of an int32 word
    lab = PF.from_labels(torch.tensor([1, 2, 2, 3, 2], dtype=torch.int32), torch.tensor([3, 2, 7], dtype=torch.int32), 4)
    assert len(lab) == 5 and lab.rows == 3 and lab.prepare().max_allowed == 3
    assert PF.from_labels(torch.tensor([1, 1], dtype=torch.int32), torch.tensor([7], dtype=torch.int32)).prepare().max_allowed == 0
    for bad in (m.float(), m.to(torch.int32), m[None], torch.zeros((), dtype=torch.bool), m.t(), m[:0], [True, False]):
        with pytest.raises(ValueError):
            PF.from_mask(bad, pack_fn=_pack_fn)
    with pytest.raises(ValueError):                                      # the packing is a gfx950 kernel: no CPU fallback
        PF.from_mask(m)
    i32 = torch.zeros(5, dtype=torch.int32)
    for a, b in ((i32.long(), i32), (i32, i32.float()), (i32[None], i32), (i32, i32[None]), ([0], i32)):
        with pytest.raises(ValueError):
            PF.from_labels(a, b)
    with pytest.raises(ValueError):
        PF(5, 0)
    with pytest.raises(ValueError):
        PF(5, 0, words=torch.zeros((1, 1), dtype=torch.int32), page_labels=i32, query_labels=i32)
    for fn, args in ((amd.filter.filter_mask, (torch.zeros(3, 70), f)), (amd.filter.filter_list, (f, 3, 4)),
                     (amd.filter.filter_ids, (torch.zeros((3, 4), dtype=torch.int64), f))):
        with pytest.raises(ValueError):                                  # the kernels have no CPU fallback
            fn(*args)


# ------------------------------------------------------------------------------------- ShardedRetriever.search(filter=), host logic
@pytest.mark.parametrize("k", [4, 50])
def test_both_routes_equal_the_truth(k):
    amd, g, pages, corpus, q = _case()
    n, n_q = len(corpus), len(q)
    s = _score_fn(q, corpus).numpy()
    assert np.isneginf(s[:, 5]).all() and (s[:, 3] == s[:, 7]).all()
    for spec in _specs(g, n_q, n):
        h = Hooks()
        r = amd.ShardedRetriever(corpus, **h.kw())
        want_s, want_i = ft.search_truth(s, ft.allowed(spec, n_q, n), k, 100)
        for route in ("mask", "list", "auto"):
            got_s, got_i = r.search(q, k, filter=_filter(amd, spec, 100), filter_route=route)
            np.testing.assert_array_equal(got_i.numpy(), want_i, err_msg=f"{spec[0]} {route}")
            np.testing.assert_array_equal(got_s.numpy(), want_s, err_msg=f"{spec[0]} {route}")
        assert h.calls["mask"] >= 1 and h.calls["list"] >= 1 and h.calls["ids"] == 0
        assert (want_i[np.isneginf(want_s)] == -1).all() and 105 not in want_i          # the allowed 0-row page is (-inf, -1)
    assert torch.equal(r.search(q, k)[1], amd.ShardedRetriever(corpus, **Hooks().kw()).search(q, k, filter=None)[1])


def test_routing_rules_of_auto_and_argument_errors():
    amd, g, pages, corpus, q = _case(seed=1, n=40)
    n, n_q = 40, len(q)
    frac = amd.filter.LIST_ROUTE_MAX_FRACTION
    assert 0 < frac <= 0.2

    def route_taken(mask_row, corpus=corpus, q=q, **kw):
        h = Hooks()
        amd.ShardedRetriever(corpus, **h.kw()).search(q, 3, filter=amd.PageFilter.from_mask(mask_row, corpus.id_base, pack_fn=_pack_fn), **kw)
        return h.calls

    at = torch.zeros(n, dtype=torch.bool)
    at[:int(n * frac)] = True                                            # max_allowed == n x fraction: the list route
    above = at.clone()
    above[-1] = True
    assert route_taken(at) == {"mask": 0, "list": 1, "ids": 0}
    assert route_taken(above) == {"mask": 1, "list": 0, "ids": 0}
    assert route_taken(above, filter_route="list")["list"] == 1 and route_taken(at, filter_route="mask")["mask"] == 1
    cand = torch.randint(100, 140, (n_q, 6), generator=g)
    assert route_taken(at, candidates=cand) == {"mask": 0, "list": 0, "ids": 1}
    assert route_taken(at, prefilter=corpus, n_candidates=4) == {"mask": 1, "list": 0, "ids": 0}
    # formats: an fp32 shard, a 256-wide one and queries of more than 128 tokens take the mask route; "list" refuses them as rerank does
    c32 = amd.pack_passages([p.float() for p in pages], CPU, batch_size=None, id_base=100)
    assert route_taken(at, corpus=c32, q=q.float())["mask"] == 1
    long_q = torch.cat([q] * 22, dim=1)
    assert long_q.shape[1] > 128 and route_taken(at, q=long_q)["mask"] == 1
    for kw in (dict(corpus=c32, q=q.float()), dict(q=long_q)):
        with pytest.raises(NotImplementedError):
            route_taken(at, filter_route="list", **kw)
    r = amd.ShardedRetriever(corpus, **Hooks().kw())
    f = amd.PageFilter.from_mask(at, 100, pack_fn=_pack_fn)
    for kw in (dict(filter_route="lists"), dict(filter_route="list", candidates=cand), dict(filter_route="list", prefilter=corpus, n_candidates=3)):
        with pytest.raises(ValueError):
            r.search(q, 3, filter=f, **kw)
    with pytest.raises(ValueError):
        r.search(q, 3, filter_route="mask")                              # goes with filter=
    for bad in (amd.PageFilter.from_mask(at, 0, pack_fn=_pack_fn), amd.PageFilter.from_mask(at[:-1], 100, pack_fn=_pack_fn),
                amd.PageFilter.from_mask(at.repeat(n_q + 1, 1), 100, pack_fn=_pack_fn), at,
                amd.PageFilter.from_labels(torch.zeros(n, dtype=torch.int32), torch.zeros(n_q - 1, dtype=torch.int32), 100)):
        for kw in (dict(), dict(candidates=cand), dict(prefilter=corpus, n_candidates=3)):
            with pytest.raises(ValueError):
                r.search(q, 3, filter=bad, **kw)


def test_two_stage_search_never_reranks_a_disallowed_page():
    amd, g, pages, corpus, q = _case(seed=2)
    n, n_q = len(corpus), len(q)
    pooled = amd.pack_passages([p[:2] for p in pages], CPU, batch_size=None, id_base=100)
    coarse, exact = _score_fn(q, pooled).numpy(), _score_fn(q, corpus).numpy()
    for spec in _specs(g, n_q, n):
        ok = ft.allowed(spec, n_q, n)
        h = Hooks()
        r = amd.ShardedRetriever(corpus, **h.kw())
        n_cand = int(ok.sum(1)[ok.sum(1) > 0].min()) + 3                 # larger than the smallest allowed set
        got_s, got_i = r.search(q, 4, prefilter=pooled, n_candidates=n_cand, filter=_filter(amd, spec, 100))
        want_s, want_i = ft.two_stage_truth(coarse, exact, ok, n_cand, 4, 100)
        np.testing.assert_array_equal(got_i.numpy(), want_i)
        np.testing.assert_array_equal(got_s.numpy(), want_s)
        (listed,) = h.reranked
        assert listed.shape == (n_q, n_cand) and (listed == -1).any()
        for row, allowed_row in zip(listed.numpy(), ok):
            assert allowed_row[row[row >= 0] - 100].all()
        cand = torch.randint(95, 100 + n + 5, (n_q, 12), generator=g)
        cand[0, 0] = -1
        before = cand.clone()
        got_s, got_i = r.search(q, 4, candidates=cand, filter=_filter(amd, spec, 100))
        assert torch.equal(cand, before)                                 # the caller's list is not written
        rs, ri = _rerank_fn(q, corpus, torch.from_numpy(ft.ids_truth(cand.numpy(), ok, 100)))
        from oracle import topk_oracle

        want_s, want_i = topk_oracle.topk(rs.numpy(), 4, 0, ri.numpy())
        want_i = np.where(np.isneginf(want_s), -1, want_i)
        np.testing.assert_array_equal(got_i.numpy(), want_i)
        np.testing.assert_array_equal(got_s.numpy(), want_s)


# --------------------------------------------------------------------------------------------- LiveCorpus.search(filter=), host logic
def test_live_corpus_deleted_and_filtered():
    import colpali_amd as amd
    from tests import live_truth

    g = torch.Generator().manual_seed(5)
    pages = [_page(g, int(k)) for k in torch.randint(1, 9, (30,), generator=g)]
    h = Hooks()
    kw = h.kw()
    live = amd.LiveCorpus(300, 32, CPU, id_base=50, mask_fn=lambda s, a: torch.from_numpy(live_truth.mask(s.numpy(), a.numpy())), **kw)
    live.add(pages)
    deleted = list(range(0, 30, 3))
    live.delete([50 + d for d in deleted])
    q = torch.stack([_page(g, 6) for _ in range(4)])
    s = _score_fn(q, live.view()).numpy()
    alive = np.ones(30, dtype=np.uint8)
    alive[deleted] = 0
    for spec in _specs(g, 4, 30):
        ok = ft.with_alive(ft.allowed(spec, 4, 30), alive)
        want_s, want_i = ft.search_truth(s, ok, 6, 50)
        for route in ("mask", "list"):
            got_s, got_i = live.search(q, 6, filter=_filter(amd, spec, 50), filter_route=route)
            np.testing.assert_array_equal(got_i.numpy(), want_i, err_msg=f"{spec[0]} {route}")
            np.testing.assert_array_equal(got_s.numpy(), want_s, err_msg=f"{spec[0]} {route}")
            assert not np.isin(got_i.numpy(), [50 + d for d in deleted]).any()
    assert h.calls["mask"] == 3 and h.calls["list"] == 3
    with pytest.raises(ValueError):
        live.search(q, 6, filter=amd.PageFilter.from_mask(torch.ones(32, dtype=torch.bool), 50, pack_fn=_pack_fn))    # the slots, not the capacity


# --------------------------------------------------------------------------------------------------------- sharded, over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _world_case(n_docs):
    g = torch.Generator().manual_seed(21)
    docs = [_page(g, n) for n in torch.randint(1, 20, (n_docs,), generator=g).tolist()]
    docs[4] = docs[n_docs - 3].clone()                                   # an exact tie across shards
    docs[6] = docs[6][:0]
    q = torch.stack([_page(g, 8) for _ in range(5)])
    specs = _specs(g, 5, n_docs)
    specs[0][1][[4, 6, n_docs - 3]] = True
    return docs, q, specs


def _shard_spec(spec, lo, hi):
    if spec[0] == "shared":
        return ("shared", spec[1][lo:hi])
    if spec[0] == "per_query":
        return ("per_query", np.ascontiguousarray(spec[1][:, lo:hi]))
    return ("labels", np.ascontiguousarray(spec[1][lo:hi]), spec[2])


def _worker(rank, world, port, n_docs, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import colpali_amd as amd

    docs, q, specs = _world_case(n_docs)
    lo, hi = amd.shard_range(n_docs, world, rank)
    shard = amd.pack_passages(docs[lo:hi], CPU, batch_size=None, id_base=lo)
    pooled = amd.pack_passages([d[:2] for d in docs[lo:hi]], CPU, batch_size=None, id_base=lo)
    r = amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, **Hooks().kw())
    out = {}
    for spec in specs:
        for route in ("mask", "list"):
            s, i = r.search(q, 6, filter=_filter(amd, _shard_spec(spec, lo, hi), lo), filter_route=route)
            out[f"{spec[0]}_{route}_s"], out[f"{spec[0]}_{route}_i"] = s.numpy(), i.numpy()
        s, i = r.search(q, 6, prefilter=pooled, n_candidates=9, filter=_filter(amd, _shard_spec(spec, lo, hi), lo))
        out[f"{spec[0]}_two_s"], out[f"{spec[0]}_two_i"] = s.numpy(), i.numpy()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs", [(2, 23), (3, 31)])
def test_sharded_filtered_search_equals_the_single_shard_truth(tmp_path, world, n_docs):
    import colpali_amd as amd

    mp.spawn(_worker, args=(world, _free_port(), n_docs, str(tmp_path)), nprocs=world, join=True)
    docs, q, specs = _world_case(n_docs)
    exact = _score_fn(q, amd.pack_passages(docs, CPU, batch_size=None)).numpy()
    coarse = _score_fn(q, amd.pack_passages([d[:2] for d in docs], CPU, batch_size=None)).numpy()
    for spec in specs:
        ok = ft.allowed(spec, 5, n_docs)
        want = {"mask": ft.search_truth(exact, ok, 6), "two": ft.two_stage_truth(coarse, exact, ok, 9, 6)}
        want["list"] = want["mask"]
        for rank in range(world):
            got = np.load(tmp_path / f"rank{rank}.npz")
            for name, (ws, wi) in want.items():
                np.testing.assert_array_equal(got[f"{spec[0]}_{name}_i"], wi, err_msg=f"rank {rank}: {spec[0]} {name}")
                np.testing.assert_array_equal(got[f"{spec[0]}_{name}_s"], ws, err_msg=f"rank {rank}: {spec[0]} {name}")
