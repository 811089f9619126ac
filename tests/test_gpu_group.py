"""Document-level search on the MI355X (colpali_amd.PageGroups, msim_group_reduce / msim_group_select, `search(group_by=)`).

Every comparison is exact (bits, ids).  The kernels only move scores and ids: synthetic score matrices on a coarse grid (many exact
ties, -inf, both zeros) go to the numpy restatement in tests/group_truth.py; end to end, the scores of the unchanged scan and rerank
kernels are fetched to the host and fed to the same restatement.  The shapes are the edges of the kernels: documents around the wave
width and around both switch-over lengths of include/maxsim.h, one document holding every page, interleaved and permuted
documents, score rows that are not 16-byte aligned, candidate rows around the power of two the selection sorts.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import filter_truth as ft
from tests import group_truth as gt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 12345.0
NINF = -np.inf
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _header_constant(name):
    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))


T_THREAD = _header_constant("MSIM_GROUP_THREAD_MAX")
T_WAVE = _header_constant("MSIM_GROUP_WAVE_MAX")


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _grid(r, n_q, n, negative=False):
    s = r.integers(-6, 7, size=(n_q, n)).astype(np.float32) / 4          # multiples of 1/4: many exact ties
    if negative:
        s = -np.abs(s) - np.float32(0.25)
    s[r.random((n_q, n)) < 0.1] = -np.inf
    if not negative:
        s[(s == 0) & (r.random((n_q, n)) < 0.5)] = -0.0
    return s


# --------------------------------------------------------------------------------------------------------------- group_reduce
def _reduce_check(amd, s, labels, id_base=0, pad=0, shift=0):
    """scores `s` in a sentinel-filled buffer of row stride n + pad starting `shift` floats in; outputs in sentinel-filled buffers of
    row stride G + 3, through the C ABI, so that a store outside [n_q, G] shows"""
    n_q, n = s.shape
    ld = n + pad
    buf = torch.full((n_q * ld + shift,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[shift:].view(n_q, ld)[:, :n]
    view.copy_(torch.from_numpy(s))
    groups = amd.PageGroups.from_labels(torch.from_numpy(labels).to(DEV), id_base)
    gids, want_s, want_p = gt.reduce_truth(s, labels, id_base)
    got_s, got_p = amd.group_reduce(view, groups)
    assert groups.group_ids.cpu().tolist() == gids.tolist() and groups.max_group == int(np.bincount(np.unique(labels, return_inverse=True)[1]).max())
    np.testing.assert_array_equal(got_p.cpu().numpy(), want_p)
    np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32))
    np.testing.assert_array_equal(_bits(buf[shift:].view(n_q, ld)[:, :n]), s.view(np.int32))          # the scores are only read
    g = len(gids)
    ld_out = g + 3
    out_s = torch.full((n_q + 1, ld_out), SENTINEL, dtype=torch.float32, device=DEV)
    out_p = torch.full((n_q + 1, ld_out), -77, dtype=torch.int64, device=DEV)
    L = amd._lib.lib()
    rc = L.msim_group_reduce(view.data_ptr(), ld, n_q, n, groups.offsets.data_ptr(), groups.pages.data_ptr(), g, id_base,
                             out_s.data_ptr(), out_p.data_ptr(), ld_out, torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, L.msim_last_error()
    np.testing.assert_array_equal(_bits(out_s[:n_q, :g]), want_s.view(np.int32))
    np.testing.assert_array_equal(out_p[:n_q, :g].cpu().numpy(), want_p)
    assert (out_s[:, g:] == SENTINEL).all() and (out_s[n_q] == SENTINEL).all() and (out_p[:, g:] == -77).all() and (out_p[n_q] == -77).all()
    return want_s, want_p


def _labels_of_sizes(sizes, r, shuffle=False):
    labels = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 + 3, sizes)
    return r.permutation(labels) if shuffle else labels


def test_reduce_documents_around_the_wave_and_both_switch_over_lengths(amd):
    sizes = [1, 63, 64, 65, T_THREAD - 1, T_THREAD, T_THREAD + 1, T_WAVE - 1, T_WAVE, T_WAVE + 1, 2, 1]
    r = np.random.default_rng(1)
    for shuffle in (False, True):                                        # contiguous documents, then their pages scattered
        labels = _labels_of_sizes(sizes, r, shuffle)
        s = _grid(r, 3, labels.size)
        _reduce_check(amd, s, labels, id_base=1000)
    s[:, labels == 3 + 7 * 8] = -np.inf                                  # the T_WAVE document, and a one-page one, all -inf
    s[:, labels == 3] = -np.inf
    want_s, want_p = _reduce_check(amd, s, labels)
    assert (want_p[:, [0, 8]] == -1).all() and np.isneginf(want_s[:, [0, 8]]).all()


@pytest.mark.parametrize("n_q", [1, 70])
def test_reduce_one_page_one_document_and_single_pages(amd, n_q):
    r = np.random.default_rng(2 + n_q)
    _reduce_check(amd, _grid(r, n_q, 1), np.zeros(1, dtype=np.int64), id_base=5)           # n = 1
    n = 700
    _reduce_check(amd, _grid(r, n_q, n), np.arange(n, dtype=np.int64)[::-1].copy())         # one page per document, ids descending
    _reduce_check(amd, _grid(r, n_q, n), np.arange(n, dtype=np.int64) % 3)                  # page p in document p % 3
    _reduce_check(amd, _grid(r, n_q, n, negative=True), np.arange(n, dtype=np.int64) // 9)  # every score negative


def test_reduce_one_document_of_5000_pages_and_40_permuted_documents(amd):
    r = np.random.default_rng(4)
    s = _grid(r, 4, 5000)
    s[0, :4000] = -np.inf                                                # the winner sits late in the list
    s[1] = 0.25                                                          # one long tie: the lowest page wins
    want_s, want_p = _reduce_check(amd, s, np.full(5000, 9, dtype=np.int64), id_base=77)
    assert want_p[1, 0] == 77 and want_s.shape == (4, 1)
    _reduce_check(amd, _grid(r, 5, 3000), r.integers(0, 40, 3000).astype(np.int64))
    _reduce_check(amd, _grid(r, 5, 3000, negative=True), r.integers(0, 40, 3000).astype(np.int64))


def test_reduce_rows_off_16_byte_alignment(amd):
    r = np.random.default_rng(5)
    sizes = [1, 5, T_THREAD + 3, 70, 300, T_WAVE + 9, 2]
    labels = _labels_of_sizes(sizes, r, shuffle=True)
    s = _grid(r, 6, labels.size)
    assert torch.empty(1, device=DEV).data_ptr() % 16 == 0
    _reduce_check(amd, s, labels, id_base=3, pad=3, shift=1)             # stride n + 3, the base 4 bytes off 16-byte alignment
    _reduce_check(amd, s, labels, pad=3)


# --------------------------------------------------------------------------------------------------------------- group_select
def _select_rows(r, m):
    """seven rows of (score, document, page) triples, one per pattern"""
    base = _grid(r, 7, m)
    gid = r.integers(0, max(m // 3, 1), size=(7, m)).astype(np.int64) * 5
    page = np.stack([r.permutation(m) for _ in range(7)]).astype(np.int64) + 100
    gid[0] = 42                                                          # every entry one document
    gid[1] = r.permutation(m) + 1000                                     # every entry its own document
    gid[2, r.permutation(m)[:(m + 1) // 2]] = -1                         # half carry id -1
    base[3] = 0.5                                                        # equal scores inside a document: the page decides ...
    gid[4] = r.permutation(m)                                            # ... and across documents: the document id decides
    base[4] = 1.25
    base[5] = -np.inf                                                    # a row of only -inf
    gid[6, ::2] = -1
    base[6, 1::2][r.random(base[6, 1::2].shape) < 0.5] = -np.inf         # either kind of "no entry"
    return base, gid, page


@pytest.mark.parametrize("m", [1, 63, 64, 65, 4095, 4096])
def test_select_equals_the_restatement(amd, m):
    r = np.random.default_rng(m)
    s, gid, page = _select_rows(r, m)
    ds, dg, dp = (torch.from_numpy(x).to(DEV) for x in (s, gid, page))
    for k in (1, 10, 1024):
        want = gt.select_truth(s, gid, page, k)
        got = amd.group_select(ds, dg, dp, k)
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1], err_msg=f"m={m} k={k}")
        np.testing.assert_array_equal(got[2].cpu().numpy(), want[2], err_msg=f"m={m} k={k}")
        np.testing.assert_array_equal(_bits(got[0]), want[0].view(np.int32), err_msg=f"m={m} k={k}")
        assert (want[1][5] == -1).all() and (want[1][0, 1:] == -1).all() and want[1][0, 0] == 42
    out = (torch.full((8, 10), SENTINEL, dtype=torch.float32, device=DEV), torch.full((8, 10), -77, dtype=torch.int64, device=DEV),
           torch.full((8, 10), -77, dtype=torch.int64, device=DEV))
    want = gt.select_truth(s, gid, page, 10)
    got = amd.group_select(ds, dg, dp, 10, out=tuple(t[:7] for t in out))            # writes the caller's tensors, and only them
    assert got[0].data_ptr() == out[0].data_ptr()
    for t, w, fill in zip(out, want, (SENTINEL, -77, -77)):
        np.testing.assert_array_equal(t[:7].cpu().numpy(), w)
        assert (t[7] == fill).all()
    wide = torch.zeros((7, 2 * m + 3), dtype=torch.float32, device=DEV)              # a strided view is made contiguous
    wide[:, :m] = ds
    got = amd.group_select(wide[:, :m], dg, dp, 10)
    np.testing.assert_array_equal(got[2].cpu().numpy(), want[2])


def test_select_limits_and_empty_rows(amd):
    z = torch.zeros((2, 4097), dtype=torch.float32, device=DEV)
    i = torch.zeros((2, 4097), dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError):
        amd.group_select(z, i, i, 5)
    with pytest.raises(NotImplementedError):
        amd.group_select(z[:, :10].contiguous(), i[:, :10].contiguous(), i[:, :10].contiguous(), 1025)
    got = amd.group_select(z[:, :0], i[:, :0], i[:, :0], 3)
    assert np.isneginf(got[0].cpu().numpy()).all() and (got[1] == -1).all() and (got[2] == -1).all()
    with pytest.raises(ValueError):
        amd.group_select(z[:, :5], i[:, :4], i[:, :5], 3)
    with pytest.raises(ValueError):
        amd.group_select(z[:, :5], i[:, :5].int(), i[:, :5], 3)


# --------------------------------------------------------------------------------------------------------------------- search
def _unit(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _search_case(dtype, dim, seed):
    """~300 ragged pages in ~45 documents of 1 .. 30 scattered pages: a page duplicated inside its document and across two documents
    (real ties), one 0-row page, one document whose only page has 0 rows; 5 ragged queries"""
    g = torch.Generator().manual_seed(seed)
    n = 301
    pages = [_unit(g, int(k), dim, dtype) for k in torch.randint(8, 81, (n,), generator=g)]
    labels = (torch.randint(0, 45, (n,), generator=g) * 3 + 2).to(torch.int64)
    pages[77] = pages[20].clone()
    labels[77] = labels[20] = 500                                        # the same page twice in one document: the lower id wins
    pages[150] = pages[33].clone()
    labels[150], labels[33] = 17, 20                                     # ... and in two documents: both score alike, 17 ranks first
    pages[10] = pages[10][:0]                                            # a 0-row page inside a document
    pages[200] = pages[200][:0]
    labels[200] = 9999                                                   # a document that is only a 0-row page
    qs = [_unit(g, int(k), dim, dtype) for k in (1, 17, 32, 33, 64)]
    return pages, labels, qs


class _FakeDist:
    """Stands in for torch.distributed inside one process: rank r's message is whatever virtual shard r produced."""

    def __init__(self, messages, me):
        self.messages, self.me = messages, me

    def all_gather_into_tensor(self, out, mine, group=None):
        self.messages[self.me] = mine.clone()
        out.copy_(torch.cat([m.reshape(-1) for m in self.messages]))


@pytest.fixture(scope="module")
def dist():
    import socket

    import torch.distributed as d

    created = False
    if not d.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        d.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        created = True
    yield d
    if created:
        d.destroy_process_group()


def _check(got, want, msg):
    assert len(got) == 3
    np.testing.assert_array_equal(got[1].cpu().numpy(), want[1], err_msg=f"{msg}: group ids")
    np.testing.assert_array_equal(got[2].cpu().numpy(), want[2], err_msg=f"{msg}: page ids")
    np.testing.assert_array_equal(_bits(got[0]), want[0].view(np.int32), err_msg=f"{msg}: scores")


@pytest.mark.parametrize("dtype,dim", [(torch.bfloat16, 128), (torch.float16, 320)])
def test_search_by_document_on_every_route(amd, dist, dtype, dim):
    pages, labels, qs = _search_case(dtype, dim, seed=dim)
    n, n_q, base = len(pages), len(qs), 40
    lab = labels.numpy()
    n_docs = len(set(lab.tolist()))
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=base)
    pooled = amd.pack_passages([p[::3].contiguous() for p in pages], DEV, batch_size=None, id_base=base)
    pq = amd.pack_queries(list(qs), DEV, layout="flat", compact=False)
    groups = amd.PageGroups.from_labels(labels.to(DEV), base)
    scan = amd.maxsim_scores(pq, corpus).cpu().numpy()
    every = (torch.arange(n, dtype=torch.int64, device=DEV) + base).repeat(n_q, 1)
    listed_scores = amd.retrieval.rerank_scores(pq, corpus, every)[0].cpu().numpy()      # what the list routes score with
    assert np.isneginf(scan[:, [10, 200]]).all() and (scan[:, 20] == scan[:, 77]).all() and (scan[:, 33] == scan[:, 150]).all()
    coarse = amd.maxsim_scores(pq, pooled).cpu().numpy()
    r1 = amd.ShardedRetriever(corpus)
    rc = amd.ShardedRetriever(corpus, world=1, rank=0, dist=dist, force_collective=True)
    rng = np.random.default_rng(3)
    shared = rng.random(n) < 0.3
    shared[[10, 20, 33, 77, 150, 200]] = True
    per = rng.random((n_q, n)) < 0.2
    per[1] = False
    gen = torch.Generator().manual_seed(8)
    cand = torch.stack([torch.randperm(n + 10, generator=gen)[:60] + base - 5 for _ in range(n_q)])
    cand[0, :3] = -1
    in_cand = np.zeros((n_q, n), dtype=bool)
    for q_, row in enumerate(cand.numpy()):
        in_cand[q_, row[(row >= base) & (row < base + n)] - base] = True
    _, kept = ft.search_truth(coarse, np.ones((n_q, n), dtype=bool), 50, base)
    in_kept = np.zeros((n_q, n), dtype=bool)
    for q_, row in enumerate(kept):
        in_kept[q_, row[row >= 0] - base] = True
    plain = r1.search(pq, 7)
    assert len(plain) == 2
    for k in (7, n_docs + 5):
        want = gt.search_truth(scan, lab, k, base)
        assert 9999 not in want[1] and (k == 7 or (want[1][:, -1] == -1).all())
        doc17 = np.argwhere(want[1] == 17)
        for q_, j in doc17:                                              # the cross-document tie: 17 right before 20, same score
            if j + 1 < k and want[1][q_, j + 1] == 20:
                assert want[0][q_, j] == want[0][q_, j + 1]
        for name, r in (("scan", r1), ("scan, forced collective", rc)):
            _check(r.search(pq, k, group_by=groups), want, f"{name} k={k}")
        _check(r1.search(qs, k, group_by=groups), want, "a host list of queries")
        for name, r in (("candidates", r1), ("candidates, forced collective", rc)):
            _check(r.search(pq, k, candidates=cand.to(DEV), group_by=groups), gt.search_truth(listed_scores, lab, k, base, in_cand), f"{name} k={k}")
        _check(r1.search(pq, k, prefilter=pooled, n_candidates=50, group_by=groups), gt.search_truth(listed_scores, lab, k, base, in_kept),
               f"prefilter k={k}")
        for spec in (("shared", shared), ("per_query", per)):
            ok = ft.allowed(spec, n_q, n)
            mask = torch.from_numpy(np.asarray(spec[1])).to(DEV)
            for route, scores in (("mask", scan), ("list", listed_scores)):
                want_f = gt.search_truth(scores, lab, k, base, ok)
                for name, r in ((route, r1), (route + ", forced collective", rc)):
                    got = r.search(pq, k, filter=amd.PageFilter.from_mask(mask, base), filter_route=route, group_by=groups)
                    _check(got, want_f, f"{spec[0]} {name} k={k}")
    # virtual shards: the answer does not depend on their number, with documents straddling every boundary
    want = gt.search_truth(scan, lab, 7, base)
    for world in (2, 3):
        shards = []
        for rank in range(world):
            lo, hi = amd.shard_range(n, world, rank)
            shards.append((amd.pack_passages(pages[lo:hi], DEV, batch_size=None, id_base=base + lo),
                           amd.PageGroups.from_labels(labels[lo:hi].to(DEV), base + lo)))
        nbytes = (n_q * 7 * 4 + 7) // 8 * 8 + 2 * n_q * 7 * 8
        messages = [torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(world)]
        for _ in range(2):                                               # the first pass fills every rank's message
            for rank, (shard, gr) in enumerate(shards):
                rr = amd.ShardedRetriever(shard, world=world, rank=rank, dist=_FakeDist(messages, rank))
                got = rr.search(pq, 7, group_by=gr)
        _check(got, want, f"world={world}")


def test_live_corpus_by_document(amd):
    g = torch.Generator().manual_seed(9)
    pages = [_unit(g, int(k)) for k in torch.randint(8, 41, (90,), generator=g)]
    qs = [_unit(g, k) for k in (8, 20, 5, 32)]
    pq = amd.pack_queries(list(qs), DEV, layout="flat", compact=False)
    n, n_q, base, k = 90, 4, 100, 7
    live = amd.LiveCorpus.from_packed(amd.pack_passages(pages[:60], DEV, batch_size=None, id_base=base), spare_rows=1500, spare_docs=40)
    live.add(pages[60:])
    labels = torch.arange(n, dtype=torch.int64) % 11 + 1
    labels[[2, 40, 88]] = 300                                            # a document that loses every page
    groups = amd.PageGroups.from_labels(labels.to(DEV), base).prepare()  # built after the last add, over all slots
    exact = amd.maxsim_scores(pq, live.view()).cpu().numpy()
    deleted = sorted({2, 40, 88} | set(range(1, 90, 4)) | {int(np.argmax(np.where(labels.numpy() == 5, exact[0], -np.inf)))})
    live.delete([base + d for d in deleted])
    alive = np.ones((n_q, n), dtype=bool)
    alive[:, deleted] = False
    mask = np.arange(n) % 3 != 0
    for step in ("deleted", "compacted"):
        want = gt.search_truth(exact, labels.numpy(), k, base, alive)
        assert 300 not in want[1] and not np.isin(want[2], [base + d for d in deleted]).any()
        _check(live.search(pq, k, group_by=groups), want, step)
        _check(live.search(pq, 20, group_by=groups), gt.search_truth(exact, labels.numpy(), 20, base, alive), step + " k=20")
        want_f = gt.search_truth(exact, labels.numpy(), k, base, alive & mask[None, :])
        for route in ("mask", "list"):
            flt = amd.PageFilter.from_mask(torch.from_numpy(mask).to(DEV), base)
            _check(live.search(pq, k, filter=flt, filter_route=route, group_by=groups), want_f, f"{step} {route}")
        live.compact()
    live.check()
    assert len(live.search(pq, k)) == 2


def test_graph_replay_reproduces_the_eager_call(amd, monkeypatch):
    pages, labels, qs = _search_case(torch.bfloat16, 128, seed=10)
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=10)
    pq = amd.pack_queries(list(qs), DEV, layout="flat", compact=False)
    r = amd.ShardedRetriever(corpus)
    fresh = amd.PageGroups.from_labels(labels.to(DEV), 10)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before the capture"):        # an unprepared PageGroups synchronises once
        r.search(pq, 7, group_by=fresh)
    monkeypatch.undo()
    groups = fresh.prepare()
    cand = (torch.arange(0, 120, dtype=torch.int64, device=DEV) * 2 + 10).repeat(len(qs), 1)
    for kw in (dict(), dict(candidates=cand)):
        eager = [t.clone() for t in r.search(pq, 7, group_by=groups, **kw)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = r.search(pq, 7, group_by=groups, **kw)
        for _ in range(2):
            for t in outs:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[1], eager[1]) and torch.equal(outs[2], eager[2])
            assert torch.equal(outs[0].view(torch.int32), eager[0].view(torch.int32))


def test_error_paths(amd):
    pages, labels, qs = _search_case(torch.bfloat16, 128, seed=11)
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=5)
    pq = amd.pack_queries(list(qs), DEV, layout="flat", compact=False)
    r = amd.ShardedRetriever(corpus)
    PG = amd.PageGroups
    for bad in (PG.from_labels(labels[:-1].to(DEV), 5), PG.from_labels(labels.to(DEV), 0), PG.from_labels(labels, 5), labels.to(DEV)):
        with pytest.raises(ValueError):
            r.search(pq, 3, group_by=bad)
    neg = labels.clone()
    neg[4] = -1
    with pytest.raises(ValueError, match="negative"):
        r.search(pq, 3, group_by=PG.from_labels(neg.to(DEV), 5))
    scores = torch.zeros((len(qs), len(pages)), dtype=torch.float32, device=DEV)
    good = PG.from_labels(labels.to(DEV), 5)
    with pytest.raises(ValueError):
        amd.group_reduce(scores[:, :-1], good)
    with pytest.raises(ValueError):
        amd.group_reduce(scores.cpu(), good)
    with pytest.raises(ValueError):
        amd.group_reduce(scores.double(), good)
