"""Candidate reranking on the MI355X (msim_fwd_candidates, colpali_amd.rerank, ShardedRetriever.search(candidates= / prefilter=)).

The contract: for every listed id c inside the corpus, rerank(q, corpus, cand)[q, j] carries the BITS of
maxsim_scores(q, corpus)[q, c - id_base]; empty and out-of-corpus entries are (-inf, -1).
"""
import os
import socket

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16, base=None):
    x = torch.randn(n, 128, generator=g)
    if base is not None:
        x = x * 0.3 + base
    return torch.nn.functional.normalize(x, dim=-1).to(dtype)


def bits_to_bf16(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _gathered(full, cand, id_base):
    """The full scan restricted to the listed ids: (-inf, -1) where an entry is empty or off the corpus."""
    n = full.shape[1]
    c = cand.cpu()
    d = c - id_base
    ok = (c >= 0) & (d >= 0) & (d < n)
    rows = torch.arange(c.shape[0]).unsqueeze(1).expand_as(c)
    g = full.cpu()[rows, d.clamp(0, max(n - 1, 0))] if n else torch.zeros(c.shape)
    return torch.where(ok, g, torch.full_like(g, -float("inf"))), torch.where(ok, c, torch.full_like(c, -1))


def _check(amd, pq, corpus, cand, ref_rounding=False):
    full = amd.maxsim_scores(pq, corpus, ref_rounding=ref_rounding)
    got_s, got_i = amd.retrieval.rerank_scores(pq, corpus, cand, ref_rounding=ref_rounding)
    want_s, want_i = _gathered(full, cand, corpus.id_base)
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i.numpy())
    np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
    again = amd.rerank(pq, corpus, cand, ref_rounding=ref_rounding)
    np.testing.assert_array_equal(_bits(again), _bits(got_s))      # repeated calls: the same bits
    return full, got_s


def _ragged_case(dtype, id_base, seed=0):
    """Queries of 1 .. 128 tokens and two all-zero ones; documents of 0 .. 2100 rows, some of them negatively aligned with the
    queries, in one 128-document block so that the short ones carry clamp0."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(128, generator=g)
    qlens = [1, 15, 16, 17, 31, 32, 33, 127, 128, 5, 40, 9]
    qs = [_unit(g, n, dtype, base) for n in qlens]
    qs[9] = torch.zeros(7, 128, dtype=dtype)                        # compaction empties these two
    qs[10] = torch.zeros(40, 128, dtype=dtype)
    dlens = [0, 1, 31, 32, 33, 1024, 2100, 3, 64, 100, 17, 0, 250]
    ps = []
    for i, n in enumerate(dlens):
        ps.append(_unit(g, n, dtype, -base if i % 3 == 1 else None) if n else torch.zeros(0, 128, dtype=dtype))
    return qs, ps


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ref_rounding", [False, True])
def test_bit_identity_with_the_gathered_full_scan(amd, dtype, ref_rounding):
    qs, ps = _ragged_case(dtype, 0)
    for batch_size, id_base in ((128, 0), (128, 7000), (None, 123)):
        corpus = amd.pack_passages(ps, DEV, batch_size=batch_size, id_base=id_base)
        if batch_size:
            assert corpus.clamp0 is not None and int(corpus.clamp0.sum()) > 0
        pq = amd.pack_queries(qs, DEV)
        assert int(pq.lengths[9]) == 0 and int(pq.lengths[10]) == 0
        n = len(ps)
        g = torch.Generator().manual_seed(1)
        rows = []
        for q in range(len(qs)):
            ids = torch.randperm(n, generator=g)[:10] + id_base
            extra = torch.tensor([-1, id_base - 1, id_base + n, ids[0].item(), id_base + 6, id_base + 5])  # empty, off-corpus, duplicates
            rows.append(torch.cat([ids, extra]))
        cand = torch.stack(rows).to(DEV)
        full, got = _check(amd, pq, corpus, cand, ref_rounding)
        gs = got.cpu()
        assert torch.equal(gs[:, 0].view(torch.int32), gs[:, 13].view(torch.int32))       # the duplicate: identical bits
        assert bool(torch.isinf(gs[:, 10:13]).all())
        assert bool((gs[9] [gs[9] != -float("inf")] == 0).all())              # 0-token queries score 0


def test_negative_similarities_under_clamp0(amd):
    z = load_golden("score_negative_clamp.npz")
    q, short, long_ = (bits_to_bf16(z[k]) for k in ("q_bits", "short_bits", "long_bits"))
    pq = amd.pack_queries([q, q], DEV)
    for bs in (128, 1):
        corpus = amd.pack_passages([short, long_], DEV, batch_size=bs, id_base=40)
        cand = torch.tensor([[40, 41], [41, 40]], device=DEV)
        for rr in (False, True):
            _check(amd, pq, corpus, cand, rr)


def _corpus(amd, g, n, lens=(1, 300), dtype=torch.bfloat16, id_base=0):
    ln = torch.randint(lens[0], lens[1] + 1, (n,), generator=g).tolist()
    return amd.pack_passages([_unit(g, k, dtype) for k in ln], DEV, batch_size=None, id_base=id_base)


def _queries(amd, g, n, lens=(1, 64), dtype=torch.bfloat16):
    ln = torch.randint(lens[0], lens[1] + 1, (n,), generator=g).tolist()
    return amd.pack_queries([_unit(g, k, dtype) for k in ln], DEV)


def test_one_document_listed_by_a_thousand_queries(amd):
    g = torch.Generator().manual_seed(2)
    corpus = _corpus(amd, g, 40, (900, 1100), id_base=10)
    pq = _queries(amd, g, 1000, (1, 128))
    other = torch.randint(10, 50, (1000, 1), generator=g)
    cand = torch.cat([torch.full((1000, 2), 17), other], dim=1).to(DEV)
    _check(amd, pq, corpus, cand)


def test_every_document_listed_once(amd):
    g = torch.Generator().manual_seed(3)
    corpus = _corpus(amd, g, 300, (0, 200))
    pq = _queries(amd, g, 3)
    cand = torch.randperm(300, generator=g).view(3, 100).to(DEV)
    _check(amd, pq, corpus, cand)


def test_single_entry_and_single_query(amd):
    g = torch.Generator().manual_seed(4)
    corpus = _corpus(amd, g, 20)
    pq = _queries(amd, g, 1, (33, 33))
    _check(amd, pq, corpus, torch.tensor([[5]], device=DEV))
    _check(amd, pq, corpus, torch.randint(0, 20, (1, 50), generator=g).to(DEV))


def test_wide_candidate_lists_with_empty_rows_and_stride(amd):
    g = torch.Generator().manual_seed(5)
    corpus = _corpus(amd, g, 500, (0, 80), id_base=1_000_000)
    pq = _queries(amd, g, 3, (1, 128))
    cand = torch.randint(1_000_000 - 5, 1_000_500 + 5, (3, 4096), generator=g)
    cand[1] = -1                                                     # a row that lists nothing
    _check(amd, pq, corpus, cand.to(DEV))
    big = torch.randint(1_000_000, 1_000_500, (3, 4096 + 40), generator=g).to(DEV)
    strided = big[:, 7:7 + 4096]
    assert strided.stride(0) == 4096 + 40
    _check(amd, pq, corpus, strided)
    allneg = torch.full((3, 8), -1, dtype=torch.int64, device=DEV)
    s = amd.rerank(pq, corpus, allneg)
    assert bool(torch.isinf(s).all() and (s < 0).all())


def test_dense_query_box_and_host_list(amd):
    g = torch.Generator().manual_seed(6)
    corpus = _corpus(amd, g, 50)
    qs = [_unit(g, 20) for _ in range(4)]
    cand = torch.randint(0, 50, (4, 12), generator=g).to(DEV)
    pq = amd.pack_queries(qs, DEV)
    want = amd.rerank(pq, corpus, cand)
    np.testing.assert_array_equal(_bits(amd.rerank(qs, corpus, cand)), _bits(want))
    np.testing.assert_array_equal(_bits(amd.rerank(torch.stack(qs).to(DEV), corpus, cand)), _bits(want))


def _truth_topk(full, cand, id_base, k):
    from oracle import topk_oracle

    s, i = _gathered(full, cand, id_base)
    return topk_oracle.topk(s.numpy(), k, 0, i.numpy())


def test_topk_of_the_listed_documents(amd):
    g = torch.Generator().manual_seed(7)
    corpus = _corpus(amd, g, 200, id_base=300)
    pq = _queries(amd, g, 9, (1, 128))
    cand = torch.stack([torch.randperm(200, generator=g)[:60] + 300 for _ in range(9)])
    cand[3, 5:] = -1                                                 # five valid entries, k = 10: padded
    cand[4, :] = 9999
    cand = cand.to(DEV)
    full = amd.maxsim_scores(pq, corpus)
    for k in (1, 10, 60, 70):
        s, i = amd.rerank(pq, corpus, cand, k)
        ws, wi = _truth_topk(full, cand, 300, k)
        np.testing.assert_array_equal(i.cpu().numpy(), wi)
        np.testing.assert_array_equal(_bits(s), ws.view(np.int32))
    s, i = amd.rerank(pq, corpus, cand, 10)
    assert (i[3, 5:] == -1).all() and torch.isinf(s[3, 5:]).all() and (i[4] == -1).all()


@pytest.fixture(scope="module")
def dist():
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


def _two_stage_case(amd, seed=8):
    g = torch.Generator().manual_seed(seed)
    full_pages = [_unit(g, int(n)) for n in torch.randint(100, 400, (300,), generator=g)]
    full = amd.pack_passages(full_pages, DEV, batch_size=None, id_base=50)
    pooled = amd.pack_passages([p[::3].contiguous() for p in full_pages], DEV, batch_size=None, id_base=50)
    pq = _queries(amd, g, 12, (1, 128))
    return full, pooled, pq


def test_sharded_search_with_candidates_and_prefilter(amd, dist):
    full, pooled, pq = _two_stage_case(amd)
    g = torch.Generator().manual_seed(9)
    cand = torch.randint(40, 360, (12, 30), generator=g).to(DEV)
    want = amd.rerank(pq, full, cand, 10)
    for force in (False, True):
        r = amd.ShardedRetriever(full, world=1, rank=0, dist=dist, force_collective=force)
        s, i = r.search(pq, k=10, candidates=cand)
        np.testing.assert_array_equal(i.cpu().numpy(), want[1].cpu().numpy())
        np.testing.assert_array_equal(_bits(s), _bits(want[0]))
    # two-stage: search(prefilter=P, n_candidates=m) == rerank(full, topk(maxsim_scores(q, P), m).ids, k)
    for m in (1, 25, 400):
        _, ci = amd.topk(amd.maxsim_scores(pq, pooled), m, pooled.id_base)
        ws, wi = amd.rerank(pq, full, ci, 10)
        for force in (False, True):
            r = amd.ShardedRetriever(full, world=1, rank=0, dist=dist, force_collective=force)
            s, i = r.search(pq, k=10, prefilter=pooled, n_candidates=m)
            np.testing.assert_array_equal(i.cpu().numpy(), wi.cpu().numpy())
            np.testing.assert_array_equal(_bits(s), _bits(ws))


def _capture(fn):
    """fn() once eagerly, warm-up on a side stream, then captured: returns (eager outputs, captured outputs, graph)."""
    eager = [t.clone() for t in fn()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # warm-up on a side stream, as torch.cuda.graph expects
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fn()
    return eager, captured, graph


def _replay_equals(eager, captured, graph):
    for _ in range(2):
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            np.testing.assert_array_equal(got.cpu().numpy().view(np.int32 if got.dtype == torch.float32 else np.int64),
                                          want.cpu().numpy().view(np.int32 if want.dtype == torch.float32 else np.int64))


def test_captured_rerank_replays_the_eager_bits(amd):
    full, _, pq = _two_stage_case(amd, 10)
    g = torch.Generator().manual_seed(11)
    cand = torch.randint(40, 360, (12, 40), generator=g).to(DEV)
    _replay_equals(*_capture(lambda: (amd.rerank(pq, full, cand),) + tuple(amd.rerank(pq, full, cand, 10))))


def test_captured_two_stage_search_replays_the_eager_bits(amd):
    full, pooled, pq = _two_stage_case(amd, 12)
    r = amd.ShardedRetriever(full)
    _replay_equals(*_capture(lambda: r.search(pq, k=10, prefilter=pooled, n_candidates=30)))


def test_shared_candidate_list_broadcast_to_every_query(amd):
    g = torch.Generator().manual_seed(13)
    corpus = _corpus(amd, g, 60, id_base=5)
    pq = _queries(amd, g, 7, (1, 128))
    row = torch.randint(0, 70, (25,), generator=g).to(DEV)
    shared = row.expand(7, 25)
    assert shared.stride(0) == 0
    _check(amd, pq, corpus, shared)


def test_device_offsets_that_disagree_with_the_host_copy_poison_the_call(amd):
    """The call validates q_off_host; a device q_off that says otherwise must not be trusted as an address: every score is NaN."""
    g = torch.Generator().manual_seed(14)
    corpus = _corpus(amd, g, 30)
    pq = _queries(amd, g, 3, (20, 20))
    bad = amd.PackedQueries(tokens=pq.tokens, offsets=torch.tensor([0, 20, 40, 300], dtype=torch.int32, device=DEV),
                            offsets_host=pq.offsets_host)
    s = amd.rerank(bad, corpus, torch.randint(0, 30, (3, 9), generator=g).to(DEV))
    assert bool(torch.isnan(s).all())


def test_error_paths(amd):
    g = torch.Generator().manual_seed(12)
    corpus = _corpus(amd, g, 10)
    pq = _queries(amd, g, 2)
    cand = torch.randint(0, 10, (2, 4), generator=g).to(DEV)
    with pytest.raises(RuntimeError):                                  # dtype mismatch
        amd.rerank([_unit(g, 8, torch.float16)] * 2, corpus, cand)
    with pytest.raises(NotImplementedError):                           # fp32
        c32 = amd.pack_passages([torch.randn(5, 128)] * 10, DEV, batch_size=None)
        amd.rerank([torch.randn(8, 128)] * 2, c32, cand)
    with pytest.raises(NotImplementedError):                           # width != 128
        c96 = amd.pack_passages([_unit(g, 5)[:, :96].contiguous()] * 10, DEV, batch_size=None)
        amd.rerank([_unit(g, 8)[:, :96].contiguous()] * 2, c96, cand)
    with pytest.raises(NotImplementedError):                           # a query over 128 tokens
        amd.rerank([_unit(g, 129), _unit(g, 4)], corpus, cand)
    for bad in (cand.to(torch.int32), cand.cpu(), cand[0], cand[:1]):
        with pytest.raises(ValueError):
            amd.rerank(pq, corpus, bad)
    with pytest.raises(RuntimeError):                                  # a CPU corpus: the GPU-only error
        amd.rerank([_unit(g, 8)] * 2, amd.pack_passages([_unit(g, 5)] * 10, torch.device("cpu"), batch_size=None), cand.cpu())
    r = amd.ShardedRetriever(corpus)
    other = _corpus(amd, g, 11)
    with pytest.raises(ValueError):
        r.search(pq, k=3, prefilter=other, n_candidates=4)
    shifted = amd.pack_passages([_unit(g, 5)] * 10, DEV, batch_size=None, id_base=1)
    with pytest.raises(ValueError):
        r.search(pq, k=3, prefilter=shifted, n_candidates=4)
    with pytest.raises(ValueError):
        r.search(pq, k=3, prefilter=corpus)                            # no n_candidates
    with pytest.raises(ValueError):
        r.search(pq, k=3, prefilter=corpus, n_candidates=4, candidates=cand)
    with pytest.raises(ValueError):
        r.search(pq, k=3, n_candidates=4)                              # n_candidates without prefilter=
