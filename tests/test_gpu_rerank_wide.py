"""Candidate reranking at width 320 (ColQwen3) on the MI355X: msim_fwd_candidates_wide, colpali_amd.rerank,
ShardedRetriever.search(candidates= / prefilter=) and LiveCorpus.search(candidates= / prefilter=).

The contract (include/maxsim.h): for every listed id c inside the corpus, rerank(q, corpus, cand)[q, j] carries the BITS the flat
panel kernel K1bPF gives maxsim_scores(q, corpus)[q, c - id_base]; empty and out-of-corpus entries are (-inf, -1).  A scan call of
ONE query length and at most four 32-token tiles runs K1sP, whose token sum is a butterfly: against it the rerank agrees to fp32
summation order, |difference| <= 2 g(L - 1) sum_i |M_i| (g(n) = n 2^-24 / (1 - n 2^-24), M_i the per-token maxima; for unit rows
sum_i |M_i| <= 1.01 L) -- a bound from the two summation errors, not from a measurement.
"""
import os
import socket

import numpy as np
import pytest
import torch

from tests import live_truth as lt
from tests.test_gpu_parity import _oracle, _random_generic, close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DIM = 320


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16, base=None, dim=DIM):
    x = torch.randn(n, dim, generator=g)
    if base is not None:
        x = x * 0.3 + base
    return torch.nn.functional.normalize(x, dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _gathered(full, cand, id_base):
    """The full scan restricted to the listed ids: (-inf, -1) where an entry is empty or off the corpus."""
    n = full.shape[1]
    c = cand.cpu()
    d = c - id_base
    ok = (c >= 0) & (d >= 0) & (d < n)
    rows = torch.arange(c.shape[0]).unsqueeze(1).expand_as(c)
    g = full.cpu()[rows, d.clamp(0, max(n - 1, 0))]
    return torch.where(ok, g, torch.full_like(g, -float("inf"))), torch.where(ok, c, torch.full_like(c, -1))


def _check(amd, pq, corpus, cand, ref_rounding=False, full=None):
    if full is None:
        full = amd.maxsim_scores(pq, corpus, ref_rounding=ref_rounding)
    got_s, got_i = amd.retrieval.rerank_scores(pq, corpus, cand, ref_rounding=ref_rounding)
    want_s, want_i = _gathered(full, cand, corpus.id_base)
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i.numpy())
    np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
    again = amd.rerank(pq, corpus, cand, ref_rounding=ref_rounding)
    np.testing.assert_array_equal(_bits(again), _bits(got_s))      # a rerun: the same bits
    return full, got_s


# every unit count 1 .. 8 (16-token units), both sides of every boundary
QLENS = [1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 80, 81, 96, 100, 112, 113, 127, 128, 7]
DLENS = [1, 31, 32, 33, 700, 1024, 1030, 0, 64, 3, 250, 0, 96]


def _ragged_case(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(DIM, generator=g)
    qs = [_unit(g, n, dtype, base) for n in QLENS]
    qs[-1] = torch.zeros(7, DIM, dtype=dtype)                       # compaction empties it: a 0-token query
    ps = [_unit(g, n, dtype, -base if i % 3 == 1 else None) if n else torch.zeros(0, DIM, dtype=dtype) for i, n in enumerate(DLENS)]
    return qs, ps


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ref_rounding", [False, True])
def test_bit_identity_with_the_flat_scan(amd, dtype, ref_rounding):
    qs, ps = _ragged_case(dtype)
    n, n_q = len(ps), len(qs)
    for batch_size, id_base in ((3, 0), (3, 7000), (None, 123)):
        corpus = amd.pack_passages(ps, DEV, batch_size=batch_size, id_base=id_base)
        if batch_size:
            assert corpus.clamp0 is not None and int(corpus.clamp0.sum()) > 0
        else:
            assert corpus.clamp0 is None or int(corpus.clamp0.sum()) == 0
        pq = amd.pack_queries(qs, DEV, layout="flat")
        assert int(pq.tokens.shape[1]) == DIM and int(pq.lengths[-1]) == 0
        assert len(set(int(x) for x in pq.lengths)) > 2               # several lengths: the scan below is K1bPF
        g = torch.Generator().manual_seed(1)
        rows = []
        for q in range(n_q):
            ids = torch.randint(0, n, (12,), generator=g) + id_base                               # random, duplicates inside a row
            extra = torch.tensor([-1, id_base - 1, id_base + n, ids[0].item(), id_base + 6, id_base + 5, id_base + 7])
            rows.append(torch.cat([ids, extra]))
        cand = torch.stack(rows).to(DEV)
        full, got = _check(amd, pq, corpus, cand, ref_rounding)
        gs = got.cpu()
        assert torch.equal(gs[:, 0].view(torch.int32), gs[:, 15].view(torch.int32))               # the duplicate: identical bits
        assert bool(torch.isinf(gs[:, 12:15]).all() and (gs[:, 12:15] < 0).all())
        assert bool((gs[-1][gs[-1] != -float("inf")] == 0).all())                                 # the 0-token query scores 0
        shared = (torch.arange(n + 2, device=DEV) + id_base - 1).expand(n_q, n + 2)               # one list for all: a broadcast view
        assert shared.stride(0) == 0
        _check(amd, pq, corpus, shared, ref_rounding, full)
        _check(amd, pq, corpus, cand[:, 4:5].contiguous(), ref_rounding, full)                    # m = 1
        _check(amd, pq, corpus, cand[:, 3:9], ref_rounding, full)                                 # a strided view


def test_the_single_length_scan_corner_agrees_to_summation_order(amd):
    """4 queries x 32 tokens: the scan of exactly these runs K1sP (butterfly token sum); the rerank carries K1bPF's bits."""
    g = torch.Generator().manual_seed(2)
    L = 32
    qs = [_unit(g, L) for _ in range(4)]
    ps = [_unit(g, n) for n in (1, 31, 32, 33, 700, 1024, 1030, 64, 200)]
    corpus = amd.pack_passages(ps, DEV, batch_size=None, id_base=9)
    cand = (torch.arange(len(ps), device=DEV) + 9).expand(4, len(ps))
    got = amd.rerank(amd.pack_queries(qs, DEV, layout="flat"), corpus, cand).cpu()
    scan = amd.maxsim_scores(amd.pack_queries(qs, DEV, layout="flat"), corpus).cpu()
    n1 = (L - 1) * 2.0 ** -24
    bound = 2.0 * (n1 / (1.0 - n1)) * 1.01 * L
    diff = float((got.double() - scan.double()).abs().max())
    print(f"K1sP corner: max |rerank - scan| = {diff:.3e}, bound = {bound:.3e}")
    assert diff <= bound
    forced = amd.maxsim_scores(amd.pack_queries(qs + [_unit(g, 33)], DEV, layout="flat"), corpus).cpu()[:4]   # a 33-token query forces K1bPF
    np.testing.assert_array_equal(_bits(got), _bits(forced))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_scores_against_the_float64_oracle(amd, dtype):
    qs, ps = _random_generic(41, 9, 128, 60, 400, DIM, dtype)
    for bs in (128, 7):
        corpus = amd.pack_passages(ps, DEV, batch_size=bs)
        want = _oracle(qs, ps, bs)
        cand = torch.stack([torch.randperm(len(ps), generator=torch.Generator().manual_seed(q)) for q in range(len(qs))])
        got = amd.rerank(qs, corpus, cand.to(DEV)).cpu().numpy()
        assert close(got, np.take_along_axis(np.asarray(want), cand.numpy(), axis=1))


def _capture(fn):
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


def test_grouping_independence_rerun_and_captured_replays(amd):
    g = torch.Generator().manual_seed(3)
    ps = [_unit(g, int(n)) for n in torch.randint(1, 300, (80,), generator=g)]
    corpus = amd.pack_passages(ps, DEV, batch_size=None, id_base=11)
    qs = [_unit(g, int(n)) for n in torch.randint(1, 129, (24,), generator=g)]
    pq = amd.pack_queries(qs, DEV, layout="flat")
    cand = torch.randint(11, 91, (24, 30), generator=g).to(DEV)
    base = amd.rerank(pq, corpus, cand)
    np.testing.assert_array_equal(_bits(amd.rerank(pq, corpus, cand)), _bits(base))               # a rerun
    perm = torch.randperm(30, generator=g).to(DEV)                                                # the same entries, other columns
    np.testing.assert_array_equal(_bits(amd.rerank(pq, corpus, cand[:, perm].contiguous())), _bits(base[:, perm]))
    order = torch.randperm(24, generator=g).tolist()                                              # the same queries in another batch
    sub = order[:7]
    pq2 = amd.pack_queries([qs[i] for i in sub] + [_unit(g, 50)], DEV, layout="flat")
    cand2 = torch.cat([cand[sub], torch.randint(11, 91, (1, 30), generator=g).to(DEV)])
    np.testing.assert_array_equal(_bits(amd.rerank(pq2, corpus, cand2)[:7]), _bits(base[sub]))
    # replays of a captured call: the counters are zeroed by a kernel node, so every replay starts from zero
    eager, captured, graph = _capture(lambda: (amd.rerank(pq, corpus, cand),) + tuple(amd.rerank(pq, corpus, cand, 10)))
    for _ in range(3):
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            view = np.int32 if got.dtype == torch.float32 else np.int64
            np.testing.assert_array_equal(got.cpu().numpy().view(view), want.cpu().numpy().view(view))
    np.testing.assert_array_equal(_bits(eager[0]), _bits(base))


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


def test_two_stage_and_sharded_search(amd, dist):
    g = torch.Generator().manual_seed(4)
    n = 120
    pages = [_unit(g, int(k)) for k in torch.randint(60, 300, (n,), generator=g)]
    qs = [_unit(g, int(k)) for k in torch.randint(1, 129, (10,), generator=g)]
    planted = torch.randperm(n, generator=g)[:10].tolist()
    for q, c in zip(qs, planted):                                   # page `c` holds query q's tokens among its own rows
        pages[c] = torch.cat([pages[c][:40], q, pages[c][40:]])
    full = amd.pack_passages(pages, DEV, batch_size=None, id_base=50)
    pq = amd.pack_queries(qs, DEV, layout="flat")
    scan = amd.maxsim_scores(pq, full)
    exact = amd.ShardedRetriever(full).search(pq, k=10)

    # a prefilter that is the corpus itself, every document a candidate: the exact search
    for force in (False, True):
        r = amd.ShardedRetriever(full, world=1, rank=0, dist=dist, force_collective=force)
        s, i = r.search(pq, k=10, prefilter=full, n_candidates=len(full))
        np.testing.assert_array_equal(i.cpu().numpy(), exact[1].cpu().numpy())
        np.testing.assert_array_equal(_bits(s), _bits(exact[0]))
        cand = torch.randint(40, 180, (10, 30), generator=torch.Generator().manual_seed(5)).to(DEV)
        s, i = r.search(pq, k=10, candidates=cand)
        ws, wi = amd.rerank(pq, full, cand, 10)
        np.testing.assert_array_equal(i.cpu().numpy(), wi.cpu().numpy())
        np.testing.assert_array_equal(_bits(s), _bits(ws))

    # pooled pages as the first stage: what stage 1 lists comes back with the exact scores
    pooled_pages = amd.HierarchicalTokenPooler().pool_embeddings([p.to(DEV) for p in pages], pool_factor=3)
    pooled = amd.pack_passages([p.cpu().to(torch.bfloat16) for p in pooled_pages], DEV, batch_size=None, id_base=50)
    m = 15
    _, ci = amd.topk(amd.maxsim_scores(pq, pooled), m, pooled.id_base)
    ws, wi = amd.rerank(pq, full, ci, 10)
    s, i = amd.ShardedRetriever(full).search(pq, k=10, prefilter=pooled, n_candidates=m)
    np.testing.assert_array_equal(i.cpu().numpy(), wi.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(ws))
    listed = 0
    for q, c in enumerate(planted):
        if (ci[q] == c + 50).any():
            listed += 1
            assert int(i[q, 0]) == c + 50
            assert _bits(s[q, 0:1])[0] == _bits(scan[q, c:c + 1])[0]
    assert listed >= 8                                              # the planted page holds the query itself: stage 1 finds it

    # three virtual ranks on one GPU: each rank's stage 1, the merge of the lists, each rank's stage 2, the merge of those
    want = amd.ShardedRetriever(full).search(pq, k=10, prefilter=pooled, n_candidates=m)
    for world in (1, 2, 3):
        shards = []
        for rank in range(world):
            lo, hi = amd.shard_range(n, world, rank)
            shards.append((amd.pack_passages(pages[lo:hi], DEV, batch_size=None, id_base=50 + lo),
                           amd.pack_passages([p.cpu().to(torch.bfloat16) for p in pooled_pages[lo:hi]], DEV, batch_size=None,
                                             id_base=50 + lo)))
        lists = [amd.topk(amd.maxsim_scores(pq, pool), m, pool.id_base) for _, pool in shards]
        _, cand = amd.merge_gathered(torch.stack([a for a, _ in lists]), torch.stack([b for _, b in lists]), m)
        np.testing.assert_array_equal(cand.cpu().numpy(), ci.cpu().numpy())
        parts = [amd.retrieval.rerank_scores(pq, shard, cand) for shard, _ in shards]
        loc = [amd.topk(a, 10, 0, b) for a, b in parts]
        s, i = amd.merge_gathered(torch.stack([a for a, _ in loc]), torch.stack([b for _, b in loc]), 10)
        np.testing.assert_array_equal(i.cpu().numpy(), want[1].cpu().numpy())
        np.testing.assert_array_equal(_bits(s), _bits(want[0]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_live_shard_candidates_and_prefilter(amd, dtype):
    g = torch.Generator().manual_seed(6)
    live = amd.LiveCorpus(9000, 200, DEV, dtype=dtype, width=DIM, id_base=50, bounce_bytes=5 * DIM * 2)
    pages, table = [], lt.SlotTable(50)

    def add(lens):
        new = [_unit(g, n, dtype) for n in lens]
        assert live.add(new).tolist() == table.add(lens)
        pages.extend(new)

    def delete(ids):
        live.delete(ids)
        table.delete(ids)

    add([1, 40, 1, 1030, 33, 64, 90, 17, 5, 250])
    delete([51, 55, 58])
    live.compact()
    table.compact()
    add([int(x) for x in torch.randint(1, 90, (12,), generator=g)])
    delete([50, 62, 70])                                            # tombstones that no compaction has removed yet
    qs = [_unit(g, n, dtype) for n in (32, 5, 17, 128, 100, 64, 1, 49)]
    pq = amd.pack_queries(qs, DEV, layout="flat")
    surv = table.survivors()
    F = amd.pack_passages([pages[s] for s in surv], DEV, batch_size=None)
    ref = amd.ShardedRetriever(F)
    cand = torch.randint(45, 50 + len(pages) + 5, (len(qs), 14), generator=g)   # ids below, inside (live and deleted) and above
    cand[1, :] = -1
    cand[2, :3] = torch.tensor([51, 62, 50])                        # deleted pages
    cand[3, 0] = cand[3, 1] = 53                                    # a duplicate
    cand = cand.to(DEV)
    pos = {s + 50: p for p, s in enumerate(surv)}
    tcand = torch.tensor([[pos.get(int(c), -1) for c in row] for row in cand.tolist()], dtype=torch.int64, device=DEV)
    for k in (5, 14):
        got_s, got_i = live.search(pq, k, candidates=cand)
        want_s, want_i = ref.search(pq, k, candidates=tcand)
        np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
        np.testing.assert_array_equal(got_i.cpu().numpy(), lt.expected_ids(want_i.cpu().numpy(), surv, 50))
    dead = {s + 50 for s, a in enumerate(table.alive) if not a}
    assert not (set(got_i.cpu().flatten().tolist()) & dead)
    assert (got_i[1] == -1).all() and torch.isinf(got_s[1]).all()
    raw_s, raw_i = live._rerank(pq, live.view(), cand)              # stage 2 itself: a deleted id is (-inf, -1)
    assert (raw_i[2, :3] == -1).all() and bool(torch.isinf(raw_s[2, :3]).all() and (raw_s[2, :3] < 0).all())

    pool_all = amd.pack_passages([p[::3].contiguous() for p in pages], DEV, batch_size=None, id_base=50)     # over the same slots
    pool_surv = amd.pack_passages([pages[s][::3].contiguous() for s in surv], DEV, batch_size=None)
    for m in (1, 6, len(surv)):
        got_s, got_i = live.search(pq, 10, prefilter=pool_all, n_candidates=m)
        want_s, want_i = ref.search(pq, 10, prefilter=pool_surv, n_candidates=m)
        np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
        np.testing.assert_array_equal(got_i.cpu().numpy(), lt.expected_ids(want_i.cpu().numpy(), surv, 50))
    with pytest.raises(NotImplementedError):                        # the int8 first stage stays at width 128
        live.int8_index()


def test_device_offsets_that_disagree_with_the_host_copy_poison_the_call(amd):
    g = torch.Generator().manual_seed(7)
    corpus = amd.pack_passages([_unit(g, int(n)) for n in torch.randint(1, 200, (30,), generator=g)], DEV, batch_size=None)
    pq = amd.pack_queries([_unit(g, 20) for _ in range(3)], DEV, layout="flat")
    bad = amd.PackedQueries(tokens=pq.tokens, offsets=torch.tensor([0, 20, 40, 300], dtype=torch.int32, device=DEV),
                            offsets_host=pq.offsets_host)
    s = amd.rerank(bad, corpus, torch.randint(0, 30, (3, 9), generator=g).to(DEV))
    assert bool(torch.isnan(s).all())


def test_the_c_abi_directly(amd):
    """out_ids = NULL, ld_scores > m, a list row stride > m; the first workspace word reads 0 afterwards."""
    from colpali_amd import _lib

    g = torch.Generator().manual_seed(8)
    corpus = amd.pack_passages([_unit(g, int(n)) for n in torch.randint(1, 200, (40,), generator=g)], DEV, batch_size=None, id_base=5)
    pq = amd.pack_queries([_unit(g, n) for n in (3, 70, 128, 16)], DEV, layout="flat")
    big = torch.randint(0, 50, (4, 20), generator=g).to(DEV)
    m, ld = 11, 16
    L = _lib.lib()
    nbytes = L.msim_fwd_candidates_wide_workspace_bytes(4, m, len(corpus), DIM)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    out = torch.full((4, ld), 7.0, dtype=torch.float32, device=DEV)
    rc = L.msim_fwd_candidates_wide(0, _lib.ptr(pq.tokens), _lib.ptr(pq.offsets), pq.offsets_host.data_ptr(), 4, _lib.ptr(corpus.blob),
                                    _lib.ptr(corpus.offsets), None, len(corpus), DIM, _lib.ptr(big), m, 20, 5, _lib.ptr(out), ld, None, 0,
                                    _lib.ptr(ws), _lib.current_stream_handle(DEV))
    assert rc == 0, L.msim_last_error()
    torch.cuda.synchronize()
    want = amd.rerank(pq, corpus, big[:, :m].contiguous())
    np.testing.assert_array_equal(_bits(out[:, :m]), _bits(want))
    assert bool((out[:, m:] == 7.0).all())                          # nothing beyond column m is written
    assert int(ws[:4].view(torch.int32)[0]) == 0
    rc = L.msim_fwd_candidates_wide(0, _lib.ptr(pq.tokens), _lib.ptr(pq.offsets), pq.offsets_host.data_ptr(), 4, _lib.ptr(corpus.blob),
                                    _lib.ptr(corpus.offsets), None, len(corpus), 128, _lib.ptr(big), m, 20, 5, _lib.ptr(out), ld, None, 0,
                                    _lib.ptr(ws), _lib.current_stream_handle(DEV))
    assert rc == -2                                                 # the wide entry does not serve width 128


def test_error_paths(amd):
    g = torch.Generator().manual_seed(9)
    corpus = amd.pack_passages([_unit(g, 5) for _ in range(10)], DEV, batch_size=None)
    cand = torch.randint(0, 10, (2, 4), generator=g).to(DEV)
    with pytest.raises(RuntimeError):                                  # dtype mismatch
        amd.rerank([_unit(g, 8, torch.float16)] * 2, corpus, cand)
    with pytest.raises(NotImplementedError):                           # fp32
        c32 = amd.pack_passages([torch.randn(5, DIM)] * 10, DEV, batch_size=None)
        amd.rerank([torch.randn(8, DIM)] * 2, c32, cand)
    for width in (96, 64):                                             # neither 128 nor 320
        with pytest.raises(NotImplementedError):
            cw = amd.pack_passages([_unit(g, 5, dim=width)] * 10, DEV, batch_size=None)
            amd.rerank([_unit(g, 8, dim=width)] * 2, cw, cand)
    with pytest.raises(NotImplementedError):                           # width-128 queries against a width-320 corpus
        amd.rerank([_unit(g, 8, dim=128)] * 2, corpus, cand)
    with pytest.raises(NotImplementedError):                           # a query over 128 tokens
        amd.rerank([_unit(g, 129), _unit(g, 4)], corpus, cand)
    with pytest.raises(RuntimeError):                                  # a CPU corpus: the GPU-only error
        amd.rerank([_unit(g, 8)] * 2, amd.pack_passages([_unit(g, 5)] * 10, torch.device("cpu"), batch_size=None), cand.cpu())
    with pytest.raises(NotImplementedError):                           # the int8 and FDE first stages stay at width 128
        amd.Int8Index.build(corpus)
    with pytest.raises(NotImplementedError):
        amd.FdeIndex.build(corpus)
