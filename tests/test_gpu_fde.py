"""Fixed dimensional encodings on the MI355X (msim_fde_*, colpali_amd.FdeIndex / fde_scores, search(prefilter=<FdeIndex>)).

The encoders are checked against the float64 restatement in tests/fde_truth.py: the kernel's bucket codes must equal phi wherever no
sign dot is within 1e-4 of 0, and given the kernel's codes every entry must be within 1 ulp of the dtype (at the true value) + 1e-6.
The scorer is checked against float64 products of its own inputs, for bit independence of the batch, and for bit-identical reruns.
"""
import os
import socket

import numpy as np
import pytest
import torch

from tests import fde_truth as ft

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LENS = (1, 15, 16, 17, 1023, 1024, 2048, 0)


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.int64).numpy()


def _ulp(v, dtype):
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(v), 1e-300)))
    return 2.0 ** (np.maximum(e, emin) - mant)


def _check_encoding(got, rows, offsets, kernel_codes, config, doc):
    """codes vs phi away from the hyperplanes; entries vs the truth evaluated on the kernel's codes."""
    G, S = ft.params(config.reps, config.ksim, config.dproj, config.seed)
    X = rows.float().cpu().double().numpy()
    kc = kernel_codes.cpu().numpy().astype(np.int64)
    d = ft.dots(X, G)
    clear = (np.abs(d) > 1e-4).all(axis=2)
    np.testing.assert_array_equal(kc[clear], ft.codes(X, G)[clear])
    want = ft.encode_all(X, offsets, G, S, doc=doc, fill_empty=config.fill_empty, phi=kc)
    got = got.float().cpu().double().numpy()
    err = np.abs(got - want)
    tol = _ulp(want, rows.dtype) + 1e-6
    bad = err > tol
    assert not bad.any(), f"{bad.sum()} entries off, worst {err[bad].max()} at truth {want[bad][np.argmax(err[bad])]}"


CONFIGS = [dict(reps=20, ksim=5, dproj=16), dict(reps=2, ksim=6, dproj=64), dict(reps=32, ksim=1, dproj=8),
           dict(reps=4, ksim=3, dproj=32), dict(reps=1, ksim=6, dproj=8)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"R{c['reps']}k{c['ksim']}d{c['dproj']}")
@pytest.mark.parametrize("fill", [True, False])
def test_document_encoder_against_the_truth(amd, dtype, cfg, fill):
    from colpali_amd.fde import encode_corpus

    config = amd.FdeConfig(**cfg, seed=3, fill_empty=fill)
    g = torch.Generator().manual_seed(21)
    pages = [_unit(g, n, dtype) for n in LENS]
    pages[1][3] = 0                                                 # a zero row: bucket 0, counted
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    rows = corpus.blob
    codes = torch.full((rows.shape[0], config.reps), 255, dtype=torch.uint8, device=DEV)
    got = encode_corpus(corpus, config, codes=codes)
    _check_encoding(got, rows, corpus.offsets.cpu().numpy(), codes, config, doc=True)
    assert (got[-1].float() == 0).all()                             # the 0-row page
    again = amd.FdeIndex.build(corpus, config, chunk_docs=3)        # chunked launches: the same bits
    np.testing.assert_array_equal(_bits(again.Fd), _bits(got))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", CONFIGS[:3], ids=lambda c: f"R{c['reps']}k{c['ksim']}d{c['dproj']}")
def test_query_encoder_against_the_truth(amd, dtype, cfg):
    config = amd.FdeConfig(**cfg, seed=5)
    g = torch.Generator().manual_seed(22)
    qs = [_unit(g, n, dtype) for n in (1, 15, 16, 17, 32, 200, 1024, 3)]
    pq = amd.pack_queries(qs, DEV, layout="flat")
    index = amd.FdeIndex(torch.zeros((1, config.dim), dtype=dtype, device=DEV), 0, config)
    codes = torch.full((pq.tokens.shape[0], config.reps), 255, dtype=torch.uint8, device=DEV)
    got = amd.encode_queries(pq, index, codes=codes)
    _check_encoding(got, pq.tokens, pq.offsets_host.numpy(), codes, config, doc=False)


def test_encoders_are_deterministic(amd):
    config = amd.FdeConfig()
    g = torch.Generator().manual_seed(23)
    corpus = amd.pack_passages([_unit(g, n) for n in (700, 1024, 33, 2048)], DEV, batch_size=None)
    a = amd.FdeIndex.build(corpus, config).Fd
    b = amd.FdeIndex.build(corpus, config).Fd
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _scores_check(amd, Fq, Fd):
    got = amd.fde.scores_from_encodings(Fq, Fd)
    q, d = Fq.double().cpu().numpy(), Fd.double().cpu().numpy()
    want = q @ d.T
    mag = np.abs(q) @ np.abs(d).T
    assert (np.abs(got.cpu().double().numpy() - want) <= 1e-5 * mag + 1e-30).all()
    return got


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n_q,F", [(1, 256), (4, 10240), (5, 256), (1000, 256), (1000, 10240), (1, 65536), (5, 65536)])
def test_scorer_against_float64(amd, dtype, n_q, F):
    g = torch.Generator().manual_seed(n_q + F)
    n_d = 1037
    Fq = (torch.randn(n_q, F, generator=g) * 0.05).to(dtype).to(DEV)
    Fd = (torch.randn(n_d, F, generator=g) * 0.05).to(dtype).to(DEV)
    got = _scores_check(amd, Fq, Fd)
    np.testing.assert_array_equal(_bits(amd.fde.scores_from_encodings(Fq, Fd)), _bits(got))       # rerun
    for lo, hi in ((0, 1), (n_q - 1, n_q), (max(0, n_q - 5), n_q)):                             # alone or in a small batch
        np.testing.assert_array_equal(_bits(amd.fde.scores_from_encodings(Fq[lo:hi], Fd)), _bits(got[lo:hi]))


def test_fde_scores_of_encoded_queries(amd):
    g = torch.Generator().manual_seed(31)
    corpus = amd.pack_passages([_unit(g, int(n)) for n in torch.randint(0, 300, (133,), generator=g)], DEV, batch_size=None)
    index = amd.FdeIndex.build(corpus)
    qs = [_unit(g, 32) for _ in range(70)]
    got = amd.fde_scores(qs, index)
    Fq = amd.encode_queries(qs, index)
    _scores_check(amd, Fq, index.Fd)
    np.testing.assert_array_equal(_bits(got[:3]), _bits(amd.fde_scores(qs[:3], index)))


def _two_stage_case(amd, seed=8, id_base=50):
    g = torch.Generator().manual_seed(seed)
    pages = [_unit(g, int(n)) for n in torch.randint(100, 400, (300,), generator=g)]
    full = amd.pack_passages(pages, DEV, batch_size=None, id_base=id_base)
    index = amd.FdeIndex.build(full)
    pq = amd.pack_queries([_unit(g, int(n)) for n in torch.randint(1, 64, (12,), generator=g)], DEV, layout="flat")
    return pages, full, index, pq


def test_two_stage_search_is_exact_rerank_of_the_fde_top_m(amd):
    _, full, index, pq = _two_stage_case(amd)
    r = amd.ShardedRetriever(full)
    for m in (1, 25, 100):
        _, ci = amd.topk(amd.fde_scores(pq, index), m, index.id_base)
        ws, wi = amd.rerank(pq, full, ci, 10)
        s, i = r.search(pq, k=10, prefilter=index, n_candidates=m)
        np.testing.assert_array_equal(i.cpu().numpy(), wi.cpu().numpy())
        np.testing.assert_array_equal(_bits(s), _bits(ws))
    es, ei = r.search(pq, k=10)
    for m in (300, 500):                                            # every page a candidate: the exact search, bit for bit
        s, i = r.search(pq, k=10, prefilter=index, n_candidates=m)
        np.testing.assert_array_equal(i.cpu().numpy(), ei.cpu().numpy())
        np.testing.assert_array_equal(_bits(s), _bits(es))


def test_captured_two_stage_fde_search_replays_the_eager_bits(amd):
    _, full, index, pq = _two_stage_case(amd, 12)
    r = amd.ShardedRetriever(full)
    fn = lambda: r.search(pq, k=10, prefilter=index, n_candidates=30)   # noqa: E731
    eager = [t.clone() for t in fn()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fn()
    for _ in range(2):
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            np.testing.assert_array_equal(_bits(got), _bits(want))


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


def test_one_rank_rccl_group_and_virtual_shards(amd, dist):
    pages, full, index, pq = _two_stage_case(amd, 14, id_base=0)
    want = amd.ShardedRetriever(full).search(pq, k=10, prefilter=index, n_candidates=40)
    s, i = amd.ShardedRetriever(full, world=1, rank=0, dist=dist, force_collective=True).search(pq, k=10, prefilter=index,
                                                                                                  n_candidates=40)
    np.testing.assert_array_equal(i.cpu().numpy(), want[1].cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(want[0]))

    world = 3
    shards = []
    for rank in range(world):
        lo, hi = amd.shard_range(len(pages), world, rank)
        shard = amd.pack_passages(pages[lo:hi], DEV, batch_size=None, id_base=lo)
        shards.append((shard, amd.FdeIndex.build(shard)))
    # three virtual ranks on one GPU: each rank's stage 1, the merge of their lists, each rank's stage 2, the merge of those
    coarse = [amd.fde_scores(pq, idx) for _, idx in shards]
    lists = []
    for rank in range(world):
        lists.append(amd.topk(coarse[rank], 40, shards[rank][1].id_base))
    all_s = torch.stack([s for s, _ in lists])
    all_i = torch.stack([i for _, i in lists])
    _, cand = amd.merge_gathered(all_s, all_i, 40)
    np.testing.assert_array_equal(cand.cpu().numpy(), amd.topk(amd.fde_scores(pq, index), 40)[1].cpu().numpy())
    parts = [amd.retrieval.rerank_scores(pq, shard, cand) for shard, _ in shards]
    loc = [amd.topk(s, 10, 0, i) for s, i in parts]
    s, i = amd.merge_gathered(torch.stack([a for a, _ in loc]), torch.stack([b for _, b in loc]), 10)
    np.testing.assert_array_equal(i.cpu().numpy(), want[1].cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(want[0]))


def test_error_paths(amd):
    _, full, index, pq = _two_stage_case(amd, 16)
    r = amd.ShardedRetriever(full)
    other = amd.FdeIndex(index.Fd[:-1].contiguous(), index.id_base, index.config)
    with pytest.raises(ValueError, match="same documents"):
        r.search(pq, k=10, prefilter=other, n_candidates=10)
    moved = amd.FdeIndex(index.Fd, index.id_base + 1, index.config)
    with pytest.raises(ValueError, match="same documents"):
        r.search(pq, k=10, prefilter=moved, n_candidates=10)
    with pytest.raises(ValueError, match="n_candidates"):
        r.search(pq, k=10, prefilter=index)
    g = torch.Generator().manual_seed(17)
    f32 = amd.pack_passages([torch.randn(5, 128, generator=g)], DEV, batch_size=None)
    with pytest.raises(NotImplementedError):
        amd.FdeIndex.build(f32)
    wide = amd.pack_passages([_unit(g, 5)[:, :64].contiguous()], DEV, batch_size=None)
    with pytest.raises(NotImplementedError):
        amd.FdeIndex.build(wide)
    with pytest.raises(RuntimeError, match="one dtype"):
        amd.fde_scores([_unit(g, 4, torch.float16)], index)
    with pytest.raises(NotImplementedError):
        amd.fde.scores_from_encodings(index.Fd.float(), index.Fd.float())
