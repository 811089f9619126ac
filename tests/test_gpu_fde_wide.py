"""Fixed dimensional encodings at width 320 on the MI355X (msim_fdew_*, colpali_amd.FdeWideIndex / fde_wide_scores,
search(prefilter=<FdeWideIndex>)).

The encoders are checked against the float64 restatement in tests/fde_wide_truth.py.  The kernel's bucket codes must equal phi
wherever no sign dot of that (row, rep) lies within 1e-4 of 0, and at most 0.5 % of the (row, rep) pairs may be excluded that way
(for unit rows and normal G the expected share is k_sim x 8e-5 <= 0.05 %).  Given the kernel's codes, every entry must lie within
    1 ulp of the dtype at the true value + (m_b + 322) * 2^-24 * sum_c A_b[c] / sqrt(d_proj),
m_b the rows of the bucket, A_b[c] the sum of |x[c]| over them for a query and their mean for a page: the fp32 accumulation bound
of ANY summation order of the bucket sum (m_b terms), the mean's division and the 320-term projection, so it does not prescribe
the kernel's order.  Unit-vector pages and queries pin every column slice exactly; reruns, chunking, batching and out= are bit
identities; the searches equal their hand compositions bit for bit.
"""
import os
import socket

import numpy as np
import pytest
import torch

from tests import fde_wide_truth as ft

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = 320
PAGE_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 1023, 1024, 2049)        # around every plausible rows-per-pass
QUERY_LENS = (1, 3, 16, 17, 32, 200, 1024)
CONFIGS = [dict(reps=20, ksim=5, dproj=16), dict(reps=2, ksim=6, dproj=64), dict(reps=32, ksim=1, dproj=8),
           dict(reps=4, ksim=3, dproj=32), dict(reps=1, ksim=6, dproj=8)]
UNIT_COLS = (0, 7, 8, 63, 64, 79, 80, 127, 128, 159, 160, 239, 240, 255, 256, 319)   # each side of every 32/64/80/128/160 split
_cfg_id = lambda c: f"R{c['reps']}k{c['ksim']}d{c['dproj']}"      # noqa: E731


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16, width=W):
    return torch.nn.functional.normalize(torch.randn(n, width, generator=g), dim=-1).to(dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.int64).numpy()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(_bits(x), _bits(y))


def _ulp(v, dtype):
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(v), 1e-300)))
    return 2.0 ** (np.maximum(e, emin) - mant)


def _accumulation_bound(X, off, kc, config, doc):
    """(m_b + 322) 2^-24 sum_c A_b[c] / sqrt(d_proj) of every (item, rep, bucket): [n_items, R, B]"""
    B = config.buckets
    mass = np.abs(X).sum(axis=1)                                    # sum_c |x[c]| of every row
    out = np.zeros((len(off) - 1, config.reps, B))
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        if a == b:
            continue
        for r in range(config.reps):
            phi = kc[a:b, r]
            m = np.bincount(phi, minlength=B).astype(np.float64)
            A = np.bincount(phi, weights=mass[a:b], minlength=B)
            if doc:
                A = A / np.maximum(m, 1)
                if config.fill_empty:                               # an empty bucket holds one row
                    for e in np.nonzero(m == 0)[0]:
                        A[e], m[e] = mass[a + ft.nearest_row(phi, e)], 1
            out[i, r] = (m + 322) * 2.0 ** -24 * A / np.sqrt(config.dproj)
    return out


def _check_encoding(got, rows, offsets, kernel_codes, config, doc):
    """codes vs phi away from the hyperplanes; entries vs the truth evaluated on the kernel's codes."""
    G, S = ft.params(config.reps, config.ksim, config.dproj, config.seed)
    off = np.asarray(offsets, dtype=np.int64)
    X = rows.float().cpu().double().numpy()[:off[-1]]
    kc = kernel_codes.cpu().numpy().astype(np.int64)[:off[-1]]
    assert kc.max(initial=0) < config.buckets, "a row's code was not written"
    clear = (np.abs(ft.dots(X, G)) > 1e-4).all(axis=2)
    print(f"\n    codes excluded near a hyperplane: {(~clear).sum()} of {clear.size} (row, rep) pairs")
    assert (~clear).mean() <= 0.005
    np.testing.assert_array_equal(kc[clear], ft.codes(X, G)[clear])
    want = ft.encode_all(X, off, G, S, doc=doc, fill_empty=config.fill_empty, phi=kc)
    got = got.float().cpu().double().numpy()
    err = np.abs(got - want)
    bound = np.repeat(_accumulation_bound(X, off, kc, config, doc), config.dproj, axis=2).reshape(want.shape)
    tol = _ulp(want, rows.dtype) + bound
    print(f"    worst error / tolerance: {(err / tol).max():.3f}")
    bad = err > tol
    assert not bad.any(), f"{bad.sum()} entries off, worst {err[bad].max()} at truth {want[bad][np.argmax(err[bad])]}"


def _pages(dtype, seed=21):
    g = torch.Generator().manual_seed(seed)
    pages = [_unit(g, n, dtype) for n in PAGE_LENS]
    pages[4][3] = 0                                                 # a zero row: bucket 0, counted
    return pages


# ------------------------------------------------------------------------------------------------ the encoders against the truth
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
@pytest.mark.parametrize("fill", [True, False], ids=["fill", "nofill"])
def test_document_encoder_against_the_truth(amd, dtype, cfg, fill):
    from colpali_amd.fde_wide import fde_wide_encode_corpus

    config = amd.FdeConfig(**cfg, seed=3, fill_empty=fill)
    corpus = amd.pack_passages(_pages(dtype), DEV, batch_size=None)
    assert corpus.width == W and corpus.offsets.cpu().tolist() == np.cumsum((0,) + PAGE_LENS).tolist()
    codes = torch.full((corpus.blob.shape[0], config.reps), 255, dtype=torch.uint8, device=DEV)
    got = fde_wide_encode_corpus(corpus, config, codes=codes)
    _check_encoding(got, corpus.blob, corpus.offsets.cpu().numpy(), codes, config, doc=True)
    assert (_bits(got[0]) == 0).all()                               # the 0-row page
    zero_row = int(np.cumsum((0,) + PAGE_LENS)[4]) + 3
    assert (codes[zero_row] == 0).all()                             # no dot of a zero row is > 0
    again = amd.FdeWideIndex.build(corpus, config, chunk_docs=3)    # chunked launches: the same bits
    np.testing.assert_array_equal(_bits(again.Fd), _bits(got))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
def test_query_encoder_against_the_truth(amd, dtype, cfg):
    config = amd.FdeConfig(**cfg, seed=5)
    g = torch.Generator().manual_seed(22)
    qs = [_unit(g, n, dtype) for n in QUERY_LENS]                   # a host list: 1024 tokens is past the flat packer's 512 at this width
    index = amd.FdeWideIndex(torch.zeros((1, config.dim), dtype=dtype, device=DEV), 0, config)
    codes = torch.full((sum(QUERY_LENS), config.reps), 255, dtype=torch.uint8, device=DEV)
    got = amd.fde_wide_encode_queries(qs, index, codes=codes)
    _check_encoding(got, torch.cat(qs), np.cumsum((0,) + QUERY_LENS), codes, config, doc=False)
    short = amd.pack_queries(qs[:5], DEV, layout="flat")            # the packed form of the short ones: the same bits
    np.testing.assert_array_equal(_bits(amd.fde_wide_encode_queries(short, index)), _bits(got[:5]))


# ------------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("fill", [True, False], ids=["fill", "nofill"])
def test_unit_vector_pages_and_queries_are_exact(amd, dtype, fill):
    """a one-row item e_c: its code is the sign pattern of G[r, :, c] and its bucket holds S[r, :, c] / 4, bit for bit (d_proj = 16:
    1 / sqrt(d_proj) is exact) -- a dropped or doubled column slice, which random data hides inside the tolerance, shows here"""
    from colpali_amd.fde_wide import fde_wide_encode_corpus

    config = amd.FdeConfig(reps=2, ksim=3, dproj=16, seed=13, fill_empty=fill)
    G, S = config.params(width=W)
    R, B = config.reps, config.buckets
    rows = torch.zeros((len(UNIT_COLS), W), dtype=dtype)
    for i, c in enumerate(UNIT_COLS):
        rows[i, c] = 1
    cols = torch.tensor(UNIT_COLS)
    want_codes = ((G[:, :, cols] > 0).long() * (1 << torch.arange(config.ksim))[None, :, None]).sum(dim=1).T      # [16, R]
    quarter = (S[:, :, cols] / 4).permute(2, 0, 1).to(dtype)                                                        # [16, R, dproj]
    assert torch.equal(quarter.float().abs(), torch.full_like(quarter.float(), 0.25))
    here = torch.zeros((len(UNIT_COLS), R, B), dtype=torch.bool)
    here.scatter_(2, want_codes[:, :, None], True)

    corpus = amd.pack_passages([r[None] for r in rows], DEV, batch_size=None)
    codes = torch.full((len(UNIT_COLS), R), 255, dtype=torch.uint8, device=DEV)
    Fd = fde_wide_encode_corpus(corpus, config, codes=codes).cpu().view(len(UNIT_COLS), R, B, config.dproj)
    np.testing.assert_array_equal(codes.cpu().long().numpy(), want_codes.numpy())
    full = quarter[:, :, None, :].expand(-1, -1, B, -1)
    want_d = full if fill else torch.where(here[..., None], full, torch.zeros_like(full))
    np.testing.assert_array_equal(_bits(Fd), _bits(want_d))

    pq = amd.pack_queries([r[None] for r in rows], DEV, layout="flat")
    index = amd.FdeWideIndex(torch.zeros((1, config.dim), dtype=dtype, device=DEV), 0, config)
    codes.fill_(255)
    Fq = amd.fde_wide_encode_queries(pq, index, codes=codes).cpu().view(len(UNIT_COLS), R, B, config.dproj)
    np.testing.assert_array_equal(codes.cpu().long().numpy(), want_codes.numpy())
    np.testing.assert_array_equal(_bits(Fq), _bits(torch.where(here[..., None], full, torch.zeros_like(full))))   # a query never fills


# ------------------------------------------------------------------------------------------------------------------ bit identities
def test_bit_identities(amd):
    from colpali_amd.fde_wide import fde_wide_encode_corpus

    config = amd.FdeConfig(reps=4, ksim=4, dproj=16, seed=2)
    g = torch.Generator().manual_seed(23)
    pages = [_unit(g, n) for n in (700, 81, 33, 0, 1024, 5, 160)]
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    a = amd.FdeWideIndex.build(corpus, config)
    np.testing.assert_array_equal(_bits(amd.FdeWideIndex.build(corpus, config).Fd), _bits(a.Fd))                  # rerun
    np.testing.assert_array_equal(_bits(amd.FdeWideIndex.build(corpus, config, chunk_docs=3).Fd), _bits(a.Fd))    # three launches
    for i in (0, 4, 6):                                                                                            # alone
        alone = amd.FdeWideIndex.build(amd.pack_passages([pages[i]], DEV, batch_size=None), config)
        np.testing.assert_array_equal(_bits(alone.Fd[0]), _bits(a.Fd[i]))
    out = torch.full((len(pages), config.dim), float("nan"), dtype=torch.bfloat16, device=DEV)
    got = fde_wide_encode_corpus(corpus, config, out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_bits(out), _bits(a.Fd))

    qs = [_unit(g, n) for n in (32, 7, 200, 81, 1)]
    pq = amd.pack_queries(qs, DEV, layout="flat")
    Fq = amd.fde_wide_encode_queries(pq, a)
    np.testing.assert_array_equal(_bits(amd.fde_wide_encode_queries(pq, a)), _bits(Fq))
    qout = torch.full((len(qs), config.dim), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert amd.fde_wide_encode_queries(pq, a, out=qout).data_ptr() == qout.data_ptr()
    np.testing.assert_array_equal(_bits(qout), _bits(Fq))
    for i in (0, 2, 4):
        np.testing.assert_array_equal(_bits(amd.fde_wide_encode_queries([qs[i]], a)[0]), _bits(Fq[i]))
    scores = amd.fde_wide_scores(pq, a)
    sout = torch.full((len(qs), len(pages)), float("nan"), dtype=torch.float32, device=DEV)
    assert amd.fde_wide_scores(pq, a, out=sout).data_ptr() == sout.data_ptr()
    np.testing.assert_array_equal(_bits(sout), _bits(scores))
    np.testing.assert_array_equal(_bits(amd.fde_wide_scores(qs[:3], a)), _bits(scores[:3]))


# ------------------------------------------------------------------------------------------------------------------ the scorer
def test_fde_wide_scores_of_encoded_queries(amd):
    g = torch.Generator().manual_seed(31)
    corpus = amd.pack_passages([_unit(g, int(n)) for n in torch.randint(0, 200, (133,), generator=g)], DEV, batch_size=None)
    index = amd.FdeWideIndex.build(corpus)
    qs = [_unit(g, 32) for _ in range(70)]
    got = amd.fde_wide_scores(qs, index)
    Fq = amd.fde_wide_encode_queries(qs, index)
    q, d = Fq.double().cpu().numpy(), index.Fd.double().cpu().numpy()
    assert got.shape == (70, 133) and got.dtype == torch.float32
    assert (np.abs(got.cpu().double().numpy() - q @ d.T) <= 1e-5 * (np.abs(q) @ np.abs(d).T) + 1e-30).all()
    np.testing.assert_array_equal(_bits(got[:3]), _bits(amd.fde_wide_scores(qs[:3], index)))


# ------------------------------------------------------------------------------------------------------------------ the searches
K, ID_BASE = 10, 50


@pytest.fixture(scope="module")
def case(amd):
    g = torch.Generator().manual_seed(8)
    pages = [_unit(g, int(n)) for n in torch.randint(20, 120, (300,), generator=g)]
    full = amd.pack_passages(pages, DEV, batch_size=None, id_base=ID_BASE)
    index = amd.FdeWideIndex.build(full, amd.FdeConfig(reps=8, ksim=4, dproj=16, seed=1))
    pq = amd.pack_queries([_unit(g, int(n)) for n in torch.randint(1, 64, (12,), generator=g)], DEV, layout="flat")
    return pages, full, index, pq


def test_two_stage_search_is_exact_rerank_of_the_fde_top_m(amd, case):
    _, full, index, pq = case
    r = amd.ShardedRetriever(full)
    for m in (1, 25, 100):
        _, ci = amd.topk(amd.fde_wide_scores(pq, index), m, index.id_base)
        _same(r.search(pq, k=K, prefilter=index, n_candidates=m), amd.rerank(pq, full, ci, K))
    exact = r.search(pq, k=K)
    for m in (300, 500):                                            # every page a candidate: the exact search, bit for bit
        _same(r.search(pq, k=K, prefilter=index, n_candidates=m), exact)


def test_three_stage_search_is_its_hand_composition(amd, case):
    _, full, index, pq = case
    f4 = amd.Fp4WideIndex.build(full)
    r = amd.ShardedRetriever(full)
    for m1, m2 in ((100, 20), (40, 40), (300, 7)):
        _, c1 = amd.topk(amd.fde_wide_scores(pq, index), m1, index.id_base)
        fs, fi = amd.fp4_wide_rerank_scores(pq, f4, c1)
        s2, c2 = amd.topk(fs, m2, 0, fi)
        c2 = torch.where(s2 == float("-inf"), torch.full_like(c2, -1), c2)
        _same(r.search(pq, k=K, prefilter=index, n_candidates=m1, refine=f4, n_refine=m2), amd.rerank(pq, full, c2, K))


def test_two_stage_search_with_a_filter_and_with_groups(amd, case):
    _, full, index, pq = case
    n, n_q, m = len(full), len(pq), 30
    g = torch.Generator().manual_seed(71)
    allowed = (torch.rand(n, generator=g) < 0.5).to(DEV)
    labels = torch.randint(0, 40, (n,), generator=g)
    r = amd.ShardedRetriever(full)
    coarse = amd.fde_wide_scores(pq, index)
    # filter=: the list is the stage-1 top m of the allowed pages; the exact rerank orders it
    ms, mi = amd.topk(torch.where(allowed[None, :], coarse, torch.full_like(coarse, float("-inf"))), m, ID_BASE)
    mi = torch.where(ms == float("-inf"), torch.full_like(mi, -1), mi)
    ws, wi = amd.rerank(pq, full, mi, K)
    wi = torch.where(ws == float("-inf"), torch.full_like(wi, -1), wi)
    got = r.search(pq, k=K, prefilter=index, n_candidates=m, filter=amd.PageFilter.from_mask(allowed, ID_BASE))
    _same(got, (ws, wi))
    assert bool(allowed[(got[1][got[1] >= 0] - ID_BASE)].all())
    # group_by=: the list stays PAGES; every document is scored by its best exact page among them
    _, ri = amd.topk(coarse, m, ID_BASE)
    es, ei = amd.rerank(pq, full, ri).cpu().numpy(), ri.cpu().numpy()
    lab = labels.numpy()
    want_s = np.full((n_q, K), -np.inf, dtype=np.float32)
    want_g, want_p = np.full((n_q, K), -1, dtype=np.int64), np.full((n_q, K), -1, dtype=np.int64)
    for row in range(n_q):
        best = {}
        for s, p in zip(es[row], ei[row]):
            d = int(lab[p - ID_BASE])
            if d not in best or (s, -p) > (best[d][0], -best[d][1]):
                best[d] = (s, p)
        for col, (d, (s, p)) in enumerate(sorted(best.items(), key=lambda kv: (-kv[1][0], kv[0]))[:K]):
            want_s[row, col], want_g[row, col], want_p[row, col] = s, d, p
    gs, gg, gp = r.search(pq, k=K, prefilter=index, n_candidates=m, group_by=amd.PageGroups.from_labels(labels.to(DEV), ID_BASE))
    np.testing.assert_array_equal(_bits(gs), want_s.view(np.int32))
    np.testing.assert_array_equal(gg.cpu().numpy(), want_g)
    np.testing.assert_array_equal(gp.cpu().numpy(), want_p)


def test_captured_two_stage_search_replays_the_eager_bits(amd, case):
    _, full, index, pq = case
    r = amd.ShardedRetriever(full)
    fn = lambda: r.search(pq, k=K, prefilter=index, n_candidates=30)   # noqa: E731
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
        _same(captured, eager)


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


def test_one_rank_rccl_group_and_virtual_shards(amd, case, dist):
    pages, full, index, pq = case
    config = index.config
    want = amd.ShardedRetriever(full).search(pq, k=K, prefilter=index, n_candidates=40)
    _same(amd.ShardedRetriever(full, world=1, rank=0, dist=dist, force_collective=True).search(pq, k=K, prefilter=index,
                                                                                                 n_candidates=40), want)
    world = 3
    shards = []
    for rank in range(world):
        lo, hi = amd.shard_range(len(pages), world, rank)
        shard = amd.pack_passages(pages[lo:hi], DEV, batch_size=None, id_base=ID_BASE + lo)
        shards.append((shard, amd.FdeWideIndex.build(shard, config)))
    # three virtual ranks on one GPU: each rank's stage 1, the merge of their lists, each rank's stage 2, the merge of those
    lists = [amd.topk(amd.fde_wide_scores(pq, idx), 40, idx.id_base) for _, idx in shards]
    _, cand = amd.merge_gathered(torch.stack([s for s, _ in lists]), torch.stack([i for _, i in lists]), 40)
    np.testing.assert_array_equal(cand.cpu().numpy(), amd.topk(amd.fde_wide_scores(pq, index), 40, ID_BASE)[1].cpu().numpy())
    parts = [amd.retrieval.rerank_scores(pq, shard, cand) for shard, _ in shards]
    loc = [amd.topk(s, K, 0, i) for s, i in parts]
    _same(amd.merge_gathered(torch.stack([a for a, _ in loc]), torch.stack([b for _, b in loc]), K), want)


# ------------------------------------------------------------------------------------------------------------------ persistence
def test_persistence_on_the_device(amd, case, tmp_path):
    pages, full, index, _ = case
    path = str(tmp_path / "w.msim")
    index.save(path, chunk_bytes=1 << 20)
    for got in (amd.load(path, DEV), amd.FdeWideIndex.load(path, DEV)):
        assert type(got) is amd.FdeWideIndex and got.id_base == ID_BASE and got.config == index.config and got.device == DEV
        _same((got.Fd, got.params[0], got.params[1]), (index.Fd, index.params[0], index.params[1]))
    lo, hi = 17, 95
    part = amd.load(path, DEV, pages=(lo, hi))
    built = amd.FdeWideIndex.build(amd.pack_passages(pages[lo:hi], DEV, batch_size=None, id_base=ID_BASE + lo), index.config)
    assert part.id_base == built.id_base == ID_BASE + lo and len(part) == hi - lo
    _same((part.Fd, part.params[0], part.params[1]), (built.Fd, built.params[0], built.params[1]))


# ------------------------------------------------------------------------------------------------------------------ past 2^32 bytes
def test_pages_past_four_gib_of_rows(amd):
    """a row starts at row x 640 bytes, which passes 2^32 at row 6 710 887: pages that straddle it, behind a zero blob, must carry
    the bits of the same pages packed alone"""
    from colpali_amd.fde_wide import fde_wide_encode_corpus

    config = amd.FdeConfig(reps=2, ksim=3, dproj=16, seed=3)                   # F = 256
    g = torch.Generator().manual_seed(41)
    lens = (5, 80, 81, 0, 17)
    pages = [_unit(g, n) for n in lens]
    zeros = 6_710_887 - 40                                                      # the second page straddles the boundary
    total = zeros + sum(lens)
    blob = torch.zeros((total, W), dtype=torch.bfloat16, device=DEV)
    assert blob.numel() * 2 > 2**32 and zeros * 640 < 2**32 < (zeros + 5 + 80) * 640
    blob[zeros:] = torch.cat(pages).to(DEV)
    off = torch.tensor(np.cumsum((0, zeros) + lens), dtype=torch.int32, device=DEV)
    corpus = amd.PackedCorpus(blob, off, None, torch.tensor((zeros,) + lens, dtype=torch.int64))
    got = fde_wide_encode_corpus(corpus, config, lo=1)                          # the zero page itself is not encoded
    alone = amd.FdeWideIndex.build(amd.pack_passages(pages, DEV, batch_size=None), config)
    assert got.shape == (len(lens), 256) and bool(got.float().abs().sum() > 0)
    np.testing.assert_array_equal(_bits(got), _bits(alone.Fd))
    del blob, corpus
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_error_paths(amd, case):
    _, full, index, pq = case
    g = torch.Generator().manual_seed(17)
    f32 = amd.pack_passages([torch.randn(5, W, generator=g)], DEV, batch_size=None)
    with pytest.raises(NotImplementedError):
        amd.FdeWideIndex.build(f32)
    narrow = amd.pack_passages([_unit(g, 5, width=128) for _ in range(3)], DEV, batch_size=None)
    with pytest.raises(NotImplementedError):
        amd.FdeWideIndex.build(narrow)
    with pytest.raises(NotImplementedError):                                   # the 128-wide class stays where it was
        amd.FdeIndex.build(full)
    with pytest.raises(RuntimeError, match="one dtype"):
        amd.fde_wide_scores([_unit(g, 4, torch.float16)], index)
    with pytest.raises(NotImplementedError):
        amd.fde_wide_scores([_unit(g, 4, width=128)], index)
    with pytest.raises(ValueError):
        amd.FdeWideIndex.build(full, chunk_docs=0)
    # the index of the other width than the shard's
    r = amd.ShardedRetriever(full)
    cfg = index.config
    with pytest.raises(ValueError, match="320 wide"):
        r.search(pq, k=K, prefilter=amd.FdeIndex(torch.zeros((len(full), cfg.dim), dtype=torch.bfloat16, device=DEV), ID_BASE, cfg),
                 n_candidates=10)
    nq = amd.pack_queries([_unit(g, 4, width=128)], DEV, layout="flat")
    with pytest.raises(ValueError, match="128 wide"):
        amd.ShardedRetriever(narrow).search(nq, k=2, prefilter=amd.FdeWideIndex(index.Fd[:3].contiguous(), 0, cfg), n_candidates=2)
    with pytest.raises(ValueError, match="same documents"):
        r.search(pq, k=K, prefilter=amd.FdeWideIndex(index.Fd[:-1].contiguous(), ID_BASE, cfg), n_candidates=10)
