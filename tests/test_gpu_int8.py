"""The int8 token-level index on the MI355X (msim_i8_*, colpali_amd.Int8Index / int8_scores, search(prefilter=<Int8Index>)).

Codes, scales and scores are checked bit for bit against the numpy restatement in tests/int8_truth.py; the maxima are exact
integers and the score's fp32 order is documented, so nothing here has a tolerance.
"""
import numpy as np
import pytest
import torch

from tests import int8_truth as it

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LENS = (0, 1, 15, 16, 17, 1023, 1024, 2048)


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _pages(g, dtype, lens=LENS):
    pages = [_unit(g, n, dtype) * (0.5 + i) for i, n in enumerate(lens)]
    pages.append(torch.zeros(5, 128, dtype=dtype))                 # all-zero page
    spike = torch.zeros(9, 128)
    spike[4, 77] = -3.0                                              # the max sits in one element
    spike[1, :5] = torch.tensor([0.75, -1.5, 0.006, 2.25, 1.0])
    pages.append(spike.to(dtype))
    return pages


def _corpus(amd, pages, clamp=None):
    c = amd.pack_passages(pages, DEV, batch_size=None)
    if clamp is not None:
        c.clamp0 = torch.tensor(clamp, dtype=torch.uint8, device=DEV)
    return c


def _truth_scores(q_blocks, corpus):
    rows = corpus.blob.float().cpu().numpy()
    off = corpus.offsets.cpu().numpy()
    d8, sd = it.quantize_pages(rows, off)
    qr = np.concatenate([q.float().numpy().reshape(-1, 128) for q in q_blocks]) if q_blocks else np.zeros((0, 128), np.float32)
    q8, sq = it.quantize_tokens(qr)
    q_off = np.cumsum([0] + [len(q) for q in q_blocks])
    c0 = None if corpus.clamp0 is None else corpus.clamp0.cpu().numpy()
    return it.scores(q8, sq, q_off, d8, sd, off, c0)


def _packed(amd, q_blocks):
    return amd.pack_queries(list(q_blocks), DEV, layout="flat", compact=False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_page_codes_and_scales_are_exact(amd, dtype):
    g = torch.Generator().manual_seed(1)
    corpus = _corpus(amd, _pages(g, dtype))
    idx = amd.Int8Index.build(corpus, chunk_docs=3)
    torch.cuda.synchronize()
    d8, sd = it.quantize_pages(corpus.blob.float().cpu().numpy(), corpus.offsets.cpu().numpy())
    np.testing.assert_array_equal(idx.codes.cpu().numpy(), d8)
    np.testing.assert_array_equal(_bits(idx.scales), sd.view(np.int32))
    assert len(idx) == len(corpus) and idx.device == DEV and idx.nbytes >= idx.codes.numel()
    assert torch.equal(idx.offsets, corpus.offsets) and idx.offsets.data_ptr() != corpus.offsets.data_ptr()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_query_codes_and_scales_are_exact(amd, dtype):
    g = torch.Generator().manual_seed(2)
    qs = [_unit(g, n, dtype) * 3 for n in (3, 0, 16, 33)]
    qs[0][1, :4] = torch.tensor([1.0, 0.5, -0.25, 0.0]).to(dtype)
    qs[0][1, 4:] = 0
    q = _packed(amd, qs)
    codes, scales = amd.quantize_queries(q)
    torch.cuda.synchronize()
    q8, sq = it.quantize_tokens(q.tokens.float().cpu().numpy())
    np.testing.assert_array_equal(codes.cpu().numpy(), q8)
    np.testing.assert_array_equal(_bits(scales), sq.view(np.int32))


@pytest.mark.parametrize("n_q", [1, 3, 4, 7, 64, 65, 257])
def test_scores_are_bit_equal_to_the_truth(amd, n_q):
    g = torch.Generator().manual_seed(10 + n_q)
    pages = _pages(g, torch.bfloat16, (0, 1, 15, 16, 17, 1023, 1024, 0, 2048, 40))
    clamp = [i % 3 == 0 for i in range(len(pages))]
    corpus = _corpus(amd, pages, clamp)
    special = [1, 16, 17, 32, 33, 64]
    lens = [special[i] if i < len(special) else int(torch.randint(1, 65, (1,), generator=g)) for i in range(n_q)]
    qs = [_unit(g, n) for n in lens]
    idx = amd.Int8Index.build(corpus)
    got = amd.int8_scores(_packed(amd, qs), idx)
    want = _truth_scores(qs, corpus)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))
    assert np.isneginf(got.cpu().numpy()[:, [0, 7]]).all()


def _ragged_corpus(amd, n_pages, seed):
    """Short ragged pages (0 .. 40 rows, many of 0-3 rows so that one 16-row chunk closes several pages), all-zero pages and
    zero rows mixed in, clamp0 on about a fifth: built straight as a PackedCorpus."""
    rng = np.random.default_rng(seed)
    choices = np.array([0, 0, 1, 2, 3, 5, 7, 15, 16, 17, 31, 33, 40])
    lens = rng.choice(choices, n_pages)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.standard_normal((int(off[-1]), 128)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows *= rng.uniform(0.25, 4.0, (rows.shape[0], 1)).astype(np.float32)
    rows[rng.random(rows.shape[0]) < 0.05] = 0                       # zero rows
    for c in np.nonzero(rng.random(n_pages) < 0.03)[0]:               # all-zero pages
        rows[off[c]:off[c + 1]] = 0
    blob = torch.from_numpy(rows).to(torch.bfloat16)
    clamp0 = (rng.random(n_pages) < 0.2).astype(np.uint8)
    corpus = amd.PackedCorpus(blob=blob.to(DEV), offsets=torch.from_numpy(off.astype(np.int32)).to(DEV),
                              clamp0=torch.from_numpy(clamp0).to(DEV), lengths=torch.from_numpy(lens.astype(np.int64)))
    return corpus, blob.float().numpy(), off, clamp0


def _pages_per_wave(n_q_groups, n_d):
    """The launch plan of msim_i8_scores: pages per wave range."""
    want = torch.cuda.get_device_properties(DEV).multi_processor_count * 32
    cap = 63 if n_q_groups == 1 else 16
    return max(1, min(cap, -(-n_q_groups * n_d // want)))


def _groups(lens):
    tiles = max(1, -(-max(lens) // 16))
    return len(lens) if tiles > 8 else -(-len(lens) // (8 // tiles))


@pytest.fixture(scope="module")
def ragged(amd):
    corpus, rows, off, clamp0 = _ragged_corpus(amd, 60000, 21)
    idx = amd.Int8Index.build(corpus)
    d8, sd = it.quantize_pages(rows, off)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx.codes.cpu().numpy(), d8)
    np.testing.assert_array_equal(_bits(idx.scales), sd.view(np.int32))
    return corpus, idx, d8, sd, off, clamp0


@pytest.mark.parametrize("lens", [[9], [1, 17, 32, 5], [32] * 7, [300], [300, 150], [16, 33, 64, 2]],
                         ids=["gw1-one", "gw1-four", "gw2-seven", "passes3", "passes-gw2", "gw2-wide"])
def test_multi_page_ranges_are_bit_equal_to_the_truth(amd, ragged, lens):
    """Every wave scores a range of many short pages as one row stream: page boundaries inside chunks, several pages (and empty
    ones) closed in one chunk, prefetch across pages, and the carried sum of long queries."""
    corpus, idx, d8, sd, off, clamp0 = ragged
    assert _pages_per_wave(_groups(lens), len(idx)) >= 8
    g = torch.Generator().manual_seed(sum(lens))
    qs = [_unit(g, n) * 2 for n in lens]
    q = _packed(amd, qs)
    got = amd.int8_scores(q, idx)
    q8, sq = it.quantize_tokens(q.tokens.float().cpu().numpy())
    want = it.scores_fast(q8, sq, q.offsets_host.numpy(), d8, sd, off, clamp0)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))


def test_multi_page_ranges_many_queries(amd):
    """257 queries (four waves of a workgroup share each 16-page range) over 20 000 short ragged pages."""
    corpus, rows, off, clamp0 = _ragged_corpus(amd, 20000, 22)
    idx = amd.Int8Index.build(corpus)
    g = torch.Generator().manual_seed(23)
    lens = torch.randint(1, 33, (257,), generator=g).tolist()
    assert _pages_per_wave(_groups(lens), len(idx)) == 16
    q = _packed(amd, [_unit(g, n) for n in lens])
    got = amd.int8_scores(q, idx)
    d8, sd = it.quantize_pages(rows, off)
    q8, sq = it.quantize_tokens(q.tokens.float().cpu().numpy())
    want = it.scores_fast(q8, sq, q.offsets_host.numpy(), d8, sd, off, clamp0)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))


def test_zero_token_query_scores_zero(amd):
    g = torch.Generator().manual_seed(3)
    corpus = _corpus(amd, [_unit(g, 5), _unit(g, 0), _unit(g, 20)])
    qs = [_unit(g, 4), torch.zeros(0, 128, dtype=torch.bfloat16), _unit(g, 2)]
    got = amd.int8_scores(_packed(amd, qs), amd.Int8Index.build(corpus)).cpu().numpy()
    assert (got[1, [0, 2]] == 0).all() and np.isneginf(got[:, 1]).all()
    np.testing.assert_array_equal(got.view(np.int32), _truth_scores(qs, corpus).view(np.int32))


def test_asymmetric_integer_operands(amd):
    """Integer-structured rows whose codes are their values: a transposed or permuted lane map gives other maxima."""
    g = torch.Generator().manual_seed(4)
    rows = (torch.arange(128)[None, :] * 7 + torch.arange(40)[:, None] * 13) % 255 - 127
    rows[0, 0] = 127                                                # page max 127: the codes are the values
    page = rows.float().to(torch.bfloat16)
    qrows = ((torch.arange(128)[None, :] * 3 + torch.arange(20)[:, None] * 29) % 255 - 127).float()
    qrows[:, 5] = 127                                               # each token's max 127
    extreme = torch.full((16, 128), 127.0)
    extreme[8:] = -127.0                                            # constant +-a rows: I = +-127^2 * 128, the int32 extreme
    corpus = _corpus(amd, [page, extreme.to(torch.bfloat16), page[:17]])
    qs = [qrows.to(torch.bfloat16), extreme[:3].to(torch.bfloat16), extreme[8:12].to(torch.bfloat16)]
    idx = amd.Int8Index.build(corpus)
    M = it.maxima(*it.quantize_tokens(qrows.numpy())[:1], idx.codes.cpu().numpy(), corpus.offsets.cpu().numpy())
    assert len(np.unique(M[:, 0])) > 10                              # the maxima distinguish lane maps
    got = amd.int8_scores(_packed(amd, qs), idx)
    np.testing.assert_array_equal(_bits(got), _truth_scores(qs, corpus).view(np.int32))
    assert got[1, 1].item() == 3 * 127 * 127 * 128          # sq = sd = 1: three tokens at the int32 extreme


def test_batch_independence_both_tilings(amd):
    g = torch.Generator().manual_seed(5)
    corpus = _corpus(amd, [_unit(g, n) for n in (300, 17, 0, 64, 1024, 5)])
    idx = amd.Int8Index.build(corpus)
    lens = torch.randint(1, 40, (1000,), generator=g).tolist()
    qs = [_unit(g, n) for n in lens]
    full = amd.int8_scores(_packed(amd, qs), idx)
    for i in (0, 1, 513, 999):
        alone = amd.int8_scores(_packed(amd, [qs[i]]), idx)
        np.testing.assert_array_equal(_bits(alone[0]), _bits(full[i]))
    few = amd.int8_scores(_packed(amd, qs[:3]), idx)
    np.testing.assert_array_equal(_bits(few), _bits(full[:3]))
    long_q = [_unit(g, 300), qs[7]]                                 # a query above one wave's tiles: several passes
    got = amd.int8_scores(_packed(amd, long_q), idx)
    np.testing.assert_array_equal(_bits(got[1]), _bits(full[7]))
    np.testing.assert_array_equal(_bits(got), _truth_scores(long_q, corpus).view(np.int32))


def test_reruns_and_graph_replays_are_bit_identical(amd):
    g = torch.Generator().manual_seed(6)
    corpus = _corpus(amd, [_unit(g, n) for n in (100, 3, 256, 0, 31)])
    idx = amd.Int8Index.build(corpus)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    first = amd.int8_scores(q, idx).clone()
    again = amd.int8_scores(q, idx)
    np.testing.assert_array_equal(_bits(first), _bits(again))
    out = torch.empty_like(first)
    amd.int8_scores(q, idx, out=out)                                 # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.int8_scores(q, idx, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(first))


def _docs(g, n, lo=1, hi=200):
    return [_unit(g, int(k)) for k in torch.randint(lo, hi, (n,), generator=g)]


def test_two_stage_search_with_the_int8_prefilter(amd):
    g = torch.Generator().manual_seed(7)
    docs = _docs(g, 60)
    docs[9] = docs[3].clone()                                        # exact ties
    corpus = amd.pack_passages(docs, DEV, batch_size=None)
    idx = amd.Int8Index.build(corpus)
    q = _packed(amd, [_unit(g, n) for n in (32, 7, 20)])
    k, m = 5, 12
    r = amd.ShardedRetriever(corpus)
    s, i = r.search(q, k=k, prefilter=idx, n_candidates=m)
    _, cand = amd.topk(amd.int8_scores(q, idx), m)                    # the int8 top m: (score desc, id asc), as search
    rs, ri = amd.rerank(q, corpus, cand, k=k)
    np.testing.assert_array_equal(i.cpu().numpy(), ri.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(rs))
    es, ei = r.search(q, k=k)
    fs, fi = r.search(q, k=k, prefilter=idx, n_candidates=len(corpus))
    np.testing.assert_array_equal(fi.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(fs), _bits(es))


def test_virtual_shards_agree(amd):
    """Two virtual ranks on one GPU (id_base 0 and 20): each rank's int8 stage 1, the merge of their lists, each rank's exact
    rerank, the merge of those -- the ids and score bits of the one-shard search."""
    g = torch.Generator().manual_seed(8)
    docs = _docs(g, 41)
    docs[30] = docs[4].clone()                                       # a tie across the two shards
    q = _packed(amd, [_unit(g, n) for n in (16, 33, 5)])
    k, m = 6, 10
    full = amd.pack_passages(docs, DEV, batch_size=None)
    full_idx = amd.Int8Index.build(full)
    want_s, want_i = amd.ShardedRetriever(full).search(q, k=k, prefilter=full_idx, n_candidates=m)
    shards = []
    for lo, hi in ((0, 20), (20, 41)):
        part = amd.pack_passages(docs[lo:hi], DEV, batch_size=None, id_base=lo)
        shards.append((part, amd.Int8Index.build(part)))
    assert shards[1][1].id_base == 20
    whole = amd.int8_scores(q, full_idx)
    for part, idx in shards:
        np.testing.assert_array_equal(_bits(amd.int8_scores(q, idx)), _bits(whole[:, idx.id_base:idx.id_base + len(idx)]))
    lists = [amd.topk(amd.int8_scores(q, idx), m, idx.id_base) for _, idx in shards]
    _, cand = amd.merge_gathered(torch.stack([a for a, _ in lists]), torch.stack([b for _, b in lists]), m)
    np.testing.assert_array_equal(cand.cpu().numpy(), amd.topk(whole, m)[1].cpu().numpy())
    parts = [amd.retrieval.rerank_scores(q, part, cand) for part, _ in shards]
    loc = [amd.topk(a, k, 0, b) for a, b in parts]
    s, i = amd.merge_gathered(torch.stack([a for a, _ in loc]), torch.stack([b for _, b in loc]), k)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(want_s))


def test_error_paths(amd):
    g = torch.Generator().manual_seed(9)
    with pytest.raises(NotImplementedError):
        amd.Int8Index.build(amd.pack_passages([torch.randn(4, 128)], DEV, batch_size=None))
    with pytest.raises(NotImplementedError):
        amd.Int8Index.build(amd.pack_passages([torch.randn(4, 320).to(torch.bfloat16)], DEV, batch_size=None))
    corpus = amd.pack_passages(_docs(g, 6), DEV, batch_size=None)
    other = amd.Int8Index.build(amd.pack_passages(_docs(g, 5), DEV, batch_size=None))
    with pytest.raises(ValueError, match="same documents"):
        amd.ShardedRetriever(corpus).search(_packed(amd, [_unit(g, 4)]), prefilter=other, n_candidates=3)
    idx = amd.Int8Index.build(corpus)
    q_cpu = amd.PackedQueries(tokens=_unit(g, 4), offsets=torch.tensor([0, 4], dtype=torch.int32),
                              offsets_host=torch.tensor([0, 4], dtype=torch.int32))
    with pytest.raises((ValueError, RuntimeError)):
        amd.int8_scores(q_cpu, idx)


def test_small_planted_recall(amd):
    """Each query is a noisy copy of rows of its planted page: the int8 top 1 % reranked finds the exact top 10."""
    g = torch.Generator().manual_seed(11)
    n_pages, n_q, k = 2000, 40, 10
    docs = [_unit(g, int(n)) for n in torch.randint(20, 60, (n_pages,), generator=g)]
    targets = torch.randint(0, n_pages, (n_q,), generator=g).tolist()
    qs = []
    for t in targets:
        src = docs[t].float()
        pick = torch.randint(0, src.shape[0], (16,), generator=g)
        qs.append(torch.nn.functional.normalize(src[pick] + 0.6 * torch.randn(16, 128, generator=g) / 11.3, dim=-1).to(torch.bfloat16))
    corpus = amd.pack_passages(docs, DEV, batch_size=None)
    q = _packed(amd, qs)
    r = amd.ShardedRetriever(corpus)
    _, exact = r.search(q, k=k)
    _, two = r.search(q, k=k, prefilter=amd.Int8Index.build(corpus), n_candidates=n_pages // 100)
    exact, two = exact.cpu().numpy(), two.cpu().numpy()
    recall = np.mean([len(set(exact[i]) & set(two[i])) / k for i in range(n_q)])
    assert recall >= 0.9, recall
