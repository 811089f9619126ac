"""The 1-bit sign index on the MI355X (msim_bin_*, colpali_amd.BinaryIndex / binary_scores, search(prefilter=<BinaryIndex>)).

Codes and scores are checked bit for bit against the numpy restatement in tests/binary_truth.py: the codes are sign bits, the maxima
exact integers and the score's fp32 order is documented, so nothing here has a tolerance.  The shapes are the kernel's edges: rows
around the 16-row chunk, pages of 1-3 rows so that one chunk closes several pages, page ranges of 1, 8-16 and 63 pages, queries
around the 16-token tile and past one wave's 128 tokens, and every launch form the dispatcher can choose.
"""
import numpy as np
import pytest
import torch

from tests import binary_truth as bt
from tests import int8_truth as it

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAGE_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1030)
QUERY_LENS = (0, 1, 16, 17, 32, 33, 128, 129, 300)
NT, D = 8, 4
ALL_FORMS = {(NT, 1, D), (NT, 2, D), (NT, 4, D)}            # every (NT, GW, D) msim_bin_scores instantiates

# query batches by the launch form they reach: name -> (query lengths, GW, passes)
BATCHES = {
    "gw1-one": ([9], 1, 1),
    "gw1-four": ([1, 17, 32, 5], 1, 1),
    "gw1-passes2": ([129], 1, 2),
    "gw2-seven": ([32] * 7, 2, 1),
    "gw2-passes3": ([300, 129], 2, 3),
    "gw4-tiles": ([0, 1, 16, 17, 32, 33, 128], 4, 1),
    "gw4-all-passes3": (list(QUERY_LENS), 4, 3),
    "gw4-wide": ([17, 32, 1, 0, 16, 33, 5], 4, 1),
}


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _packed(amd, q_blocks):
    return amd.pack_queries(list(q_blocks), DEV, layout="flat", compact=False)


def _plan(amd, n_q, max_q, n_d, d_rows):
    """(NT, GW, D, pages per wave range) of msim_bin_scores for a shape"""
    plan = torch.zeros(4, dtype=torch.int32)
    assert amd._lib.lib().msim_bin_scores_plan(n_q, max_q, n_d, d_rows, plan.data_ptr()) == 0
    return tuple(plan.tolist())


def _passes(max_q):
    tiles = (max_q + 15) // 16
    return max(1, (tiles + NT - 1) // NT)


def _index_of_codes(amd, codes, lens, clamp0=None, id_base=0):
    """a BinaryIndex straight from host codes uint8 [rows, 16] and page lengths"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c0 = None if clamp0 is None else torch.from_numpy(np.asarray(clamp0, dtype=np.uint8)).to(DEV)
    return amd.BinaryIndex(torch.from_numpy(codes).to(DEV), torch.from_numpy(off).to(DEV), c0,
                           torch.from_numpy(np.asarray(lens, dtype=np.int64)), id_base), off


def _truth(q, codes, off, clamp0=None):
    """the truth scores of packed queries `q` (quantized by the int8 truth) against host codes"""
    q8, sq = it.quantize_tokens(q.tokens.float().cpu().numpy())
    return bt.scores(q8, sq, q.offsets_host.numpy(), codes, off, clamp0)


def _check(amd, q, idx, codes, off, clamp0=None):
    got = amd.binary_scores(q, idx)
    want = _truth(q, codes, off, clamp0)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))
    return got, want


# ---------------------------------------------------------------------------------------------------------------------- encode
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_encode_is_bit_equal_to_the_truth(amd, dtype):
    g = torch.Generator().manual_seed(1)
    lens = [0, 1, 15, 16, 17, 33, 5]                                 # 87 rows: the last 16-row block of the launch is partial
    rows = torch.cat([_unit(g, n, dtype) for n in lens])
    raw = bt.raw_bits(rows).copy()
    raw[0, :8] = [0x0000, 0x8000, 0x0001, 0x8001, 0x7fc0, 0xffc0, 0x7e00, 0xfe00]     # +-0.0, +-subnormal, +-NaN of both formats
    raw[3] &= 0x7fff                                                 # a row of all +
    raw[4] |= 0x8000                                                 # a row of all -
    raw[20] = 0x8000                                                 # a row of -0.0
    raw[21] = 0x0000                                                 # a row of +0.0
    raw[86, ::3] ^= 0x8000
    blob = torch.from_numpy(raw.view(np.int16)).view(dtype)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    corpus = amd.PackedCorpus(blob=blob.to(DEV), offsets=torch.from_numpy(off).to(DEV),
                              clamp0=torch.tensor([1, 0, 0, 1, 0, 0, 1], dtype=torch.uint8, device=DEV),
                              lengths=torch.tensor(lens, dtype=torch.int64), id_base=11)
    idx = amd.BinaryIndex.build(corpus)
    torch.cuda.synchronize()
    want = bt.encode(raw)
    np.testing.assert_array_equal(idx.codes.cpu().numpy(), want)
    assert (want[3] == 0xff).all() and (want[4] == 0).all() and (want[20] == 0).all() and (want[21] == 0xff).all()
    assert len(idx) == len(corpus) and idx.device == DEV and idx.id_base == 11
    assert idx.nbytes == 87 * 16 + 8 * 4 + 7
    assert torch.equal(idx.offsets, corpus.offsets) and idx.offsets.data_ptr() != corpus.offsets.data_ptr()
    assert torch.equal(idx.clamp0, corpus.clamp0) and idx.clamp0.data_ptr() != corpus.clamp0.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------- scores
@pytest.fixture(scope="module")
def edges(amd):
    """The page lengths round the 16-row chunk, two empty pages at the end, clamp0 on a random half: built through
    BinaryIndex.build from a bf16 corpus."""
    g = torch.Generator().manual_seed(2)
    lens = list(PAGE_LENS) + [0, 0]
    pages = [_unit(g, n) for n in lens]
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    clamp0 = (torch.rand(len(lens), generator=g) < 0.5).to(torch.uint8)
    corpus.clamp0 = clamp0.to(DEV)
    idx = amd.BinaryIndex.build(corpus)
    codes = bt.encode(bt.raw_bits(torch.cat(pages)))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx.codes.cpu().numpy(), codes)
    return idx, codes, corpus.offsets.cpu().numpy(), clamp0.numpy(), lens


@pytest.mark.parametrize("name", list(BATCHES))
def test_scores_are_bit_equal_to_the_truth(amd, edges, name):
    idx, codes, off, clamp0, lens = edges
    qlens, gw, passes = BATCHES[name]
    assert _plan(amd, len(qlens), max(qlens), len(idx), len(codes))[:3] == (NT, gw, D) and _passes(max(qlens)) == passes
    g = torch.Generator().manual_seed(len(name) + sum(qlens))
    q = _packed(amd, [_unit(g, n) * 2 for n in qlens])
    got, want = _check(amd, q, idx, codes, off, clamp0)
    got = got.cpu().numpy()
    empty = [i for i, n in enumerate(lens) if n == 0]
    assert np.isneginf(got[:, empty]).all() and np.isfinite(np.delete(got, empty, axis=1)).all()
    for i, n in enumerate(qlens):
        if n == 0:                                                  # a 0-token query scores 0 against every page that has rows
            assert (np.delete(got[i], empty) == 0).all()


@pytest.fixture(scope="module")
def tiny_pages(amd):
    """70 000 pages of 0-3 rows (one 16-row chunk closes several pages, empty ones among them), the last three empty, clamp0 on a
    random half; the codes are random bits, so the index is made from them directly.  One wave scores a range of 8 or more pages."""
    rng = np.random.default_rng(3)
    n = 70000
    lens = rng.choice(np.array([0, 1, 1, 2, 2, 3]), n)
    lens[-3:] = 0
    if lens.sum() % 16 == 0:
        lens[0] += 1
    codes = rng.integers(0, 256, (int(lens.sum()), 16), dtype=np.uint8)
    clamp0 = (rng.random(n) < 0.5).astype(np.uint8)
    idx, off = _index_of_codes(amd, codes, lens, clamp0)
    return idx, codes, off, clamp0


@pytest.mark.parametrize("name", ["gw1-four", "gw1-passes2", "gw2-seven", "gw2-passes3", "gw4-wide"])
def test_ranges_of_one_to_three_row_pages(amd, tiny_pages, name):
    idx, codes, off, clamp0 = tiny_pages
    qlens, gw, _ = BATCHES[name]
    plan = _plan(amd, len(qlens), max(qlens), len(idx), len(codes))
    assert plan[:3] == (NT, gw, D) and plan[3] >= 8, plan
    g = torch.Generator().manual_seed(40 + sum(qlens))
    _check(amd, _packed(amd, [_unit(g, n) for n in qlens]), idx, codes, off, clamp0)


@pytest.mark.parametrize("n_pages", [63, 64, 65, 130])
@pytest.mark.parametrize("name", ["gw1-four", "gw4-wide"])
def test_page_counts_around_a_full_range(amd, n_pages, name):
    rng = np.random.default_rng(n_pages)
    lens = rng.integers(0, 41, n_pages)
    codes = rng.integers(0, 256, (int(lens.sum()), 16), dtype=np.uint8)
    clamp0 = (rng.random(n_pages) < 0.5).astype(np.uint8)
    idx, off = _index_of_codes(amd, codes, lens, clamp0)
    qlens = BATCHES[name][0]
    g = torch.Generator().manual_seed(n_pages)
    _check(amd, _packed(amd, [_unit(g, n) for n in qlens]), idx, codes, off, clamp0)


def test_full_ranges_of_63_pages(amd):
    """Enough 0-3 row pages that one query group's waves take the full 63 pages each: 65 pages past a whole number of waves, so the
    last ranges are a full one and a short one."""
    want_waves = torch.cuda.get_device_properties(DEV).multi_processor_count * 32
    n = want_waves * 63 + 65
    rng = np.random.default_rng(5)
    lens = rng.choice(np.array([0, 1, 1, 1, 2, 3]), n)
    codes = rng.integers(0, 256, (int(lens.sum()), 16), dtype=np.uint8)
    idx, off = _index_of_codes(amd, codes, lens)
    qlens = [32, 7]
    assert _plan(amd, len(qlens), 32, n, len(codes)) == (NT, 1, D, 63)
    g = torch.Generator().manual_seed(6)
    _check(amd, _packed(amd, [_unit(g, k) for k in qlens]), idx, codes, off)


def test_every_launch_form_is_reached(amd, edges, tiny_pages):
    """The shapes of the parity tests above, by the form msim_bin_scores_plan names for them: every (NT, GW, D) the dispatcher
    instantiates, one pass and several, and page ranges of 1, of 8 or more and of the full 63 pages."""
    forms, passes, ranges = set(), set(), set()
    for idx, codes in ((edges[0], edges[1]), (tiny_pages[0], tiny_pages[1])):
        for qlens, gw, n_pass in BATCHES.values():
            plan = _plan(amd, len(qlens), max(qlens), len(idx), len(codes))
            assert plan[1] == gw
            forms.add(plan[:3])
            passes.add((plan[1], _passes(max(qlens)) > 1))
            ranges.add(1 if plan[3] == 1 else 8 if plan[3] >= 8 else 0)
    assert forms == ALL_FORMS, (forms, ALL_FORMS)
    assert passes == {(gw, many) for gw in (1, 2, 4) for many in (False, True)}
    assert ranges == {1, 8}


# ----------------------------------------------------------------------------------------------------------------- phantom rows
def _negative_queries(g, qlens):
    """every token all-negative: the all-(-1) row that zero bits decode to scores +sum |q8|, above every real row"""
    return [-(_unit(g, n).abs() + 2.0 ** -6) for n in qlens]


def _phantom_scores(q):
    """what every page would score if ONE all-(-1) row reached its maxima: the sequential sum of float(sum |q8_i|) * sq_i"""
    q8, sq = it.quantize_tokens(q.tokens.float().cpu().numpy())
    assert (q8 < 0).all()
    top = np.abs(q8.astype(np.int64)).sum(axis=1).astype(np.float32)
    qo = q.offsets_host.numpy()
    out = np.zeros(len(qo) - 1, dtype=np.float32)
    for i in range(len(qo) - 1):
        t = np.float32(0)
        for k in range(qo[i], qo[i + 1]):
            t = np.float32(t + np.float32(top[k] * sq[k]))
        out[i] = t
    return out


def _ragged_range_lens(rng, n, ppw):
    """page lengths of which no wave range of `ppw` pages (a wave's row stream) ends on a 16-row chunk boundary"""
    lens = rng.choice(np.array([1, 2, 3, 5, 17]), n)
    for p0 in range(0, n, ppw):
        if lens[p0:p0 + ppw].sum() % 16 == 0:
            lens[min(p0 + ppw, n) - 1] += 1
    assert all(lens[p0:p0 + ppw].sum() % 16 for p0 in range(0, n, ppw))
    return lens


@pytest.mark.parametrize("name,n_pages", [("gw1-four", 12), ("gw4-wide", 12), ("gw1-passes2", 12), ("gw1-four", 70000), ("gw2-seven", 70000)])
def test_rows_past_a_range_never_score(amd, name, n_pages):
    qlens = [n for n in BATCHES[name][0] if n]
    g = torch.Generator().manual_seed(7)
    q = _packed(amd, _negative_queries(g, qlens))
    rng = np.random.default_rng(8)
    ppw = _plan(amd, len(qlens), max(qlens), n_pages, 2 * n_pages)[3]
    lens = _ragged_range_lens(rng, n_pages, ppw)
    assert _plan(amd, len(qlens), max(qlens), n_pages, int(lens.sum()))[3] == ppw and (ppw == 1) == (n_pages == 12)
    codes = rng.integers(0, 256, (int(lens.sum()), 16), dtype=np.uint8)
    idx, off = _index_of_codes(amd, codes, lens)
    got, want = _check(amd, q, idx, codes, off)
    assert (want < _phantom_scores(q)[:, None]).all()              # one phantom row would have changed every one of these scores


@pytest.mark.parametrize("n_pages", [12, 70000])
def test_a_winner_on_the_first_and_the_last_row_scores(amd, n_pages):
    """The mask's other side: the all-(-1) row as a REAL row -- row 0 of every even page, the last row of every odd one -- is the
    winner of every token, and the score is the one a phantom row would give."""
    qlens = [17, 32, 5]
    g = torch.Generator().manual_seed(9)
    q = _packed(amd, _negative_queries(g, qlens))
    rng = np.random.default_rng(10)
    ppw = _plan(amd, len(qlens), max(qlens), n_pages, 2 * n_pages)[3]
    lens = _ragged_range_lens(rng, n_pages, ppw)
    codes = rng.integers(0, 256, (int(lens.sum()), 16), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(lens)])
    codes[off[:-1][0::2]] = 0                                        # row 0 of the even pages
    codes[off[1:][1::2] - 1] = 0                                     # the last row of the odd pages
    idx, off = _index_of_codes(amd, codes, lens)
    got, want = _check(amd, q, idx, codes, off)
    np.testing.assert_array_equal(want.view(np.int32), np.broadcast_to(_phantom_scores(q)[:, None], want.shape).view(np.int32))


# ------------------------------------------------------------------------------------------------------------------- placement
def test_permuting_the_pages_permutes_the_bits(amd, edges):
    idx, codes, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(11)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    base = amd.binary_scores(q, idx)
    perm = np.random.default_rng(12).permutation(len(lens))
    p_codes = np.concatenate([codes[off[c]:off[c + 1]] for c in perm])
    p_idx, _ = _index_of_codes(amd, p_codes, np.asarray(lens)[perm], clamp0[perm])
    np.testing.assert_array_equal(_bits(amd.binary_scores(q, p_idx)), _bits(base)[:, perm])


def test_scores_do_not_depend_on_the_batch(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(13)
    lens = torch.randint(1, 40, (300,), generator=g).tolist()
    qs = [_unit(g, n) for n in lens]
    full = amd.binary_scores(_packed(amd, qs), idx)                       # GW 4
    for i in (0, 1, 157, 299):
        np.testing.assert_array_equal(_bits(amd.binary_scores(_packed(amd, [qs[i]]), idx)[0]), _bits(full[i]))     # GW 1
    np.testing.assert_array_equal(_bits(amd.binary_scores(_packed(amd, qs[:3]), idx)), _bits(full[:3]))
    long_q = [_unit(g, 300), qs[7]]                                       # beside a query of several passes: GW 2
    np.testing.assert_array_equal(_bits(amd.binary_scores(_packed(amd, long_q), idx)[1]), _bits(full[7]))
    again = amd.binary_scores(_packed(amd, qs), idx)
    np.testing.assert_array_equal(_bits(again), _bits(full))


# -------------------------------------------------------------------------------------------------------------- broken offsets
def test_broken_device_offsets_come_back_as_nan_over_that_range_only(amd, edges):
    idx, codes, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(14)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17)])
    assert _plan(amd, 3, 32, len(idx), len(codes))[3] == 1               # one page per range: a broken offset spoils its two pages
    want = _truth(q, codes, off, clamp0)
    for j, bad_value in ((5, len(codes) + 7), (9, -1)):
        bad = torch.from_numpy(off.copy())
        bad[j] = bad_value
        broken = amd.BinaryIndex(idx.codes, bad.to(DEV), idx.clamp0, idx.lengths)
        got = amd.binary_scores(q, broken).cpu().numpy()
        assert np.isnan(got[:, [j - 1, j]]).all()
        keep = [c for c in range(len(lens)) if c not in (j - 1, j)]
        np.testing.assert_array_equal(got[:, keep].view(np.int32), want[:, keep].view(np.int32))
    # a query whose offsets leave the token count: NaN over that query only (an empty page stays -inf)
    q8, sq = amd.quantize_queries(q)
    q_bad = q.offsets.clone()
    q_bad[2] = int(q.tokens.shape[0]) + 3
    got = amd.binary_scores_from_codes(q8, sq, q_bad, 32, idx).cpu().numpy()
    rows = [c for c, n in enumerate(lens) if n]
    assert np.isnan(got[1:, rows]).all()
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))


# ------------------------------------------------------------------------------------------------------------ two-stage search
def _docs(g, n, lo=1, hi=120):
    return [_unit(g, int(k)) for k in torch.randint(lo, hi, (n,), generator=g)]


@pytest.fixture(scope="module")
def shard(amd):
    g = torch.Generator().manual_seed(15)
    docs = _docs(g, 60)
    docs[9] = docs[3].clone()                                        # exact ties
    corpus = amd.pack_passages(docs, DEV, batch_size=None, id_base=100)
    q = _packed(amd, [_unit(g, n) for n in (32, 7, 20)])
    return corpus, amd.BinaryIndex.build(corpus), q


def test_two_stage_search_with_the_binary_prefilter(amd, shard):
    corpus, idx, q = shard
    k, m = 5, 12
    r = amd.ShardedRetriever(corpus)
    es, ei = r.search(q, k=k)
    fs, fi = r.search(q, k=k, prefilter=idx, n_candidates=len(corpus))         # every page is a candidate: the exact search
    np.testing.assert_array_equal(fi.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(fs), _bits(es))
    s, i = r.search(q, k=k, prefilter=idx, n_candidates=m)
    _, cand = amd.topk(amd.binary_scores(q, idx), m, idx.id_base)              # the top m of stage 1: (score desc, id asc), as search
    rs, ri = amd.rerank(q, corpus, cand, k=k)
    np.testing.assert_array_equal(i.cpu().numpy(), ri.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(rs))
    exact = amd.maxsim_scores(q, corpus)                                       # every returned score carries the exact scan's bits
    assert (i >= 100).all()
    np.testing.assert_array_equal(_bits(s), _bits(torch.gather(exact, 1, i - 100)))


def test_two_stage_search_with_a_filter_and_with_groups(amd, shard):
    corpus, idx, q = shard
    n, k, m = len(corpus), 5, 12
    g = torch.Generator().manual_seed(16)
    allowed = torch.rand(n, generator=g) < 0.5
    r = amd.ShardedRetriever(corpus)
    s, i = r.search(q, k=k, prefilter=idx, n_candidates=m, filter=amd.PageFilter.from_mask(allowed.to(DEV), 100))
    coarse = amd.binary_scores(q, idx).masked_fill(~allowed.to(DEV)[None, :], float("-inf"))
    _, cand = amd.topk(coarse, m, idx.id_base)
    assert allowed[(cand - 100).cpu()].all()                                   # every candidate is an allowed page
    rs, ri = amd.rerank(q, corpus, cand, k=k)
    np.testing.assert_array_equal(i.cpu().numpy(), ri.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(rs))
    assert allowed[(i - 100).cpu()].all()

    labels = torch.randint(0, 9, (n,), generator=g)
    gs, gid, gpage = r.search(q, k=k, prefilter=idx, n_candidates=m, group_by=amd.PageGroups.from_labels(labels.to(DEV), 100))
    _, cand = amd.topk(amd.binary_scores(q, idx), m, idx.id_base)
    ps, pi = (t.cpu() for t in amd.rerank(q, corpus, cand, k=m))               # the reranked list, best page first (score desc, id asc)
    for row in range(len(q)):
        best = {}
        for sc, page in zip(ps[row].tolist(), pi[row].tolist()):
            best.setdefault(int(labels[page - 100]), (sc, page))                # a document's first entry is its best page
        want = sorted(((sc, d, page) for d, (sc, page) in best.items()), key=lambda e: (-e[0], e[1]))[:k]
        want += [(float("-inf"), -1, -1)] * (k - len(want))
        assert gid[row].tolist() == [d for _, d, _ in want] and gpage[row].tolist() == [p for _, _, p in want]
        assert gs[row].tolist() == [sc for sc, _, _ in want]


def test_two_stage_search_over_a_residual_corpus(amd):
    g = torch.Generator().manual_seed(17)
    K = 256
    C = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).to(torch.bfloat16)
    pages = []
    for n in torch.randint(1, 60, (40,), generator=g).tolist():
        near = C[torch.randint(0, K, (n,), generator=g)].float()
        pages.append(torch.nn.functional.normalize(near + 0.035 * torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16))
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=7)
    idx = amd.BinaryIndex.build(corpus)                                        # from the bf16 pages, before they are dropped
    cut = (torch.arange(1, 4, dtype=torch.float32) - 2) * 0.03
    edges_ = torch.cat([cut[:1] - 0.04, cut, cut[-1:] + 0.04])
    rc = amd.ResidualCorpus.build(corpus, index=amd.CentroidIndex.build(corpus, centroids=C.to(DEV)), bits=2, cutoffs=cut.to(DEV),
                                  weights=((edges_[:-1] + edges_[1:]) / 2).contiguous().to(DEV))
    q = _packed(amd, [torch.nn.functional.normalize(C[torch.randint(0, K, (n,), generator=g)].float()
                                                     + 0.1 * torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16) for n in (32, 9)])
    k, m = 4, 10
    s, i = amd.ShardedRetriever(rc).search(q, k=k, prefilter=idx, n_candidates=m)
    _, cand = amd.topk(amd.binary_scores(q, idx), m, idx.id_base)
    rs, ri = amd.residual_rerank_scores(q, rc, cand)
    ws, wi = amd.topk(rs, k, 0, ri)
    np.testing.assert_array_equal(i.cpu().numpy(), wi.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(ws))
    assert (i >= 7).all()


# --------------------------------------------------------------------------------------------------------------------- hipGraph
def test_a_captured_binary_scores_replays_the_eager_bits(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(18)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    first = amd.binary_scores(q, idx).clone()
    out = torch.empty_like(first)
    amd.binary_scores(q, idx, out=out)                               # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.binary_scores(q, idx, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(first))


def test_error_paths(amd, shard):
    corpus, idx, q = shard
    g = torch.Generator().manual_seed(19)
    with pytest.raises(NotImplementedError, match="the binary index takes"):
        amd.BinaryIndex.build(amd.pack_passages([torch.randn(4, 128)], DEV, batch_size=None))
    with pytest.raises(NotImplementedError, match="the binary index takes"):
        amd.BinaryIndex.build(amd.pack_passages([torch.randn(4, 320).to(torch.bfloat16)], DEV, batch_size=None))
    other = amd.BinaryIndex.build(amd.pack_passages(_docs(g, 5), DEV, batch_size=None))
    with pytest.raises(ValueError, match="same documents"):
        amd.ShardedRetriever(corpus).search(q, prefilter=other, n_candidates=3)
    with pytest.raises(ValueError, match="out must be"):
        amd.binary_scores(q, idx, out=torch.empty(3, 5, device=DEV))
