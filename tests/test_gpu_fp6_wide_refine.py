"""The list form of the e2m3 scorer of the wide FP4 index (msim_f4w_candidates_q6, fp6_wide_rerank_scores) and search with the e2m3
hooks on a 320-wide shard, on the GPU: ShardedRetriever / LiveCorpus(fp4_wide_score_fn=fp6_wide_scores,
fp4_wide_rerank_fn=fp6_wide_rerank_scores).  The independent reference is tests/fp6_wide_truth.py; nothing here has a tolerance:
every comparison is on the int32 view of the scores.  The list sizes of the search tests come from the TRUTH's worst e2m3 rank of an
exact top-k page, never from the code under test."""
import numpy as np
import pytest
import torch

from tests import fp4_wide_truth as wt
from tests import fp6_wide_truth as f6w
from tests import test_gpu_fp4_wide as tw
from tests.test_gpu_fp4_wide import DEV, PAGE_LENS, W, _bits, _index_of_codes, _packed, _random_codes, _unit
from tests.test_gpu_fp4_wide_refine import MAX_Q, NEG_INF_BITS, _expected, _lists, _plan, _same
from tests.test_gpu_fp6_wide import _truth, amd  # noqa: F401  (`amd` is a fixture)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------- bits against the scan
@pytest.fixture(scope="module")
def edge_codes():
    """tests/test_gpu_fp4_wide_refine.py's: random codes over the page lengths round the 16-row chunk, one page of 0 rows"""
    rng = np.random.default_rng(60)
    lens = list(PAGE_LENS)
    codes, scales = _random_codes(rng, sum(lens))
    clamp0 = (np.arange(len(lens)) % 2).astype(np.uint8)
    return codes, scales, lens, clamp0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_bits_equal_the_scan_and_the_truth_in_every_form(amd, edge_codes, dtype):
    """Every entry is bit-identical to fp6_wide_scores gathered at the list (and to the truth): batches whose longest query is
    1 .. 128 tokens -- NT = 1, 2, 4, 8, each at both of its edges -- with a 0-token query in each; lists of width 1, 7 and 64 with
    duplicates, -1 and ids just outside the shard; both id_bases; clamp0 none and mixed; a page of 0 rows among the pages."""
    codes, scales, lens, mixed = edge_codes
    assert 0 in lens
    n = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    g = torch.Generator().manual_seed(61)
    rng = np.random.default_rng(62)
    nt_seen = set()
    for max_q in MAX_Q:
        q_lens = sorted({max_q, 1, max(max_q // 2, 1), max(max_q - 1, 1)}) + [0]
        q = _packed(amd, [tw._scaled(g, k, dtype) for k in q_lens])
        n_q = len(q_lens)
        for clamp0 in (None, mixed):
            want = _truth(q, codes, scales, off, clamp0)
            for id_base in (0, 1000):
                idx, _ = _index_of_codes(amd, codes, scales, lens, clamp0, id_base)
                full = amd.fp6_wide_scores(q, idx).cpu().numpy()
                np.testing.assert_array_equal(full.view(np.int32), want.view(np.int32))
                for cand in _lists(rng, n_q, n, id_base):
                    nt_seen.add(_plan(amd, n_q, max_q, cand.shape[1])[0])       # msim_f4w_candidates_plan describes both codes
                    s, i = amd.fp6_wide_rerank_scores(q, idx, torch.from_numpy(cand).to(DEV))
                    exp_s, exp_i = _expected(want, cand, id_base)
                    np.testing.assert_array_equal(_bits(s), _expected(full, cand, id_base)[0],      # the scan, gathered at the list
                                                  err_msg=f"max_q={max_q} m={cand.shape[1]} id_base={id_base}")
                    np.testing.assert_array_equal(_bits(s), exp_s)
                    np.testing.assert_array_equal(i.cpu().numpy(), exp_i)
                    assert (_bits(s)[exp_i < 0] == NEG_INF_BITS).all()          # -1 and foreign ids: (-inf, -1)
                    empty = np.isin(cand - id_base, [c for c, k in enumerate(lens) if k == 0]) & (exp_i >= 0)
                    assert empty.any() or cand.shape[1] < 64
                    assert (_bits(s)[empty] == NEG_INF_BITS).all()              # a page of 0 rows: -inf under its own id
    assert nt_seen == {1, 2, 4, 8}                                    # every instantiation was launched


def test_more_than_128_tokens_raises(amd, edge_codes):
    codes, scales, lens, mixed = edge_codes
    idx, _ = _index_of_codes(amd, codes, scales, lens, mixed, 0)
    g = torch.Generator().manual_seed(63)
    cand = torch.zeros((2, 3), dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="at most 128 tokens .got 129."):
        amd.fp6_wide_rerank_scores(_packed(amd, [_unit(g, 129), _unit(g, 4)]), idx, cand)
    s, _ = amd.fp6_wide_rerank_scores(_packed(amd, [_unit(g, 128), _unit(g, 4)]), idx, cand)
    assert torch.isfinite(s).all()
    fake = 1 << 20                                                    # the ABI refuses a 129-token bound before it looks at the device
    assert amd._lib.lib().msim_f4w_candidates_q6(fake, fake, fake, 2, 133, 129, fake, fake, fake, None, 11, 346, 320, fake, 3, 3, 0, fake, 3,
                                                 None, None) == -2


def test_duplicates_a_broadcast_row_and_out(amd, edge_codes):
    codes, scales, lens, mixed = edge_codes
    n = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    idx, _ = _index_of_codes(amd, codes, scales, lens, mixed, 40)
    g = torch.Generator().manual_seed(64)
    q = _packed(amd, [_unit(g, k) for k in (32, 5, 17, 1)])
    want = _truth(q, codes, scales, off, mixed)
    dup = np.array([[43, 43, 43, 40, -1, 43, 39, 40 + n, 40]] * 4, dtype=np.int64)      # an id listed four times is scored four times
    s, i = amd.fp6_wide_rerank_scores(q, idx, torch.from_numpy(dup).to(DEV))
    exp_s, exp_i = _expected(want, dup, 40)
    np.testing.assert_array_equal(_bits(s), exp_s)
    np.testing.assert_array_equal(i.cpu().numpy(), exp_i)
    assert (_bits(s)[:, [0, 1, 2, 5]] == _bits(s)[:, :1]).all()
    # one list row for every query: a broadcast (stride 0) row is copied
    row = torch.from_numpy(dup[:1]).to(DEV)
    sb, ib = amd.fp6_wide_rerank_scores(q, idx, row.expand(4, dup.shape[1]))
    np.testing.assert_array_equal(_bits(sb), exp_s)
    np.testing.assert_array_equal(ib.cpu().numpy(), exp_i)
    # out=: written in place and returned
    out = torch.full((4, dup.shape[1]), 7.0, dtype=torch.float32, device=DEV)
    so, _ = amd.fp6_wide_rerank_scores(q, idx, torch.from_numpy(dup).to(DEV), out=out)
    assert so.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_bits(out), exp_s)
    with pytest.raises(ValueError):
        amd.fp6_wide_rerank_scores(q, idx, torch.from_numpy(dup).to(DEV), out=torch.empty((4, 3), device=DEV))


def test_a_broken_offset_becomes_nan_in_that_entry_only(amd, edge_codes):
    """No broken offset below becomes an address: the kernel reads d_off[d] and d_off[d + 1] for an id it has checked against
    [id_base, id_base + n_d), and returns NaN unless 0 <= r0 <= r1 <= d_rows and r1 - r0 <= 2^23 before it forms the descriptors.
    The offsets are bad data in a tensor of the right size, as tests/test_gpu_fp4_wide_refine.py has them."""
    codes, scales, lens, mixed = edge_codes
    n, rows = len(lens), sum(lens)
    idx, off = _index_of_codes(amd, codes, scales, lens, mixed, 0)
    g = torch.Generator().manual_seed(64)
    q = _packed(amd, [_unit(g, k) for k in (32, 5, 17)])
    want = _truth(q, codes, scales, off, mixed)
    cand = np.stack([np.random.default_rng(65 + i).permutation(np.arange(-1, n + 1)) for i in range(3)]).astype(np.int64)
    exp_s, exp_i = _expected(want, cand, 0)
    for j, value, spoiled in ((10, off[9] - 1, (9, 10)), (10, rows + 7, (9, 10)), (5, -1, (4, 5))):
        bad = off.copy()
        bad[j] = value
        if j == 10:
            bad[11] = value if value > rows else off[11]              # page 10 stays a page of 0 rows where it can
        broken = amd.Fp4WideIndex(idx.codes, idx.scales, torch.from_numpy(bad).to(DEV), idx.clamp0, idx.lengths)
        s, i = amd.fp6_wide_rerank_scores(q, broken, torch.from_numpy(cand).to(DEV))
        got = _bits(s)
        hit = np.isin(cand, spoiled)
        nan_pages = [c for c in spoiled if not (0 <= bad[c] <= bad[c + 1] <= rows)]
        assert nan_pages
        assert np.isnan(s.cpu().numpy()[np.isin(cand, nan_pages)]).all()
        np.testing.assert_array_equal(got[~hit], exp_s[~hit])
        np.testing.assert_array_equal(i.cpu().numpy(), exp_i)


def test_a_captured_rerank_follows_the_list(amd, edge_codes):
    codes, scales, lens, mixed = edge_codes
    idx, _ = _index_of_codes(amd, codes, scales, lens, mixed, 50)
    g = torch.Generator().manual_seed(68)
    q = _packed(amd, [_unit(g, k) for k in (32, 5, 17, 64, 1)])
    rng = np.random.default_rng(69)
    first, second = (torch.from_numpy(50 + rng.integers(-1, len(lens) + 1, (5, 9))).to(DEV) for _ in range(2))
    cand = first.clone()
    out = torch.empty((5, 9), dtype=torch.float32, device=DEV)
    amd.fp6_wide_rerank_scores(q, idx, cand, out=out)                # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, ids = amd.fp6_wide_rerank_scores(q, idx, cand, out=out)
    for lst in (second, first):
        cand.copy_(lst)                                               # in place: the graph holds the tensor's address
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_s, want_i = amd.fp6_wide_rerank_scores(q, idx, lst)
        np.testing.assert_array_equal(_bits(out), _bits(want_s))
        np.testing.assert_array_equal(ids.cpu().numpy(), want_i.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ the search
K, ID_BASE = tw.K, 100


def e2m3_ranks(qs, pages, off, allowed=None):
    """tests/test_gpu_fp4_wide.py: fp4_ranks, from the e2m3 truth: rank[q, c] = pages (allowed ones) that (score desc, id asc)
    puts before page c"""
    S = f6w.score_blocks([wt.raw_bits(q) for q in qs], wt.raw_bits(torch.cat(pages)), off).astype(np.float64)
    if allowed is not None:
        S = np.where(allowed[None, :], S, -np.inf)
    order = np.argsort(-S, axis=1, kind="stable")
    ranks = np.empty_like(order)
    for i in range(len(qs)):
        ranks[i, order[i]] = np.arange(S.shape[1])
    return ranks


@pytest.fixture(scope="module")
def search(amd):
    """the 300-page planted fixture of tests/test_gpu_fp4_wide.py, with the e2m3 truth's ranks"""
    pages, qs = tw.search_case()
    off = np.concatenate([[0], np.cumsum([len(p) for p in pages])])
    exact = tw.exact_scores(qs, torch.cat(pages).double().numpy(), off)
    ranks = e2m3_ranks(qs, pages, off)
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=ID_BASE)
    r = amd.ShardedRetriever(corpus, fp4_wide_score_fn=amd.fp6_wide_scores, fp4_wide_rerank_fn=amd.fp6_wide_rerank_scores)
    return corpus, amd.Fp4WideIndex.build(corpus), _packed(amd, qs), pages, qs, off, exact, ranks, r


def test_two_and_three_stage_search_return_the_exact_search(amd, search):
    corpus, idx, q, pages, qs, off, exact, ranks, r = search
    n = len(corpus)
    m = tw.worst_rank(exact, ranks) + 1                              # the shortest list that holds every exact top-k page
    print(f"worst e2m3 rank of an exact top-{K} page: {m - 1}")
    assert K <= m < n
    es, ei = r.search(q, k=K)
    assert (ei[:, 0].cpu() - ID_BASE).tolist() == [37 * j + 11 for j in range(6)]       # the planted pages come first
    _same(r.search(q, k=K, prefilter=idx, n_candidates=m), (es, ei))
    all_ids = torch.arange(ID_BASE, ID_BASE + n, dtype=torch.int64, device=DEV).expand(len(qs), n)
    _same(r.search(q, k=K, candidates=all_ids, refine=idx, n_refine=m), (es, ei))
    _same(r.search(q, k=K, prefilter=idx, n_candidates=min(2 * m, n), refine=idx, n_refine=m), (es, ei))
    # stage 1 is fp6_wide_scores: the list is the truth's, in (score desc, id asc) order
    _, cand = amd.topk(amd.fp6_wide_scores(q, idx), m, idx.id_base)
    want = np.argsort(-_truth(q, *wt.encode(wt.raw_bits(torch.cat(pages))), off).astype(np.float64), axis=1, kind="stable")[:, :m]
    np.testing.assert_array_equal(cand.cpu().numpy() - ID_BASE, want)


def test_search_with_a_filter_and_with_groups(amd, search):
    corpus, idx, q, pages, qs, off, exact, ranks, r = search
    n = len(corpus)
    all_ids = torch.arange(ID_BASE, ID_BASE + n, dtype=torch.int64, device=DEV).expand(len(qs), n)
    g = torch.Generator().manual_seed(16)
    allowed = torch.rand(n, generator=g) < 0.5
    m = tw.worst_rank(exact, e2m3_ranks(qs, pages, off, allowed.numpy()), allowed=allowed.numpy()) + 1
    assert K <= m <= int(allowed.sum())
    flt = amd.PageFilter.from_mask(allowed.to(DEV), ID_BASE)
    es, ei = r.search(q, k=K, filter=flt)
    assert allowed[(ei - ID_BASE).cpu()].all()
    _same(r.search(q, k=K, prefilter=idx, n_candidates=m, filter=flt), (es, ei))
    _same(r.search(q, k=K, candidates=all_ids, refine=idx, n_refine=m, filter=flt), (es, ei))

    labels = torch.randint(0, 60, (n,), generator=g)
    lab = labels.numpy()
    best = np.full((len(qs), 60), -1)
    doc_s = np.full((len(qs), 60), -np.inf)
    for c in range(n):                                               # every document's best page, the lower id on a tie
        better = exact[:, c] > doc_s[:, lab[c]]
        doc_s[better, lab[c]], best[better, lab[c]] = exact[better, c], c
    top_docs = np.argsort(-doc_s, axis=1, kind="stable")[:, :K]
    mg = int(np.take_along_axis(ranks, np.take_along_axis(best, top_docs, axis=1), axis=1).max()) + 1
    assert K <= mg < n
    groups = amd.PageGroups.from_labels(labels.to(DEV), ID_BASE)
    want = r.search(q, k=K, group_by=groups)
    _same(r.search(q, k=K, prefilter=idx, n_candidates=mg, group_by=groups), want)
    _same(r.search(q, k=K, candidates=all_ids, refine=idx, n_refine=mg, group_by=groups), want)


# ------------------------------------------------------------------------------------------------------------------------ live
def test_a_live_wide_shard_with_the_e2m3_hooks(amd):
    """After add / delete / compact, search(prefilter=live.fp4_index()) and search(refine=live.fp4_index()) with the e2m3 hooks equal
    the same search over a frozen retriever built from the survivors, and no deleted page is ever returned."""
    g = torch.Generator().manual_seed(70)
    lens = torch.randint(1, 101, (40,), generator=g).tolist()
    lens[3], lens[17] = 1, 100
    pages = [_unit(g, k) for k in lens]
    q = _packed(amd, [_unit(g, k) for k in (5, 16, 17, 32, 33)])
    hooks = dict(fp4_wide_score_fn=amd.fp6_wide_scores, fp4_wide_rerank_fn=amd.fp6_wide_rerank_scores)
    live = amd.LiveCorpus(sum(lens) + 64, 44, DEV, width=W, id_base=ID_BASE, **hooks)
    live.add(pages[:30])
    assert isinstance(live.fp4_index(), amd.Fp4WideIndex)
    dead = list(range(ID_BASE + 1, ID_BASE + 30, 3))
    live.delete(dead)
    live.add(pages[30:])                                             # the index is kept in step by add ...
    dead += [ID_BASE + 33, ID_BASE + 39]
    live.delete(dead[-2:])
    alive = [c for c in range(40) if c + ID_BASE not in dead]
    fresh = amd.pack_passages([pages[c] for c in alive], DEV, batch_size=None)
    fresh_idx = amd.Fp4WideIndex.build(fresh)
    fresh_ids = torch.arange(len(alive), dtype=torch.int64, device=DEV).expand(5, len(alive))
    slot = torch.tensor(alive, dtype=torch.int64, device=DEV) + ID_BASE
    all_ids = torch.arange(ID_BASE, ID_BASE + 40, dtype=torch.int64, device=DEV).expand(5, 40)
    r = amd.ShardedRetriever(fresh, **hooks)
    for compacted in (False, True):
        if compacted:
            live.compact()                                           # ... and by compact
        for m in (1, 7, len(alive) - 1):
            for got, want in ((live.search(q, tw.K, prefilter=live.fp4_index(), n_candidates=m),
                               r.search(q, tw.K, prefilter=fresh_idx, n_candidates=m)),
                              (live.search(q, tw.K, candidates=all_ids, refine=live.fp4_index(), n_refine=m),
                               r.search(q, tw.K, candidates=fresh_ids, refine=fresh_idx, n_refine=m))):
                s, i = got
                assert not np.isin(i.cpu().numpy(), dead).any()
                ws, wi = want
                wi = torch.where(wi >= 0, slot[wi.clamp(min=0)], wi)
                _same((s, i), (ws, wi))
        # the live index's bits are the frozen one's
        idx = live.fp4_index()
        full = amd.fp6_wide_scores(q, idx)[:, torch.tensor(alive, device=DEV)]
        np.testing.assert_array_equal(_bits(full), _bits(amd.fp6_wide_scores(q, fresh_idx)))
    live.check()
