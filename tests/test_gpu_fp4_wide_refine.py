"""The list form of the wide FP4 scorer (msim_f4w_candidates, fp4_wide_rerank_scores) and the three-stage route
search(refine=<Fp4WideIndex>, n_refine=) on a 320-wide shard, on the GPU.  The independent reference is tests/fp4_wide_truth.py;
nothing here has a tolerance: every comparison is on the int32 view of the scores."""
import numpy as np
import pytest
import torch

from tests import fp4_wide_truth as wt
from tests.test_gpu_fp4_wide import (DEV, PAGE_LENS, _bits, _index_of_codes, _packed, _random_codes, _truth, _unit,  # noqa: F401
                                     amd)                            # `amd` is a fixture

pytestmark = pytest.mark.gpu

NEG_INF_BITS = np.array([-np.inf], dtype=np.float32).view(np.int32)[0]
MAX_Q = (1, 16, 17, 32, 33, 64, 65, 128)             # a batch's longest query: every NT in {1, 2, 4, 8}, each at both of its edges


def _plan(amd, n_q, max_q, m):
    plan = torch.zeros(4, dtype=torch.int32)
    assert amd._lib.lib().msim_f4w_candidates_plan(n_q, max_q, m, plan.data_ptr()) == 0
    return tuple(plan.tolist())


def _expected(want, cand, id_base):
    """(score bits int32 [n_q, m], ids int64 [n_q, m]) the list form must return for `cand` (host int64) given the [n_q, n] matrix"""
    n = want.shape[1]
    local = cand - id_base
    valid = (cand >= 0) & (local >= 0) & (local < n)
    s = np.full(cand.shape, -np.inf, dtype=np.float32)
    rows = np.broadcast_to(np.arange(cand.shape[0])[:, None], cand.shape)
    s[valid] = want[rows[valid], local[valid]]
    return s.view(np.int32), np.where(valid, cand, -1)


def _lists(rng, n_q, n, id_base):
    """lists of width 1, 7 and 64: every page, duplicates, -1, id_base - 1 and id_base + n, in another order for every query"""
    special = np.array([-1, id_base - 1, id_base + n], dtype=np.int64)
    wide = np.stack([rng.permutation(np.concatenate([id_base + np.arange(n), special, id_base + rng.integers(0, n, 64 - n - 3)]))
                     for _ in range(n_q)])
    seven = np.stack([rng.permutation(np.concatenate([id_base + rng.integers(0, n, 4), special])) for _ in range(n_q)])
    one = np.concatenate([special, id_base + rng.integers(0, n, max(n_q - 3, 0))])[:n_q, None]
    return [one if n_q >= 3 else id_base + rng.integers(0, n, (n_q, 1)), seven, wide]


# ----------------------------------------------------------------------------------------------------- bits against the truth
@pytest.fixture(scope="module")
def edge_codes():
    rng = np.random.default_rng(60)
    lens = list(PAGE_LENS)
    codes, scales = _random_codes(rng, sum(lens))
    clamp0 = (np.arange(len(lens)) % 2).astype(np.uint8)
    return codes, scales, lens, clamp0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_bits_equal_the_truth_in_every_form(amd, edge_codes, dtype):
    codes, scales, lens, mixed = edge_codes
    n = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    g = torch.Generator().manual_seed(61)
    rng = np.random.default_rng(62)
    nt_seen = set()
    for max_q in MAX_Q:
        q_lens = sorted({max_q, 1, max(max_q // 2, 1), max(max_q - 1, 1)}) + [0]
        q = _packed(amd, [_unit(g, k, dtype) for k in q_lens])
        n_q = len(q_lens)
        for clamp0 in (None, mixed):
            want = _truth(q, codes, scales, off, clamp0)
            for id_base in (0, 1000):
                idx, _ = _index_of_codes(amd, codes, scales, lens, clamp0, id_base)
                full = amd.fp4_wide_scores(q, idx).cpu().numpy()
                np.testing.assert_array_equal(full.view(np.int32), want.view(np.int32))
                for cand in _lists(rng, n_q, n, id_base):
                    nt_seen.add(_plan(amd, n_q, max_q, cand.shape[1])[0])
                    s, i = amd.fp4_wide_rerank_scores(q, idx, torch.from_numpy(cand).to(DEV))
                    exp_s, exp_i = _expected(want, cand, id_base)
                    np.testing.assert_array_equal(_bits(s), exp_s, err_msg=f"max_q={max_q} m={cand.shape[1]} id_base={id_base}")
                    np.testing.assert_array_equal(i.cpu().numpy(), exp_i)
                    np.testing.assert_array_equal(_bits(s), _expected(full, cand, id_base)[0])       # the scan, gathered at the list
                    assert (_bits(s)[exp_i < 0] == NEG_INF_BITS).all()
    assert nt_seen == {1, 2, 4, 8}                                    # every instantiation was launched


def test_the_plan_takes_the_smallest_tile_count_that_holds_the_query(amd):
    assert [_plan(amd, 5, max_q, 7)[0] for max_q in MAX_Q] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert _plan(amd, 5, 0, 7)[0] == 1
    nt, d, waves, wgs = _plan(amd, 5, 32, 7)
    assert (nt, waves, wgs) == (2, 4, 9) and 1 <= d <= 4              # waves per workgroup, ceil(35 / 4) workgroups


# --------------------------------------------------------------------------------------------------------- all-negative pages
def test_all_negative_pages_score_negative(amd):
    g = torch.Generator().manual_seed(63)
    row = _unit(g, 1)
    pages = [row.repeat(17, 1), row.repeat(33, 1)]
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=5)
    idx = amd.Fp4WideIndex.build(corpus)
    codes, scales = idx.codes.cpu().numpy(), idx.scales.cpu().numpy()
    np.testing.assert_array_equal(codes, wt.encode(wt.raw_bits(torch.cat(pages)))[0])
    off = np.array([0, 17, 50])
    cand = torch.tensor([[6, 5, 6]], dtype=torch.int64, device=DEV)
    for q_len in (1, 17, 40, 70):                                     # NT = 1, 2, 4, 8: each has its own masked path
        q = _packed(amd, [-row.repeat(q_len, 1)])
        want = _truth(q, codes, scales, off, None)
        assert (want < 0).all()
        s, i = amd.fp4_wide_rerank_scores(q, idx, cand)
        assert (s < 0).all()                                          # a made-up zero row of the last partial chunk would make it 0
        np.testing.assert_array_equal(_bits(s), _expected(want, cand.cpu().numpy(), 5)[0])
        clamped = amd.Fp4WideIndex(idx.codes, idx.scales, idx.offsets, torch.ones(2, dtype=torch.uint8, device=DEV), idx.lengths, 5)
        s0, _ = amd.fp4_wide_rerank_scores(q, clamped, cand)
        assert (_bits(s0) == 0).all()
        np.testing.assert_array_equal(_bits(s0), _expected(_truth(q, codes, scales, off, np.ones(2, np.uint8)), cand.cpu().numpy(), 5)[0])


# -------------------------------------------------------------------------------------------------------------- broken inputs
def test_broken_inputs_become_nan_and_nothing_else_moves(amd, edge_codes):
    """No broken offset below becomes an address: the kernel reads d_off[d] and d_off[d + 1] for an id it has checked against
    [id_base, id_base + n_d), and returns NaN unless 0 <= r0 <= r1 <= d_rows and r1 - r0 <= 2^23 before it forms the descriptors;
    the same for q_off[q], q_off[q + 1] against q_rows and 16 NT before a query row is read."""
    codes, scales, lens, mixed = edge_codes
    n, rows = len(lens), sum(lens)
    idx, off = _index_of_codes(amd, codes, scales, lens, mixed, 0)
    g = torch.Generator().manual_seed(64)
    q = _packed(amd, [_unit(g, k) for k in (32, 5, 17)])
    want = _truth(q, codes, scales, off, mixed)
    cand = np.stack([np.random.default_rng(65 + i).permutation(np.arange(-1, n + 1)) for i in range(3)]).astype(np.int64)
    exp_s, exp_i = _expected(want, cand, 0)
    # (j, value): off[j] = value.  Page 9 ends before it starts; page 9 reaches past d_rows (page 10, 0 rows, then runs backwards);
    # a negative offset in the middle spoils the page that ends there and the page that starts there
    for j, value, spoiled in ((10, off[9] - 1, (9, 10)), (10, rows + 7, (9, 10)), (5, -1, (4, 5))):
        bad = off.copy()
        bad[j] = value
        if j == 10:
            bad[11] = value if value > rows else off[11]              # page 10 stays a page of 0 rows where it can
        broken = amd.Fp4WideIndex(idx.codes, idx.scales, torch.from_numpy(bad).to(DEV), idx.clamp0, idx.lengths)
        s, i = amd.fp4_wide_rerank_scores(q, broken, torch.from_numpy(cand).to(DEV))
        got = _bits(s)
        hit = np.isin(cand, spoiled)
        nan_pages = [c for c in spoiled if not (0 <= bad[c] <= bad[c + 1] <= rows)]
        assert nan_pages
        assert np.isnan(s.cpu().numpy()[np.isin(cand, nan_pages)]).all()
        np.testing.assert_array_equal(got[~hit], exp_s[~hit])
        np.testing.assert_array_equal(i.cpu().numpy(), exp_i)

    # a 129-token query behind a max_q_tokens of 128, and a query whose offsets leave the token count, through the raw entry
    L = amd._lib.lib()
    long_q = _packed(amd, [_unit(g, k) for k in (129, 5, 128)])
    qc, qs = amd.fp4_wide_quantize_queries(long_q)
    want = _truth(long_q, codes, scales, off, mixed)
    exp_s, exp_i = _expected(want, cand, 0)
    has_rows = np.isin(cand, [c for c, k in enumerate(lens) if k])
    d_cand = torch.from_numpy(cand).to(DEV)

    def raw(q_off):
        out = torch.zeros(cand.shape, dtype=torch.float32, device=DEV)
        ids = torch.zeros(cand.shape, dtype=torch.int64, device=DEV)
        rc = L.msim_f4w_candidates(qc.data_ptr(), qs.data_ptr(), q_off.data_ptr(), 3, int(qc.shape[0]), 128, idx.codes.data_ptr(),
                                   idx.scales.data_ptr(), idx.offsets.data_ptr(), idx.clamp0.data_ptr(), n, rows, 320, d_cand.data_ptr(),
                                   cand.shape[1], cand.shape[1], 0, out.data_ptr(), cand.shape[1], ids.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return out.cpu().numpy(), ids.cpu().numpy()

    s, i = raw(long_q.offsets)
    assert np.isnan(s[0][has_rows[0]]).all()
    np.testing.assert_array_equal(s.view(np.int32)[0][~has_rows[0]], exp_s[0][~has_rows[0]])
    np.testing.assert_array_equal(s.view(np.int32)[1:], exp_s[1:])
    np.testing.assert_array_equal(i, exp_i)
    q_bad = long_q.offsets.clone()
    q_bad[3] = int(qc.shape[0]) + 3
    s, i = raw(q_bad)
    assert np.isnan(s[[0, 2]][has_rows[[0, 2]]]).all()
    np.testing.assert_array_equal(s.view(np.int32)[1], exp_s[1])
    np.testing.assert_array_equal(i, exp_i)


# ------------------------------------------------------------------------------------------------------- past 2 GiB of codes
def test_a_page_past_two_gib_of_codes(amd):
    if torch.cuda.mem_get_info(DEV)[0] < 4 << 30:
        pytest.skip("needs 4 GB of free device memory")
    rows = 14_200_000 + 49
    rng = np.random.default_rng(66)
    c_head, s_head = _random_codes(rng, 16)
    c_tail, s_tail = _random_codes(rng, 33)
    codes = torch.zeros((rows, wt.ROW_BYTES), dtype=torch.uint8, device=DEV)
    scales = torch.zeros((rows,), dtype=torch.uint8, device=DEV)
    codes[:16], scales[:16] = torch.from_numpy(c_head).to(DEV), torch.from_numpy(s_head).to(DEV)
    codes[rows - 33:], scales[rows - 33:] = torch.from_numpy(c_tail).to(DEV), torch.from_numpy(s_tail).to(DEV)
    assert (rows - 33) * wt.ROW_BYTES > 1 << 31
    lens = [16, rows - 49, 33]
    off = torch.tensor([0, 16, rows - 33, rows], dtype=torch.int32, device=DEV)
    idx = amd.Fp4WideIndex(codes, scales, off, None, torch.tensor(lens), 0)
    g = torch.Generator().manual_seed(67)
    q = _packed(amd, [_unit(g, k) for k in (33, 4)])
    cand = np.array([[2, 0, 2, -1], [0, 2, 3, 0]], dtype=np.int64)
    want = _truth(q, np.concatenate([c_head, c_tail]), np.concatenate([s_head, s_tail]), np.array([0, 16, 49]), None)
    want3 = np.stack([want[:, 0], np.full(2, np.nan, np.float32), want[:, 1]], axis=1)     # the middle page is never listed
    s, i = amd.fp4_wide_rerank_scores(q, idx, torch.from_numpy(cand).to(DEV))
    exp_s, exp_i = _expected(want3, cand, 0)
    np.testing.assert_array_equal(_bits(s), exp_s)
    np.testing.assert_array_equal(i.cpu().numpy(), exp_i)
    del codes, scales, idx
    torch.cuda.empty_cache()


# -------------------------------------------------------------------------------------------------------------------- hipGraph
def test_a_captured_rerank_follows_the_list(amd, edge_codes):
    codes, scales, lens, mixed = edge_codes
    idx, _ = _index_of_codes(amd, codes, scales, lens, mixed, 50)
    g = torch.Generator().manual_seed(68)
    q = _packed(amd, [_unit(g, k) for k in (32, 5, 17, 64, 1)])
    rng = np.random.default_rng(69)
    first, second = (torch.from_numpy(50 + rng.integers(-1, len(lens) + 1, (5, 9))).to(DEV) for _ in range(2))
    cand = first.clone()
    out = torch.empty((5, 9), dtype=torch.float32, device=DEV)
    amd.fp4_wide_rerank_scores(q, idx, cand, out=out)                # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, ids = amd.fp4_wide_rerank_scores(q, idx, cand, out=out)
    for lst in (second, first):
        cand.copy_(lst)                                               # in place: the graph holds the tensor's address
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_s, want_i = amd.fp4_wide_rerank_scores(q, idx, lst)
        np.testing.assert_array_equal(_bits(out), _bits(want_s))
        np.testing.assert_array_equal(ids.cpu().numpy(), want_i.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------- the route
K, ID_BASE = 5, 100


@pytest.fixture(scope="module")
def route(amd):
    g = torch.Generator().manual_seed(70)
    lens = torch.randint(1, 101, (40,), generator=g).tolist()
    lens[3], lens[17] = 1, 100
    pages = [_unit(g, k) for k in lens]
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=ID_BASE)
    q = _packed(amd, [_unit(g, k) for k in (5, 16, 17, 32, 33)])
    all_ids = torch.arange(ID_BASE, ID_BASE + 40, dtype=torch.int64, device=DEV).expand(5, 40)
    return corpus, amd.Fp4WideIndex.build(corpus), q, pages, all_ids


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x.dtype == torch.float32:
            np.testing.assert_array_equal(_bits(x), _bits(y))
        else:
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())


def test_refining_to_the_whole_list_changes_nothing(amd, route):
    corpus, idx, q, pages, _ = route
    pooled = amd.pack_passages([p.float().mean(0, keepdim=True).to(torch.bfloat16) for p in pages], DEV, batch_size=None, id_base=ID_BASE)
    r = amd.ShardedRetriever(corpus)
    for m1 in (1, 7, 20, 39):
        _same(r.search(q, K, prefilter=pooled, n_candidates=m1, refine=idx, n_refine=m1),
              r.search(q, K, prefilter=pooled, n_candidates=m1))


def test_refining_every_page_is_the_fp4_first_stage(amd, route):
    corpus, idx, q, _, all_ids = route
    r = amd.ShardedRetriever(corpus)
    for m in (1, 7, 20, 39):
        _same(r.search(q, K, candidates=all_ids, refine=idx, n_refine=m), r.search(q, K, prefilter=idx, n_candidates=m))


def test_refine_with_a_filter_and_with_groups(amd, route):
    corpus, idx, q, _, all_ids = route
    g = torch.Generator().manual_seed(71)
    allowed = torch.rand(40, generator=g) < 0.6
    labels = torch.randint(0, 9, (40,), generator=g)
    r = amd.ShardedRetriever(corpus)
    fine = amd.fp4_wide_scores(q, idx)
    flt = amd.PageFilter.from_mask(allowed.to(DEV), ID_BASE)
    groups = amd.PageGroups.from_labels(labels.to(DEV), ID_BASE)
    for m in (1, 7, 20):
        # filter=: the refined list is the FP4 top m of the allowed pages; the exact rerank orders it
        masked = torch.where(allowed.to(DEV)[None, :], fine, torch.full_like(fine, float("-inf")))
        ms, mi = amd.topk(masked, m, ID_BASE)
        mi = torch.where(ms == float("-inf"), torch.full_like(mi, -1), mi)
        ws, wi = amd.rerank(q, corpus, mi, K)
        wi = torch.where(ws == float("-inf"), torch.full_like(wi, -1), wi)
        _same(r.search(q, K, candidates=all_ids, refine=idx, n_refine=m, filter=flt), (ws, wi))
        # group_by=: the refined list is the FP4 top m PAGES; every document is scored by its best exact page among them
        _, ri = amd.topk(fine, m, ID_BASE)
        es, ei = amd.rerank(q, corpus, ri).cpu().numpy(), ri.cpu().numpy()
        lab = labels.numpy()
        want_s = np.full((5, K), -np.inf, dtype=np.float32)
        want_g, want_p = np.full((5, K), -1, dtype=np.int64), np.full((5, K), -1, dtype=np.int64)
        for row in range(5):
            best = {}
            for s, p in zip(es[row], ei[row]):
                d = int(lab[p - ID_BASE])
                if d not in best or (s, -p) > (best[d][0], -best[d][1]):
                    best[d] = (s, p)
            for col, (d, (s, p)) in enumerate(sorted(best.items(), key=lambda kv: (-kv[1][0], kv[0]))[:K]):
                want_s[row, col], want_g[row, col], want_p[row, col] = s, d, p
        gs, gg, gp = r.search(q, K, candidates=all_ids, refine=idx, n_refine=m, group_by=groups)
        np.testing.assert_array_equal(_bits(gs), want_s.view(np.int32))
        np.testing.assert_array_equal(gg.cpu().numpy(), want_g)
        np.testing.assert_array_equal(gp.cpu().numpy(), want_p)


# ------------------------------------------------------------------------------------------------------------------------ live
def test_a_live_wide_shard_never_refines_a_deleted_page(amd, route):
    corpus, _, q, pages, _ = route
    live = amd.LiveCorpus.from_packed(corpus, 64, 4)
    assert isinstance(live.fp4_index(), amd.Fp4WideIndex)
    dead = list(range(ID_BASE + 1, ID_BASE + 40, 3))
    live.delete(dead)
    alive = [c for c in range(40) if c + ID_BASE not in dead]
    fresh = amd.pack_passages([pages[c] for c in alive], DEV, batch_size=None)
    fresh_ids = torch.arange(len(alive), dtype=torch.int64, device=DEV).expand(5, len(alive))
    slot = torch.tensor(alive, dtype=torch.int64, device=DEV) + ID_BASE
    all_ids = torch.arange(ID_BASE, ID_BASE + 40, dtype=torch.int64, device=DEV).expand(5, 40)
    r = amd.ShardedRetriever(fresh)
    fresh_idx = amd.Fp4WideIndex.build(fresh)
    for compacted in (False, True):
        if compacted:
            live.compact()
        for m in (1, 7, len(alive) - 1):
            s, i = live.search(q, K, candidates=all_ids, refine=live.fp4_index(), n_refine=m)
            assert not np.isin(i.cpu().numpy(), dead).any()
            ws, wi = r.search(q, K, candidates=fresh_ids, refine=fresh_idx, n_refine=m)
            wi = torch.where(wi >= 0, slot[wi.clamp(min=0)], wi)
            _same((s, i), (ws, wi))
    live.check()
