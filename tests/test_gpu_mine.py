"""Hard-negative mining and the page gather on the MI355X (colpali_amd.mine_hard_negatives / gather_pages, msim_mine_bounds,
msim_mine_mask, msim_gather_pages).

Every check is exact: the scores are those of the unchanged full scan (fetched to the host and fed to the numpy restatement in
tests/mine_truth.py), the selection is a total order, the gather is a copy.  The shapes are the edges of the kernels: rows that are
no multiple of the 4-column lane group, matrices whose rows are not 16-byte aligned, pages around the 16-row piece count, ids off the
shard.
"""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import live_truth as lt
from tests import mine_truth as mt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EINVAL = -1
FAKE = 1 << 20
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _ragged(g, n, lo=1, hi=41, dim=128, dtype=torch.bfloat16):
    return [_unit(g, int(k), dim, dtype) for k in torch.randint(lo, hi, (n,), generator=g)]


def _packed(amd, q_blocks):
    return amd.pack_queries(list(q_blocks), DEV, layout="flat", compact=False)


def _check(amd, q, corpus, positives, n_neg, **kw):
    """mine_hard_negatives against the truth over the scan's own scores; returns (scores np, neg_scores, neg_ids)."""
    s = amd.maxsim_scores(q, corpus).cpu().numpy()
    got_s, got_i = amd.mine_hard_negatives(q, corpus, positives, n_neg, **kw)
    assert got_s.shape == (len(q), n_neg) and got_s.dtype == torch.float32 and got_i.dtype == torch.int64
    host = tuple(p.cpu().numpy() for p in positives) if isinstance(positives, tuple) else positives.cpu().numpy()
    alive = kw.get("alive")
    want_s, want_i = mt.mine(s, mt.as_lists(host, len(q)), n_neg, corpus.id_base, kw.get("max_ratio"), kw.get("skip_top", 0),
                             None if alive is None else alive.cpu().numpy())
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32))       # the scan's own bits
    return s, got_s.cpu().numpy(), got_i.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- exact selection
@pytest.mark.parametrize("dtype,dim,n_q,n", [(torch.bfloat16, 128, 7, 301), (torch.float16, 128, 5, 67), (torch.bfloat16, 320, 4, 45)])
def test_selection_is_exact(amd, dtype, dim, n_q, n):
    g = torch.Generator().manual_seed(1)
    corpus = amd.pack_passages(_ragged(g, n, dim=dim, dtype=dtype), DEV, batch_size=None)
    q = _packed(amd, [_unit(g, int(k), dim, dtype) for k in torch.randint(1, 33, (n_q,), generator=g)])
    pos = torch.randint(0, n, (n_q, 3), generator=g).to(DEV)
    _check(amd, q, corpus, pos, 8)
    _check(amd, q, corpus, pos, 8, max_ratio=0.95, skip_top=5)
    s = amd.maxsim_scores(q, corpus)
    before = s.clone()
    a_s, a_i = amd.mine_hard_negatives(None, corpus, pos, 8, max_ratio=0.95, scores=s)       # the caller's matrix: copied, not touched
    b_s, b_i = amd.mine_hard_negatives(q, corpus, pos, 8, max_ratio=0.95)
    assert torch.equal(a_i, b_i) and torch.equal(a_s, b_s) and torch.equal(_as_int(s), _as_int(before))


def _as_int(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ the mask touches nothing else
def _mask_case(amd, n, ld, seed, max_ratio, with_alive, n_q=5, shift=0):
    r = np.random.default_rng(seed)
    s = (r.standard_normal((n_q, n)) * 4 + 6).astype(np.float32)
    s[r.random((n_q, n)) < 0.1] = -np.inf
    s[0, :] = np.float32(7.25)                                           # a constant row: every column on one side of the bound
    alive = (r.random(n) > 0.3).astype(np.uint8) if with_alive else None
    pos_list = [[int(x) for x in r.integers(-2, n + 2, size=r.integers(0, 4))] for _ in range(n_q)]
    pos_list[1] = []
    ids = torch.tensor([i for row in pos_list for i in row], dtype=torch.int64, device=DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(row) for row in pos_list])]), dtype=torch.int32, device=DEV)
    buf = torch.full((n_q * ld + shift,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[shift:].view(n_q, ld)[:, :n]
    view.copy_(torch.from_numpy(s))
    alive_d = None if alive is None else torch.from_numpy(alive).to(DEV)
    bounds = None
    if max_ratio is not None:
        bounds = amd.mine.mine_bounds(view, (ids, off), 0, alive=alive_d)
        np.testing.assert_array_equal(_bits(bounds), mt.bounds(s, pos_list, 0, alive).view(np.int32))
        local = amd.mine.mine_bounds(view, (ids, off), 0, alive=alive_d, local=True)
        np.testing.assert_array_equal(_bits(local), mt.bounds(s, pos_list, 0, alive, none=-np.inf).view(np.int32))
    out = amd.mine.mine_mask(view, (ids, off), 0, bounds, max_ratio, alive_d)
    assert out.data_ptr() == view.data_ptr()
    want = np.full((n_q, ld), SENTINEL, dtype=np.float32)
    want[:, :n] = mt.masked(s, pos_list, 0, max_ratio, alive)
    np.testing.assert_array_equal(_bits(buf[shift:].view(n_q, ld)), want.view(np.int32), err_msg=f"n={n} ld={ld}")
    assert (buf[:shift] == SENTINEL).all()
    ok = mt.eligible(s, pos_list, 0, max_ratio, alive)
    return ok


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_mask_writes_minus_inf_into_ineligible_columns_and_nothing_else(amd, n):
    ld = (n + 4 + 3) // 4 * 4                                            # rows 16-byte aligned: the vector path, with slack behind n
    seen = np.zeros((2,), dtype=np.int64)
    for seed, (ratio, with_alive) in enumerate([(0.95, True), (0.95, False), (None, True), (None, False), (1.5, True)]):
        ok = _mask_case(amd, n, ld, 10 * n + seed, ratio, with_alive)
        seen += [ok.sum(), (~ok).sum()]
    assert seen.min() > 0                                                # both kinds of column occurred


@pytest.mark.parametrize("n", [5, 64, 257])
def test_mask_on_rows_that_are_only_4_byte_aligned(amd, n):
    ld = n + 3 if (n + 3) % 2 else n + 4                                 # odd: every row starts at another alignment
    assert ld % 2 == 1
    _mask_case(amd, n, ld, n, 0.95, True)
    _mask_case(amd, n, ld, n + 1, None, True)
    _mask_case(amd, n, (n + 7) // 4 * 4, n + 2, 0.95, True, shift=1)     # ld a multiple of 4, the matrix itself 4 bytes off


# ------------------------------------------------------------------------------------------------------------------------ ties
def test_ties_are_cut_in_id_order_at_both_window_edges(amd):
    g = torch.Generator().manual_seed(2)
    qs = [_unit(g, 8), _unit(g, 12)]
    docs = _ragged(g, 40)
    twin = torch.cat([qs[0], _unit(g, 3)])                               # holds query 0's own tokens: the best page by far
    copies = [3, 11, 12, 20, 33]
    for c in copies:
        docs[c] = twin.clone()
    corpus = amd.pack_passages(docs, DEV, batch_size=None)
    q = _packed(amd, qs)
    pos = torch.tensor([-1, 5], device=DEV)
    s, _, _ = _check(amd, q, corpus, pos, 3)
    assert len({s[0, c].tobytes() for c in copies}) == 1 and (np.delete(s[0], copies) < s[0, 3]).all()      # five exact ties on top
    for skip, n_neg, head in ((0, 3, [3, 11, 12]), (2, 2, [12, 20]), (1, 4, [11, 12, 20, 33]), (4, 3, [33]), (3, 1, [20])):
        _, _, ids = _check(amd, q, corpus, pos, n_neg, skip_top=skip)
        assert ids[0, :len(head)].tolist() == head, (skip, n_neg)


# ------------------------------------------------------------------------------------------------------------- positives forms
def test_the_three_forms_of_positives_agree(amd):
    g = torch.Generator().manual_seed(3)
    n, base = 50, 1000
    corpus = amd.pack_passages(_ragged(g, n), DEV, batch_size=None, id_base=base)
    q = _packed(amd, [_unit(g, k) for k in (4, 9, 32, 1, 17, 8)])
    one = torch.tensor([1003, -1, 1049, 999, 1050, 1000], device=DEV)    # below id_base and at id_base + n: ignored
    lists = [[1003, 1003, 1007], [], [-1, 1049], [999, 1050, -5], [1000, 1001, 1002, 1001], [1025]]
    P = max(len(x) for x in lists)
    padded = torch.tensor([x + [-1] * (P - len(x)) for x in lists], device=DEV)
    csr = (torch.tensor([i for x in lists for i in x], dtype=torch.int64, device=DEV),
           torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int32, device=DEV))
    one_csr = (one.clone(), torch.arange(7, dtype=torch.int32, device=DEV))
    for kw in (dict(), dict(max_ratio=0.95), dict(max_ratio=0.95, skip_top=2)):
        _, a_s, a_i = _check(amd, q, corpus, one, 6, **kw)
        for form in (one[:, None].contiguous(), one_csr):
            _, b_s, b_i = _check(amd, q, corpus, form, 6, **kw)
            np.testing.assert_array_equal(a_i, b_i)
            np.testing.assert_array_equal(a_s.view(np.int32), b_s.view(np.int32))
        _, c_s, c_i = _check(amd, q, corpus, padded, 6, **kw)
        _, d_s, d_i = _check(amd, q, corpus, csr, 6, **kw)
        np.testing.assert_array_equal(c_i, d_i)
        np.testing.assert_array_equal(c_s.view(np.int32), d_s.view(np.int32))
        assert c_i.min() >= base and c_i.max() < base + n
        for row, mine in zip(lists, c_i):
            assert not set(row) & set(mine.tolist())
    host = amd.mine_hard_negatives(q, corpus, padded.cpu(), 6)[1]        # host positives are uploaded
    assert torch.equal(host, amd.mine_hard_negatives(q, corpus, padded, 6)[1])


# ------------------------------------------------------------------------------------------------------------------- max_ratio
def planted_ratio_case(g):
    """(queries, pages): query 0's positive is page 2 (the query's own tokens: score ~8); page 5 is a near-duplicate scoring
    ~7.86 (above 0.95 x 8 = 7.6), page 9 one scoring ~6.5 (below); query 1 has no positive."""
    qs = [_unit(g, 8), _unit(g, 8)]
    docs = _ragged(g, 24, lo=3, hi=20)
    docs[2] = torch.cat([qs[0], _unit(g, 4)])
    near = qs[0].float()
    near[7] = torch.nn.functional.normalize(near[7] + 0.6 * _unit(g, 1)[0].float(), dim=-1)
    docs[5] = torch.cat([near.to(torch.bfloat16), _unit(g, 2)])
    docs[9] = torch.cat([qs[0][:6], _unit(g, 5)])
    return qs, docs


def check_planted_scores(s):
    """the planted scores sit far more than an fp32 ulp (~5e-7 at 8) from the bound"""
    thresh = np.float32(0.95) * s[0, 2]
    assert s[0, 2] == s[0].max() and s[0, 5] > thresh + 0.1 and s[0, 9] < thresh - 0.1 and s[0, 9] > np.delete(s[0], [2, 5, 9]).max()


def test_max_ratio_drops_the_near_duplicate_above_the_bound_only(amd):
    qs, docs = planted_ratio_case(torch.Generator().manual_seed(4))
    corpus = amd.pack_passages(docs, DEV, batch_size=None)
    q = _packed(amd, qs)
    pos = torch.tensor([2, -1], device=DEV)
    s, _, plain = _check(amd, q, corpus, pos, 4)
    check_planted_scores(s)
    assert plain[0, :2].tolist() == [5, 9]
    _, _, ids = _check(amd, q, corpus, pos, 4, max_ratio=0.95)
    assert ids[0, 0] == 9 and 5 not in ids[0] and 2 not in ids[0]        # the first is dropped, the second kept
    assert ids[1].tolist() == plain[1].tolist()                          # no positive: nothing is dropped
    _, _, far = _check(amd, q, corpus, pos, 4, max_ratio=0.5)            # 0.5 x 8: both near-duplicates go
    assert 5 not in far[0] and 9 not in far[0]


def sign_case():
    """every similarity negative (tests/helpers.py: far_side_case, the inputs of tests/test_gpu_sign_edges.py)"""
    g = torch.Generator().manual_seed(5)
    d_lens = torch.randint(1, 41, (60,), generator=g).tolist()
    return helpers.far_side_case(5, [8, 8, 5], d_lens, 128, torch.bfloat16)[:2]


def check_sign_scores(s, pos_col):
    """-> per query (kept although BETTER than the positive, kept in all, dropped): with pos < 0 the bound 0.95 x pos lies ABOVE pos"""
    assert (s < 0).all()
    out = []
    for q, c in enumerate(pos_col):
        pos = s[q, c]
        thresh = np.float32(0.95) * pos
        assert thresh > pos
        others = np.delete(s[q], c)
        out.append((int(((others > pos) & ~(others > thresh)).sum()), int((~(others > thresh)).sum()), int((others > thresh).sum())))
    return out


def sign_positives(s):
    """the 8th worst page of every query as its positive: pages on either side of it, and of the bound"""
    return np.argsort(s, axis=1, kind="stable")[:, 7]


def test_max_ratio_sign_quirk_on_all_negative_similarities(amd):
    qs, docs = sign_case()
    corpus = amd.pack_passages(docs, DEV, batch_size=None)
    q = _packed(amd, qs)
    s = amd.maxsim_scores(q, corpus).cpu().numpy()
    pos_col = sign_positives(s)
    counts = check_sign_scores(s, pos_col)
    assert all(better > 0 and dropped > 0 for better, _, dropped in counts), counts
    pos = torch.from_numpy(pos_col).to(DEV)
    _, got_s, got_i = _check(amd, q, corpus, pos, len(docs), max_ratio=0.95)
    for row, (better, kept, dropped) in enumerate(counts):               # literally: pages BETTER than the positive are mined, up
        p = s[row, pos_col[row]]                                         # to 0.95 x pos (above pos); the ones beyond it are dropped
        assert (got_i[row] >= 0).sum() == kept
        assert (got_s[row, :kept] <= np.float32(0.95) * p).all() and (got_s[row, :kept] > p).sum() == better
        assert pos_col[row] not in got_i[row]


# ------------------------------------------------------------------------------------------------------------------ starvation
def test_starved_rows_end_in_minus_inf_and_minus_one(amd):
    g = torch.Generator().manual_seed(6)
    docs = _ragged(g, 12)
    docs[4] = docs[4][:0]                                                # pages of 0 rows: score -inf, never mined
    docs[7] = docs[7][:0]
    corpus = amd.pack_passages(docs, DEV, batch_size=None)
    q = _packed(amd, [_unit(g, k) for k in (5, 8, 3)])
    pos = torch.tensor([[0, 1, -1], [-1, -1, -1], [11, 11, 2]], device=DEV)
    _, got_s, got_i = _check(amd, q, corpus, pos, 15)
    assert [(r >= 0).sum() for r in got_i] == [8, 10, 8] and not np.isin(got_i, [4, 7]).any()
    assert all((r[(r >= 0).sum():] == -1).all() for r in got_i) and np.isneginf(got_s[got_i < 0]).all()
    _check(amd, q, corpus, pos, 4, skip_top=7)                           # the window runs off the end of the eligible list
    everything = torch.arange(12, device=DEV).repeat(3, 1)
    _, all_s, all_i = _check(amd, q, corpus, everything, 5, max_ratio=0.95)
    assert (all_i == -1).all() and np.isneginf(all_s).all()              # every page a positive


# ----------------------------------------------------------------------------------------------------------------------- alive
def test_live_corpus_mines_only_live_slots(amd):
    g = torch.Generator().manual_seed(7)
    pages = _ragged(g, 40)
    pages[9] = pages[3].clone()
    qs = [_unit(g, k) for k in (8, 20, 5, 32)]
    q = _packed(amd, qs)
    live = amd.LiveCorpus.from_packed(amd.pack_passages(pages[:30], DEV, batch_size=None, id_base=100), spare_rows=400, spare_docs=20)
    live.add(pages[30:])
    deleted = [2, 3, 17, 29, 31, 38]
    live.delete([100 + d for d in deleted])
    pos = torch.tensor([[103, 105], [117, -1], [-1, -1], [139, 100]], device=DEV)    # deleted positives among them
    surv = [c for c in range(40) if c not in deleted]
    fresh = amd.pack_passages([pages[c] for c in surv], DEV, batch_size=None)
    where = {100 + c: p for p, c in enumerate(surv)}
    fresh_pos = torch.tensor([[where.get(i, -1) for i in row] for row in pos.tolist()], device=DEV)
    for kw in (dict(), dict(max_ratio=0.95, skip_top=1)):
        want_s, want_i = amd.mine_hard_negatives(q, fresh, fresh_pos, 36, **kw)
        want_i = lt.expected_ids(want_i.cpu().numpy(), surv, id_base=100)
        for step in ("deleted", "compacted"):
            got_s, got_i = live.mine(q, pos, 36, **kw)
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=step)
            np.testing.assert_array_equal(_bits(got_s), _bits(want_s), err_msg=step)
            assert not np.isin(got_i.cpu().numpy(), [100 + d for d in deleted]).any()
            live.compact()
        live.check()
    assert (want_i[:, -1] == -1).all()                                   # 34 live pages, 36 asked for
    direct = amd.mine_hard_negatives(q, live.view(), pos, 36, alive=live.alive[:len(live)])
    assert torch.equal(direct[1], live.mine(q, pos, 36)[1])


# ---------------------------------------------------------------------------------------------------------------- gather_pages
def _torch_gather(corpus, ids, pad):
    """the torch loop: corpus.blob[off[c]:off[c + 1]] into a zeroed box, on the host"""
    blob, off = corpus.blob.cpu(), corpus.offsets.cpu().tolist()
    ids = ids.cpu()
    box = torch.zeros(tuple(ids.shape) + (pad, blob.shape[1]), dtype=blob.dtype)
    lens = torch.zeros(tuple(ids.shape), dtype=torch.int32)
    flat_box, flat_lens = box.view(ids.numel(), pad, blob.shape[1]), lens.view(-1)
    for j, i in enumerate(ids.reshape(-1).tolist()):
        c = i - corpus.id_base
        if i >= 0 and 0 <= c < len(corpus):
            m = min(off[c + 1] - off[c], pad)
            flat_box[j, :m] = blob[off[c]:off[c] + m]
            flat_lens[j] = m
    return box, lens


def _same_bytes(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.cpu().reshape(-1).view(torch.uint8), b.cpu().reshape(-1).view(torch.uint8))    # reshape: a 0-dim loss too


GATHER_LENS = (1, 15, 16, 17, 40, 0, 3, 33, 40, 2)


@pytest.mark.parametrize("dtype,dim", [(torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 320), (torch.float16, 320),
                                       (torch.float32, 128)])
def test_gather_pages_equals_a_torch_loop(amd, dtype, dim):
    g = torch.Generator().manual_seed(8)
    base = 70
    corpus = amd.pack_passages([_unit(g, n, dim, dtype) for n in GATHER_LENS], DEV, batch_size=None, id_base=base)
    n = len(GATHER_LENS)
    for shape in ((5,), (3, 4), (2, 3, 2)):
        ids = torch.randint(base, base + n, shape, generator=g)
        ids.view(-1)[0] = -1
        ids.view(-1)[1] = base + n                                       # off the shard, either side
        ids.view(-1)[2] = base - 1
        ids.view(-1)[3] = base + 4                                       # a page of L_pad rows
        ids.view(-1)[4] = base + 5                                       # a page of 0 rows
        for pad in (None, 64, 16, 0):
            L = 40 if pad is None else pad
            want_box, want_len = _torch_gather(corpus, ids, L)
            sentinel = torch.full(tuple(shape) + (L, dim), 7.0, dtype=dtype, device=DEV)
            box, lens = amd.gather_pages(corpus, ids.to(DEV), pad, out=sentinel)
            assert box.data_ptr() == sentinel.data_ptr() and box.shape == tuple(shape) + (L, dim) and lens.dtype == torch.int32
            assert _same_bytes(box, want_box) and torch.equal(lens.cpu(), want_len), (shape, pad)       # every byte was written
            box2, lens2 = amd.gather_pages(corpus, ids.to(DEV), pad)
            assert _same_bytes(box2, want_box) and torch.equal(lens2.cpu(), want_len) and box2.dtype == dtype
            if L >= 40:
                host_box, host_len = amd.gather_pages(corpus, ids, pad)                                 # host ids: checked, uploaded
                assert _same_bytes(host_box, want_box) and torch.equal(host_len.cpu(), want_len)
            elif L:
                with pytest.raises(ValueError, match="pad_to"):          # the host path raises where the device path truncates
                    amd.gather_pages(corpus, ids, pad)
        assert want_len.max() == 0 and (lens == 0).all()                 # pad_to = 0: lengths only
    rows = torch.tensor([base + c for c in range(n)])
    box, lens = amd.gather_pages(corpus, rows.to(DEV), 16)
    assert lens.cpu().tolist() == [min(k, 16) for k in GATHER_LENS]      # the truncated count


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_mine_gather_and_the_explicit_negative_loss(amd):
    g = torch.Generator().manual_seed(9)
    pages = _ragged(g, 64, lo=4, hi=30)
    q_host = torch.stack([_unit(g, 12) for _ in range(8)])
    pos = torch.randperm(64, generator=g)[:8]
    for i, c in enumerate(pos.tolist()):                                 # a real positive: the page answers its query (score ~12), so
        pages[c] = torch.cat([q_host[i], pages[c]])                      # 0.95 x pos lies far above every other page
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    pos = pos.to(DEV)
    neg_s, neg_i = amd.mine_hard_negatives(q_host.to(DEV), corpus, pos, 4, max_ratio=0.95)
    assert (neg_i >= 0).all() and not (neg_i == pos[:, None]).any()
    box, lens = amd.gather_pages(corpus, neg_i)
    docs, _ = amd.gather_pages(corpus, pos)
    want_box, want_lens = _torch_gather(corpus, neg_i, int(corpus.lengths.max()))
    assert _same_bytes(box, want_box) and torch.equal(lens.cpu(), want_lens) and box.shape[:2] == (8, 4)
    results = []
    for neg in (box, want_box.to(DEV)):
        qd = q_host.to(DEV).requires_grad_(True)
        dd = docs.clone().requires_grad_(True)
        nd = neg.clone().requires_grad_(True)
        loss = amd.ColbertNegativeCELoss()(qd, dd, nd)
        loss.backward()
        results.append((loss.detach(), qd.grad, dd.grad, nd.grad))
    assert torch.isfinite(results[0][0]) and float(results[0][3].abs().max()) > 0
    for a, b in zip(*results):
        assert _same_bytes(a, b)


# --------------------------------------------------------------------------------------------------------------------- capture
def test_reruns_and_graph_replays_are_bit_identical(amd):
    g = torch.Generator().manual_seed(10)
    corpus = amd.pack_passages(_ragged(g, 90), DEV, batch_size=None, id_base=10)
    q = _packed(amd, [_unit(g, k) for k in (32, 5, 17, 1)])
    pos = torch.tensor([[12, 40], [-1, 99], [10, 10], [55, 200]], device=DEV)
    alive = torch.ones(90, dtype=torch.uint8, device=DEV)
    alive[[6, 44]] = 0

    def run():
        s, i = amd.mine_hard_negatives(q, corpus, pos, 5, max_ratio=0.95, skip_top=1, alive=alive)
        box, lens = amd.gather_pages(corpus, i, 24)
        return s, i, box, lens

    first = [t.clone() for t in run()]
    for t, u in zip(first, run()):
        assert _same_bytes(t, u)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for t, u in zip(first, outs):
            assert _same_bytes(t, u)
    assert (first[1] >= 10).all() and not np.isin(first[1].cpu().numpy(), [16, 54]).any()


# ----------------------------------------------------------------------------------------------------------------- error paths
def test_error_paths(amd):
    g = torch.Generator().manual_seed(11)
    pages = _ragged(g, 6)
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    host_corpus = amd.pack_passages(pages, torch.device("cpu"), batch_size=None)
    q = torch.stack([_unit(g, 4) for _ in range(3)])
    pos = torch.tensor([0, 1, -1], device=DEV)
    with pytest.raises(RuntimeError, match="MI355X"):                    # the GPU-only error of rerank and align
        amd.mine_hard_negatives(q.to(DEV), host_corpus, pos, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        amd.gather_pages(host_corpus, pos)
    with pytest.raises(ValueError, match="different devices"):
        amd.mine_hard_negatives(q, corpus, pos, 2)                       # queries on the host
    scores = amd.maxsim_scores(q.to(DEV), corpus)
    with pytest.raises(ValueError, match="different devices"):
        amd.mine_hard_negatives(None, corpus, pos, 2, scores=scores.cpu())
    with pytest.raises(ValueError, match="different devices"):
        amd.mine_hard_negatives(q.to(DEV), corpus, pos, 2, alive=torch.ones(6, dtype=torch.uint8))
    with pytest.raises(ValueError):
        amd.mine_hard_negatives(None, corpus, pos, 2, scores=scores[:, :5])
    with pytest.raises(ValueError):
        amd.gather_pages(corpus, pos.to(torch.int32))
    with pytest.raises(ValueError):
        amd.gather_pages(corpus, pos, out=torch.empty((3, 7, 128), dtype=torch.bfloat16, device=DEV))
    L = amd._lib.lib()
    for args in ((None, 10, 4, 10, FAKE, FAKE, 5), (FAKE + 2, 10, 4, 10, FAKE, FAKE, 5), (FAKE, 9, 4, 10, FAKE, FAKE, 5),
                 (FAKE, 10, 4, 10, FAKE, None, 5), (FAKE, 10, 4, 10, FAKE + 4, FAKE, 5)):
        scores_p, ld, n_q, n, ids_p, off_p, nnz = args
        assert L.msim_mine_bounds(scores_p, ld, n_q, n, ids_p, off_p, nnz, 0, None, 0, FAKE, None) == EINVAL, args
        assert L.msim_mine_mask(scores_p, ld, n_q, n, FAKE, 0.95, None, ids_p, off_p, nnz, 0, None) == EINVAL, args
    assert L.msim_mine_bounds(FAKE, 10, 4, 10, FAKE, FAKE, 5, 0, None, 0, None, None) == EINVAL
    for kw in (dict(rows=None), dict(out=FAKE + 8), dict(ids=None), dict(row_bytes=24), dict(lens=FAKE + 2)):
        a = dict(rows=FAKE, row_bytes=256, ids=FAKE, out=FAKE, lens=FAKE)
        a.update(kw)
        assert L.msim_gather_pages(a["rows"], a["row_bytes"], 100, FAKE, 10, 0, a["ids"], 6, 8, a["out"], a["lens"], None) == EINVAL, kw
