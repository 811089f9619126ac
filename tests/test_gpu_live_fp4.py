"""The live FP4 index on the MI355X (LiveCorpus.fp4_index, msim_f4_live_compact; widths 128 and 320).

The contract, checked bit for bit: after any history of add / delete / compact the used prefix of `live.fp4_index()` is
`Fp4Index.build(live.view())` / `Fp4WideIndex.build(live.view())`, and with S the surviving pages in slot order and
F = pack_passages(S, batch_size=None), `live.search(prefilter=live.fp4_index())` returns the scores of
`ShardedRetriever(F).search(prefilter=<index>.build(F))` and its ids mapped back to slots (tests/live_truth.py).  The yardsticks
are the builds over a frozen corpus and numpy; nothing here has a tolerance.
"""
import numpy as np
import pytest
import torch

from tests import live_truth as lt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _rows(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _index_cls(amd, dim):
    return amd.Fp4WideIndex if dim == 320 else amd.Fp4Index


def _same(got, want, surv, id_base=0):
    """a live result against the same search over the packed survivors: score bits, and positions mapped back to slot ids"""
    assert len(got) == len(want)
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
    if len(got) == 3:                                                     # group_by: (scores, document ids, best pages)
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
    np.testing.assert_array_equal(got[-1].cpu().numpy(), lt.expected_ids(want[-1].cpu().numpy(), surv, id_base))


def _same_index(live, idx, want):
    """the used prefix of a live index against a build over `live.view()`"""
    r, n = live.rows_used, len(live)
    assert type(idx) is type(want) and len(idx) == n and idx.id_base == live.id_base
    assert torch.equal(idx.codes[:r], want.codes[:r]) and torch.equal(idx.scales[:r], want.scales[:r])
    assert torch.equal(idx.offsets, want.offsets) and idx.clamp0 is None and torch.equal(idx.lengths, want.lengths)


# ---------------------------------------------------------------------------------------------------------------- the raw ABI
def _raw_compact(L, codes, scales, off, alive, crb, bounce_rows):
    """two calls of msim_f4_live_compact over host arrays (codes uint8 [bound + 5, crb], scales uint8 [bound + 5]) against numpy"""
    bound, n = int(off[-1]), len(alive)
    d_codes = torch.from_numpy(codes).to(DEV)
    d_scales = torch.zeros(scales.size + 3, dtype=torch.uint8, device=DEV)[3:]            # the scale bytes need no alignment
    d_scales.copy_(torch.from_numpy(scales))
    d_off, d_alive = torch.from_numpy(off.astype(np.int32)).to(DEV), torch.tensor(alive, dtype=torch.uint8, device=DEV)
    used = torch.zeros(1, dtype=torch.int64, device=DEV)
    bounce = torch.zeros(bounce_rows * (crb + 1), dtype=torch.uint8, device=DEV)
    ws = torch.zeros(L.msim_f4_live_compact_workspace_bytes(n, bounce.numel()), dtype=torch.uint8, device=DEV)
    new_off = lt.compact_offsets(off, alive)
    want_codes, want_scales = lt.compact_rows(codes, off, alive), lt.compact_rows(scales, off, alive)
    for _ in range(2):                                                                   # the second call changes nothing
        rc = L.msim_f4_live_compact(d_codes.data_ptr(), crb, d_scales.data_ptr(), bound, d_off.data_ptr(), d_alive.data_ptr(), n,
                                    used.data_ptr(), ws.data_ptr(), bounce.data_ptr(), bounce.numel(), None)
        assert rc == 0, L.msim_last_error()
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32)[0]) == 0 and int(used[0]) == new_off[-1]
        np.testing.assert_array_equal(d_off.cpu().numpy(), new_off)
        got_codes, got_scales = d_codes.cpu().numpy(), d_scales.cpu().numpy()
        np.testing.assert_array_equal(got_codes[:new_off[-1]], want_codes[:new_off[-1]])
        np.testing.assert_array_equal(got_scales[:new_off[-1]], want_scales[:new_off[-1]])
        np.testing.assert_array_equal(got_codes[bound:], codes[bound:])                  # nothing past the bound
        np.testing.assert_array_equal(got_scales[bound:], scales[bound:])


def _random_arrays(g, rows, crb):
    return (torch.randint(0, 256, (rows, crb), generator=g, dtype=torch.uint8).numpy(),
            torch.randint(0, 256, (rows,), generator=g, dtype=torch.uint8).numpy())


@pytest.mark.parametrize("crb", [64, 160])
def test_raw_abi_small_chunks_and_a_page_across_chunks(amd, crb):
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(5 + crb)
    lens = [3, 50, 1, 1, 17, 4, 33, 2, 9, 1]
    alive = [1, 0, 1, 0, 0, 1, 1, 0, 1, 1]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for bounce_rows in (1, 4):                                                           # every chunk boundary falls inside a page
        codes, scales = _random_arrays(g, int(off[-1]) + 5, crb)
        _raw_compact(L, codes, scales, off, alive, crb, bounce_rows)


@pytest.mark.parametrize("crb", [64, 160])
def test_raw_abi_a_chunk_of_several_workgroups(amd, crb):
    """about 3000 rows through a bounce buffer of 1500: a chunk spans several workgroups of the code mover (256 rows of 64 bytes,
    102 of 160) and two of the scale mover (1024 rows), and pages cross their boundaries"""
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(9)
    lens = [40, 700, 1, 310, 655, 2, 480, 97, 1, 520, 230, 64]
    alive = [1, 1, 0, 1, 1, 0, 1, 0, 1, 0, 1, 1]                                         # one third dead, the first dead page not first
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert 3000 <= off[-1] <= 3200 and sum(1 for a in alive if not a) * 3 == len(alive)
    codes, scales = _random_arrays(g, int(off[-1]) + 5, crb)
    _raw_compact(L, codes, scales, off, alive, crb, 1500)


def test_raw_abi_broken_offsets_set_the_status_word_and_move_nothing(amd):
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(6)
    codes, scales = (torch.from_numpy(a).to(DEV) for a in _random_arrays(g, 14, 160))
    keep = codes.clone(), scales.clone()
    bad = torch.tensor([0, 5, 3, 9], dtype=torch.int32, device=DEV)                      # not monotonic
    alive = torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    used = torch.zeros(1, dtype=torch.int64, device=DEV)
    bounce = torch.zeros(4 * 161, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(L.msim_f4_live_compact_workspace_bytes(3, bounce.numel()), dtype=torch.uint8, device=DEV)
    rc = L.msim_f4_live_compact(codes.data_ptr(), 160, scales.data_ptr(), 9, bad.data_ptr(), alive.data_ptr(), 3, used.data_ptr(),
                                ws.data_ptr(), bounce.data_ptr(), bounce.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(ws[:4].view(torch.int32)[0]) == 1 and int(used[0]) == 9
    assert torch.equal(keep[0], codes) and torch.equal(keep[1], scales) and bad.tolist() == [0, 5, 3, 9]


# ------------------------------------------------------------------------------------------------------------- random history
class Model:
    """What the live corpus must be equal to: the pages by slot, and who survives."""

    def __init__(self, amd, live, dim):
        self.amd, self.live, self.dim = amd, live, dim
        self.pages, self.table = [], lt.SlotTable(live.id_base)

    def add(self, pages, on_device=False):
        got = self.live.add(torch.stack(pages).to(DEV) if on_device else pages)
        assert got.tolist() == self.table.add([len(p) for p in pages])
        self.pages += pages

    def delete(self, ids, on_device=False):
        self.live.delete(torch.tensor(ids, dtype=torch.int64, device=DEV) if on_device else ids)
        known = [i for i in dict.fromkeys(ids) if 0 <= i - self.live.id_base < len(self.pages)]     # the device form ignores the rest
        self.table.delete([i for i in known if self.table.alive[i - self.live.id_base]])

    def compact(self):
        self.live.compact()
        self.table.compact()

    def packed(self):
        surv = self.table.survivors()
        return (self.amd.pack_passages([self.pages[s] for s in surv], DEV, batch_size=None) if surv else None), surv

    def check(self, queries, k, n_candidates=6, **live_kw):
        amd, live, cls = self.amd, self.live, _index_cls(self.amd, self.dim)
        assert live.rows_used == self.table.rows_used and len(live) == len(self.pages)
        np.testing.assert_array_equal(live.view().offsets.cpu().numpy(), self.table.offsets())
        idx = live.fp4_index()
        _same_index(live, idx, cls.build(live.view()))
        F, surv = self.packed()
        for q in queries:
            got = live.search(q, k, prefilter=idx, n_candidates=n_candidates)
            if F is None:
                assert np.isneginf(got[0].cpu().numpy()).all() and (got[1].cpu().numpy() == -1).all()
                continue
            want = amd.ShardedRetriever(F, **live_kw).search(q, k, prefilter=cls.build(F), n_candidates=n_candidates)
            _same(got, want, surv, live.id_base)
        live.check()


@pytest.mark.parametrize("dtype,dim,bounce_rows", [(torch.bfloat16, 128, None), (torch.float16, 128, 7), (torch.bfloat16, 320, 5)])
def test_a_random_history_keeps_the_index_equal_to_a_fresh_build(amd, dtype, dim, bounce_rows):
    g = torch.Generator().manual_seed(2000 + dim + (0 if dtype == torch.bfloat16 else 1))
    live = amd.LiveCorpus(9000, 400, DEV, dtype=dtype, width=dim, id_base=50,
                          bounce_bytes=None if bounce_rows is None else bounce_rows * dim * 2)
    m = Model(amd, live, dim)
    qs4 = [_rows(g, n, dim, dtype) for n in (32, 5, 17, 32)]
    qs40 = [_rows(g, int(n), dim, dtype) for n in torch.randint(1, 40, (40,), generator=g)]
    queries = [amd.pack_queries(qs4, DEV), amd.pack_queries(qs40, DEV)]

    def lens(n):
        return [int(x) for x in torch.randint(1, 90, (n,), generator=g)]

    m.add([_rows(g, n, dim, dtype) for n in [1, 40, 1, 2100] + lens(8)])                 # 1-row pages, one page above 2048 rows
    m.check(queries, 10)
    for _ in range(40):
        op = int(torch.randint(0, 10, (1,), generator=g))
        alive_ids = [s + live.id_base for s in m.table.survivors()]
        if op < 3 and len(m.pages) < 380 and live.rows_used < 6000:
            if op == 0:
                per = int(torch.randint(1, 30, (1,), generator=g))
                m.add([_rows(g, per, dim, dtype) for _ in range(3)], on_device=True)      # a [n, rows, width] device tensor
            else:
                m.add([_rows(g, n, dim, dtype) for n in lens(int(torch.randint(1, 6, (1,), generator=g)))])
        elif op < 7 and alive_ids:
            pick = torch.randperm(len(alive_ids), generator=g)[:int(torch.randint(1, 5, (1,), generator=g))].tolist()
            ids = [alive_ids[p] for p in pick]
            if op == 6:
                m.delete(ids + [7, 10_000, ids[0]], on_device=True)                       # foreign ids and a repeat: ignored
            else:
                m.delete(ids)
        else:
            m.compact()
        m.check(queries, 10)
    m.compact()
    m.check(queries, 500)                                                                 # k above the number of live pages
    if m.table.survivors():
        m.delete([s + live.id_base for s in m.table.survivors()])                         # delete everything ...
    m.check(queries, 10)
    m.compact()
    assert live.rows_used == 0
    m.check(queries, 10)
    m.add([_rows(g, n, dim, dtype) for n in lens(4)])                                     # ... then add again: new ids, rows from 0
    m.check(queries, 10)


# --------------------------------------------------------------------------------------------------------- order of first use
@pytest.mark.parametrize("dim", [128, 320])
def test_order_of_first_use_and_drop(amd, dim):
    g = torch.Generator().manual_seed(12 + dim)
    cls = _index_cls(amd, dim)
    pq = amd.pack_queries([_rows(g, n, dim) for n in (32, 7)], DEV)
    live = amd.LiveCorpus(3000, 40, DEV, width=dim, id_base=3)
    idx = live.fp4_index()                                                                # before any add
    assert isinstance(idx, cls) and len(idx) == 0
    s, i = live.search(pq, 5, prefilter=idx, n_candidates=3)
    assert np.isneginf(s.cpu().numpy()).all() and (i.cpu().numpy() == -1).all()
    live.add([_rows(g, int(n), dim) for n in torch.randint(1, 90, (20,), generator=g)])
    _same_index(live, live.fp4_index(), cls.build(live.view()))

    late = amd.LiveCorpus(3000, 40, DEV, width=dim, id_base=3)                            # after deletes, before compact
    late.add([_rows(g, int(n), dim) for n in torch.randint(1, 90, (20,), generator=g)])
    late.delete([4, 5, 11, 22])
    rows = late.rows_used
    idx = late.fp4_index()
    assert idx.codes.shape[0] == rows                                                     # over the view: dead rows included
    _same_index(late, idx, cls.build(late.view()))
    late.compact()
    assert late.rows_used < rows
    idx = late.fp4_index()
    _same_index(late, idx, cls.build(late.view()))
    keep = idx.codes.clone(), idx.scales.clone()
    late.drop_fp4_index()
    late.drop_fp4_index()                                                                 # nothing left to drop: a no-op
    again = late.fp4_index()
    assert torch.equal(again.codes, keep[0]) and torch.equal(again.scales, keep[1])
    late.check()


def test_int8_and_fp4_indexes_both_kept_in_step(amd):
    g = torch.Generator().manual_seed(21)
    live = amd.LiveCorpus(6000, 80, DEV, bounce_bytes=9 * 256)
    live.add([_rows(g, int(n)) for n in torch.randint(1, 120, (30,), generator=g)])
    live.int8_index()
    live.fp4_index()

    def both():
        i8, want8 = live.int8_index(), amd.Int8Index.build(live.view())
        assert torch.equal(i8.codes[:live.rows_used], want8.codes[:live.rows_used])
        np.testing.assert_array_equal(_bits(i8.scales), _bits(want8.scales))
        _same_index(live, live.fp4_index(), amd.Fp4Index.build(live.view()))
        live.check()

    both()
    live.delete([0, 7, 8, 29])
    live.compact()
    both()
    live.add(torch.stack([_rows(g, 13) for _ in range(5)]).to(DEV))
    live.delete(torch.tensor([31, 2, 500], dtype=torch.int64, device=DEV))
    both()
    live.compact()
    both()
    live.add([_rows(g, int(n)) for n in torch.randint(1, 120, (10,), generator=g)])
    both()


def _shard_with_deletes(amd, g, n_pages=60, **kw):
    pages = [_rows(g, int(n)) for n in torch.randint(1, 120, (n_pages,), generator=g)]
    gone = [3, 4, 17, 40, 59]
    live = amd.LiveCorpus(8000, n_pages + 4, DEV, **kw)
    live.add(pages)
    live.fp4_index()
    live.delete(gone)
    surv = [s for s in range(n_pages) if s not in gone]
    return live, pages, surv, amd.pack_passages([pages[s] for s in surv], DEV, batch_size=None)


def test_fp6_queries_as_the_fp4_hook(amd):
    g = torch.Generator().manual_seed(31)
    live, _, surv, F = _shard_with_deletes(amd, g, fp4_score_fn=amd.fp6_scores)
    pq = amd.pack_queries([_rows(g, n) for n in (32, 9, 20)], DEV)
    ref = amd.ShardedRetriever(F, fp4_score_fn=amd.fp6_scores)
    for _ in range(2):                                                                    # before and after the compaction
        _same(live.search(pq, 10, prefilter=live.fp4_index(), n_candidates=8),
              ref.search(pq, 10, prefilter=amd.Fp4Index.build(F), n_candidates=8), surv)
        live.compact()
    live.check()


def test_filter_and_group_by_over_the_fp4_prefilter(amd):
    g = torch.Generator().manual_seed(32)
    live, _, surv, F = _shard_with_deletes(amd, g)
    pq = amd.pack_queries([_rows(g, n) for n in (32, 9, 20)], DEV)
    slot_mask = torch.rand(60, generator=g) > 0.4
    slot_labels = torch.randint(0, 6, (60,), generator=g) * 7 + 3
    ref, ref_idx = amd.ShardedRetriever(F), amd.Fp4Index.build(F)
    _same(live.search(pq, 5, prefilter=live.fp4_index(), n_candidates=8, filter=amd.PageFilter.from_mask(slot_mask.to(DEV), 0)),
          ref.search(pq, 5, prefilter=ref_idx, n_candidates=8, filter=amd.PageFilter.from_mask(slot_mask[surv].to(DEV), 0)), surv)
    _same(live.search(pq, 5, prefilter=live.fp4_index(), n_candidates=8, group_by=amd.PageGroups.from_labels(slot_labels.to(DEV), 0)),
          ref.search(pq, 5, prefilter=ref_idx, n_candidates=8, group_by=amd.PageGroups.from_labels(slot_labels[surv].to(DEV), 0)), surv)


def test_formats_the_fp4_index_refuses(amd):
    for dtype, dim in ((torch.float32, 100), (torch.bfloat16, 64)):
        live = amd.LiveCorpus(100, 4, DEV, dtype=dtype, width=dim)
        with pytest.raises(NotImplementedError, match="the fp4 index takes bfloat16 / float16 pages"):
            live.fp4_index()
        live.drop_fp4_index()


# -------------------------------------------------------------------------------------------------------------- graph capture
def test_captured_compact_and_fp4_search_replay_the_same_result(amd):
    g = torch.Generator().manual_seed(8)
    pq = amd.pack_queries([_rows(g, n) for n in (32, 9, 20)], DEV)
    state = torch.Generator().manual_seed(80)

    def fresh():
        state.manual_seed(80)
        return _shard_with_deletes(amd, state, bounce_bytes=64 * 256)                    # the index is requested outside the capture

    warm = fresh()[0]                                                                    # loads every kernel outside the capture
    warm.compact()
    eager = [t.clone() for t in warm.search(pq, 10, prefilter=warm.fp4_index(), n_candidates=8)]
    live, _, surv, F = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        live.compact()
        captured = live.search(pq, 10, prefilter=live.fp4_index(), n_candidates=8)
    for _ in range(3):                                                                   # the second and third compaction find nothing to move
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
    live.check()
    _same_index(live, live.fp4_index(), amd.Fp4Index.build(live.view()))
    _same(captured, amd.ShardedRetriever(F).search(pq, 10, prefilter=amd.Fp4Index.build(F), n_candidates=8), surv)
